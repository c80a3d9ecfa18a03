// GIF's variable-width LZW on palette indices: plain C++, host only, no HIP includes (a stand-alone program may include this file alone).
// DESIGN.md section 4.4 has the container; the rules, which tests/gif_ref.py restates:
//   clear = 1 << m (m = minimum code size, 2..8), end = clear + 1, first free code clear + 2, first width m + 1;
//   a clear code first; codes packed least significant bit first;
//   after a code is emitted: a full table (next free code 4096) emits a clear code and resets; otherwise the width grows by one when the
//   next free code equals 2^width, and the string (emitted code, next index) takes the next free code;
//   after the last code the same width rule, then the end code; an empty input is clear, end.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <new>

// bytes that hold the stream of any n indices: at most n + 2 codes of 12 bits plus one clear code per 3838 codes emitted
static inline size_t kpx_lzw_bound(size_t n) { return n + n / 2 + n / 1024 + 16; }

namespace kpx_lzw_detail {

constexpr int HASH_BITS = 14, HASH_SIZE = 1 << HASH_BITS;             // 4096 strings at most: load <= 1/4

struct Table {
    int32_t key[HASH_SIZE];                                           // (prefix << 8 | index) + 1; 0 = empty
    uint16_t code[HASH_SIZE];
    void clear() { memset(key, 0, sizeof(key)); }
    static unsigned slot(int32_t k) { return ((uint32_t)k * 2654435761u) >> (32 - HASH_BITS); }
    int find(int32_t k, unsigned* at) const {                          // -> the code of string k, or -1 and the slot to put it in
        unsigned h = slot(k);
        while (key[h]) {
            if (key[h] == k) return code[h];
            h = (h + 1) & (HASH_SIZE - 1);
        }
        *at = h;
        return -1;
    }
};

struct Bits {
    uint8_t* out;
    size_t cap, n;
    uint32_t acc;
    int have;
    bool ok;
    void put(unsigned code, int width) {
        acc |= (uint32_t)code << have;
        have += width;
        while (have >= 8) byte();
    }
    void byte() {
        if (n < cap) out[n] = (uint8_t)acc; else ok = false;
        ++n;
        acc >>= 8;
        have -= 8;
    }
    void flush() { if (have > 0) { have = 8; byte(); } }
};

}  // namespace kpx_lzw_detail

// idx[n] (every index < 1 << min_code) -> the LZW byte stream in out[out_bytes] (no sub-blocks).  Returns the bytes written; -1 for a null
// pointer, min_code outside 2..8, an index out of range, a stream that does not fit out_bytes (or an int), or no memory for the table.
static inline long long kpx_lzw_encode(const uint8_t* idx, size_t n, int min_code, uint8_t* out, size_t out_bytes) {
    using namespace kpx_lzw_detail;
    if ((!idx && n) || !out || min_code < 2 || min_code > 8) return -1;
    const unsigned clear = 1u << min_code, end = clear + 1;
    for (size_t i = 0; i < n; ++i)
        if (idx[i] >= clear) return -1;
    Table* t = new (std::nothrow) Table;
    if (!t) return -1;
    t->clear();
    Bits b{out, out_bytes, 0, 0, 0, true};
    unsigned next = end + 1;
    int width = min_code + 1;
    b.put(clear, width);
    if (n) {
        unsigned prefix = idx[0];
        for (size_t i = 1; i < n; ++i) {
            const unsigned k = idx[i];
            const int32_t key = (int32_t)((prefix << 8) | k) + 1;
            unsigned at = 0;
            const int found = t->find(key, &at);
            if (found >= 0) {
                prefix = (unsigned)found;
                continue;
            }
            b.put(prefix, width);
            if (next == 4096) {
                b.put(clear, width);
                t->clear();
                next = end + 1;
                width = min_code + 1;
            } else {
                if (next == (1u << width)) ++width;
                t->key[at] = key;
                t->code[at] = (uint16_t)next++;
            }
            prefix = k;
        }
        b.put(prefix, width);
        if (next == (1u << width) && width < 12) ++width;
    }
    b.put(end, width);
    b.flush();
    delete t;
    return b.ok ? (long long)b.n : -1;
}
