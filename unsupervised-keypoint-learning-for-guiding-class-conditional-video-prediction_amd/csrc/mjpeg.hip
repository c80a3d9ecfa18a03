// Baseline JPEG scans of 8-bit RGB frames (include/kpx.h "Motion-JPEG"; evaluate.py --video, kpx_amd/mjpeg.py): colour transform, 4:2:0
// subsampling, 8 x 8 DCT, quantisation and Huffman coding on the device, so only compressed bytes cross to the host.  Integers only: the bytes
// are a function of the pixels and the tables, not of the grid or the order of execution (tests/mjpeg_ref.py is the numpy restatement).
//
// Three passes over a workspace, no atomics, nothing but kernel launches:
//   1. jpeg_transform_kernel   one workgroup per 16 x 16 MCU: 768 bytes of RGB through LDS -> six blocks of 64 zig-zag int16 coefficients
//   2. jpeg_entropy_kernel     one wavefront per restart interval (one row of MCUs).  64 blocks at a time: lane l codes block l into a bit
//                              string of its own in LDS and a wavefront prefix sum of the lengths gives every string its place; then lane l
//                              GATHERS output byte l, l + 64, ... from the strings that cover it, so every output byte has one writer and
//                              nothing is OR-ed across lanes; a ballot over the 0xFF bytes places the stuffed zeros.  The interval goes
//                              into a slab of its own (worst-case size), its length into `lens`.
//   3. jpeg_offsets_kernel, jpeg_pack_kernel   interval and frame offsets by integer sums in a fixed order, then the slabs are copied to
//                              their packed places with RSTm between them.
//
// The bound (kpx_jpeg_scan_bound).  Samples lie in [-128, 127], so a quantised DC lies in [-1024, 1016] (Q = 1) and a DC difference in
// [-2040, 2040]: category 11 at most, whose code is 9 bits (luma) / 11 bits (chroma) long in the Annex K tables: at most 11 + 11 = 22 bits.
// An AC coefficient is below 128 (sum_x |T[1][x]|)^2 / 2^26 = 841 in magnitude: category 10 at most, and the longest AC code has 16 bits:
// 26 bits for each of 63 coefficients, and then no EOB.  A block is therefore at most
// 22 + 63 * 26 = 1660 bits = 207.5 bytes; an interval of b blocks at most ceil(1660 b / 8) <= 208 b bytes before stuffing and 416 b after
// (every byte 0xFF).  Six blocks per MCU: 2496 bytes per MCU, 3.25 times its 768 bytes of RGB, plus two bytes of RSTm per MCU row but the last.
#include "kpx_common.h"

enum { JP_BLOCK_BITS = 1660, JP_BLOCK_BYTES = 208, JP_MCU_BOUND = 6 * 2 * JP_BLOCK_BYTES, JP_MIN = 16, JP_MAX = 4096,
       JP_STRIDE = 53 /* words per bit string: 52 of data, one of padding; odd, so the lanes' strings start on different banks */ };

// ---- ITU T.81 Annex K.3 - K.6 as (number of codes per length, symbols in code order); the canonical codes are built at compile time
struct JpegHuff {
    uint32_t dc[2][12];        // (length << 16) | code of a DC category; [0] luma, [1] chroma
    uint32_t ac[2][256];       // the same of an AC symbol run << 4 | category
};

struct JpegSpec {
    uint8_t bits[16];
    uint8_t vals[162];
};

constexpr JpegSpec JP_DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpegSpec JP_DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpegSpec JP_AC_LUMA = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr JpegSpec JP_AC_CHROMA = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

constexpr void jp_fill(uint32_t* out, const JpegSpec& s) {        // T.81 Annex C: codes of one length count up, the next length appends a 0
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) out[s.vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}
constexpr JpegHuff jp_build() {
    JpegHuff h = {};
    jp_fill(h.dc[0], JP_DC_LUMA);
    jp_fill(h.dc[1], JP_DC_CHROMA);
    jp_fill(h.ac[0], JP_AC_LUMA);
    jp_fill(h.ac[1], JP_AC_CHROMA);
    return h;
}
__device__ const JpegHuff jp_huff = jp_build();

// T[u][x] = rint(8192 alpha(u) cos((2x + 1) u pi / 16)), alpha(0) = sqrt(1/8), alpha(u) = 1/2
__device__ const int16_t jp_dct[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                                       3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                                       2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                                       1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
// the place in the scan of the coefficient at natural index v * 8 + u
__device__ const uint8_t jp_scan_pos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                            10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct JpegQuant { uint8_t q[2][64]; };

// ------------------------------------------------------------------------------------------------------------------ pass 1
// One workgroup of 256 threads per MCU; coef[mcu][6][64] int16 in scan order, mcu = (n * rows + my) * cols + mx.
__global__ __launch_bounds__(256) void jpeg_transform_kernel(const uint8_t* __restrict__ rgb, int H, int W, int wide, JpegQuant qt,
                                                             int16_t* __restrict__ coef) {
    __shared__ uint32_t raw[16 * 12];             // 16 rows of 48 bytes
    __shared__ int16_t S[6][64];                  // level-shifted samples: four Y blocks, Cb, Cr
    __shared__ uint8_t C[2][16][16];              // clamped full-resolution Cb, Cr
    __shared__ int32_t G[6][64];                  // rows transformed: G[b][y][u]
    __shared__ int16_t out[6 * 64];
    __shared__ int16_t T[64];
    const int t = threadIdx.x, cols = W >> 4, rows = H >> 4;
    const size_t mcu = blockIdx.x;
    const int mx = (int)(mcu % cols), my = (int)((mcu / cols) % rows);
    const size_t n = mcu / ((size_t)cols * rows);
    if (t < 64) T[t] = jp_dct[t];
    if (t < 192) {
        const int row = t / 12, word = t % 12;
        const uint8_t* p = rgb + ((n * H + (size_t)(my * 16 + row)) * W + (size_t)mx * 16) * 3 + word * 4;
        raw[t] = wide ? *(const uint32_t*)p : (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    __syncthreads();
    {
        const int y = t >> 4, x = t & 15;
        const uint8_t* px = (const uint8_t*)raw + y * 48 + x * 3;
        const int r = px[0], g = px[1], b = px[2];
        const int yy = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
        const int cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32768) >> 16;
        const int cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32768) >> 16;
        S[(y >> 3) * 2 + (x >> 3)][(y & 7) * 8 + (x & 7)] = (int16_t)(yy - 128);
        C[0][y][x] = (uint8_t)min(max(cb, 0), 255);
        C[1][y][x] = (uint8_t)min(max(cr, 0), 255);
    }
    __syncthreads();
    if (t < 128) {
        const int c = t >> 6, cy = (t >> 3) & 7, cx = t & 7;
        const int s = C[c][2 * cy][2 * cx] + C[c][2 * cy][2 * cx + 1] + C[c][2 * cy + 1][2 * cx] + C[c][2 * cy + 1][2 * cx + 1];
        S[4 + c][cy * 8 + cx] = (int16_t)(((s + 2) >> 2) - 128);
    }
    __syncthreads();
    for (int o = t; o < 384; o += 256) {          // G[b][y][u] = sum_x S[b][y][x] T[u][x]: |G| <= 8 * 128 * 4017 < 2^23
        const int b = o >> 6, y = (o >> 3) & 7, u = o & 7;
        int acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += (int)S[b][y * 8 + x] * (int)T[u * 8 + x];
        G[b][y * 8 + u] = acc;
    }
    __syncthreads();
    for (int o = t; o < 384; o += 256) {          // F[v][u] = sum_y T[v][y] G[b][y][u]: |F| < 2^38, exact in int64
        const int b = o >> 6, v = (o >> 3) & 7, u = o & 7;
        long long f = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) f += (long long)T[v * 8 + y] * (long long)G[b][y * 8 + u];
        const unsigned q = qt.q[b < 4 ? 0 : 1][v * 8 + u];
        const unsigned long long a = (unsigned long long)(f < 0 ? -f : f) + ((unsigned long long)q << 25);
        const int c = (int)((unsigned)(a >> 26) / q);          // floor((|F| + Q 2^25) / (Q 2^26)): one rounding, half away from zero
        out[b * 64 + jp_scan_pos[v * 8 + u]] = (int16_t)(f < 0 ? -c : c);
    }
    __syncthreads();
    if (t < 192) ((uint32_t*)(coef + mcu * 384))[t] = ((const uint32_t*)out)[t];
}

// ------------------------------------------------------------------------------------------------------------------ pass 2
struct JpegBits {                                  // MSB-first bits into 32-bit words of LDS (byte j of the string is bits 31-8(j%4).. of word j/4)
    uint32_t* w;
    unsigned long long acc;
    int n, words;
    __device__ __forceinline__ void put(uint32_t code, int len) {      // len <= 26, n < 32 on entry
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            w[words++] = (uint32_t)(acc >> n);
        }
    }
};

__device__ __forceinline__ void jp_value(int v, int& cat, uint32_t& extra) {
    cat = 32 - __clz(v < 0 ? -v : v);
    extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
}

// `need` bits (1..8) of the concatenation of the strings str[0..65) from bit p on; start[b] is the first bit of string b, start[65] = total.
// Past the end the bits are 1 (the padding of the last byte of an interval).
__device__ __forceinline__ uint32_t jp_gather(const uint32_t* str, const int* start, int total, int p, int need) {
    int lo = 0, hi = 65;                           // the last b with start[b] <= p (strings of no bits before it are skipped)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= p) lo = mid; else hi = mid;
    }
    int b = lo;
    uint32_t v = 0;
    while (need > 0 && p < total) {
        const int end = start[b + 1];
        if (end <= p) { ++b; continue; }
        const int take = min(need, end - p), q = p - start[b];
        const uint32_t* w = str + b * JP_STRIDE + (q >> 5);
        const unsigned long long two = ((unsigned long long)w[0] << 32) | w[1];       // w[1] may be the string's padding word: shifted out
        v = (v << take) | ((uint32_t)(two >> (64 - (q & 31) - take)) & ((1u << take) - 1u));
        p += take;
        need -= take;
    }
    return need > 0 ? (v << need) | ((1u << need) - 1u) : v;
}

// One wavefront per restart interval.  coef as pass 1 wrote it; slab: interval i owns bytes [i * cols * JP_MCU_BOUND, (i + 1) * ...).
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int cols, uint8_t* __restrict__ slabs,
                                                          int32_t* __restrict__ lens) {
    __shared__ uint32_t str[65 * JP_STRIDE];       // string 0: the bits (< 8) the last round left over; string 1 + l: lane l's block
    __shared__ int start[66];
    __shared__ uint32_t hdc[2][12], hac[2][256];
    const int lane = threadIdx.x;
    const size_t interval = blockIdx.x;
    const int nb = cols * 6;
    const int16_t* blocks = coef + interval * (size_t)nb * 64;
    uint8_t* slab = slabs + interval * (size_t)cols * JP_MCU_BOUND;
    if (lane < 24) hdc[lane / 12][lane % 12] = jp_huff.dc[lane / 12][lane % 12];
    for (int i = lane; i < 512; i += 64) hac[i >> 8][i & 255] = jp_huff.ac[i >> 8][i & 255];
    if (lane == 0) str[0] = 0;
    __syncthreads();
    int outpos = 0, carry = 0;                     // bytes written to the slab; bits waiting in string 0
    for (int c0 = 0; c0 < nb; c0 += 64) {
        const int blk = c0 + lane;
        int bits = 0;
        if (blk < nb) {
            const int mcu = blk / 6, k = blk % 6, tab = k < 4 ? 0 : 1;
            const int16_t* z = blocks + (size_t)blk * 64;
            int pred = 0;                          // the DC of the previous block of the same component in this interval
            if (k >= 1 && k <= 3) pred = z[-64];
            else if (mcu > 0) pred = z[k == 0 ? -3 * 64 : -6 * 64];
            JpegBits bw = {str + (1 + lane) * JP_STRIDE, 0ull, 0, 0};
            int cat;
            uint32_t extra;
            const int diff = (int)z[0] - pred;
            if (diff == 0) {
                bw.put(hdc[tab][0] & 0xffff, hdc[tab][0] >> 16);
            } else {
                jp_value(diff, cat, extra);
                const uint32_t h = hdc[tab][cat];
                bw.put(((h & 0xffff) << cat) | extra, (int)(h >> 16) + cat);
            }
            int run = 0;
            for (int i = 0; i < 8; ++i) {
                const uint4 v4 = ((const uint4*)z)[i];
                const uint32_t wv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (i == 0 && j == 0) continue;
                    const int v = (int)(int16_t)(wv[j >> 1] >> ((j & 1) * 16));
                    if (v == 0) { ++run; continue; }
                    while (run >= 16) {
                        bw.put(hac[tab][0xf0] & 0xffff, hac[tab][0xf0] >> 16);
                        run -= 16;
                    }
                    jp_value(v, cat, extra);
                    const uint32_t h = hac[tab][(run << 4) | cat];
                    bw.put(((h & 0xffff) << cat) | extra, (int)(h >> 16) + cat);
                    run = 0;
                }
            }
            if (run > 0) bw.put(hac[tab][0] & 0xffff, hac[tab][0] >> 16);      // EOB unless coefficient 63 is non-zero
            bits = bw.words * 32 + bw.n;
            if (bw.n > 0) bw.w[bw.words] = (uint32_t)(bw.acc << (32 - bw.n));
        }
        int incl = bits;                           // inclusive prefix sum of the lengths over the wavefront
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 0) { start[0] = 0; start[1] = carry; }
        start[lane + 2] = carry + incl;
        __syncthreads();
        const int total = start[65];
        const bool last = c0 + 64 >= nb;
        const int nout = last ? (total + 7) >> 3 : total >> 3;
        int ffs = 0;
        for (int base = 0; base < nout; base += 64) {
            const int j = base + lane;
            const bool have = j < nout;
            const uint32_t byte = have ? jp_gather(str, start, total, j * 8, 8) : 0u;
            const bool ff = have && byte == 0xffu;
            const unsigned long long m = __ballot(ff);
            const int pos = outpos + j + ffs + __popcll(m & ((1ull << lane) - 1ull));
            if (have) {
                slab[pos] = (uint8_t)byte;
                if (ff) slab[pos + 1] = 0;
            }
            ffs += __popcll(m);
        }
        outpos += nout + ffs;
        const int left = last ? 0 : total & 7;
        const uint32_t rest = left ? jp_gather(str, start, total, nout * 8, left) : 0u;
        __syncthreads();                           // every lane has read the strings before string 0 changes and the next round writes
        if (lane == 0) str[0] = left ? rest << (32 - left) : 0u;
        carry = left;
    }
    if (lane == 0) lens[interval] = outpos;
}

// ------------------------------------------------------------------------------------------------------------------ pass 3
// row_off[n][r]: where interval r starts inside frame n (its RSTm follows it); frame_len[n]
__global__ void jpeg_frame_kernel(const int32_t* __restrict__ lens, int N, int rows, int32_t* __restrict__ row_off, int64_t* __restrict__ frame_len) {
    const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= (size_t)N) return;
    int off = 0;
    for (int r = 0; r < rows; ++r) {
        row_off[n * rows + r] = off;
        off += lens[n * rows + r] + (r < rows - 1 ? 2 : 0);
    }
    frame_len[n] = off;
}

// offsets[0] = 0, offsets[n + 1] = offsets[n] + frame_len[n]: one workgroup, thread t owns a run of consecutive frames
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const int64_t* __restrict__ frame_len, int N, int64_t* __restrict__ offsets) {
    __shared__ long long part[256];
    const int t = threadIdx.x, per = (N + 255) / 256;
    const int lo = min(t * per, N), hi = min(lo + per, N);
    long long s = 0;
    for (int n = lo; n < hi; ++n) s += frame_len[n];
    part[t] = s;
    __syncthreads();
    long long before = 0;
    for (int i = 0; i < t; ++i) before += part[i];
    if (t == 0) offsets[0] = 0;
    for (int n = lo; n < hi; ++n) {
        before += frame_len[n];
        offsets[n + 1] = before;
    }
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint8_t* __restrict__ slabs, const int32_t* __restrict__ lens,
                                                        const int32_t* __restrict__ row_off, const int64_t* __restrict__ offsets, int rows, int cols,
                                                        uint8_t* __restrict__ scans) {
    const size_t interval = blockIdx.x;
    const int r = (int)(interval % rows), len = lens[interval];
    const uint8_t* src = slabs + interval * (size_t)cols * JP_MCU_BOUND;
    uint8_t* dst = scans + offsets[interval / rows] + row_off[interval];
    for (int i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
    if (r < rows - 1 && threadIdx.x < 2) dst[len + threadIdx.x] = threadIdx.x ? (uint8_t)(0xd0 + (r & 7)) : (uint8_t)0xff;
}

// ------------------------------------------------------------------------------------------------------------------ host
static bool jp_sizes_ok(long long N, int H, int W) {
    return N >= 1 && H >= JP_MIN && W >= JP_MIN && H <= JP_MAX && W <= JP_MAX && H % 16 == 0 && W % 16 == 0 && N * H * W < (1ll << 31);
}

static size_t jp_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct JpegPlan { size_t coef, slabs, lens, row_off, frame_len, total; };

static JpegPlan jp_plan(int N, int H, int W) {
    const size_t mcus = (size_t)N * (H / 16) * (W / 16), intervals = (size_t)N * (H / 16);
    JpegPlan p;
    p.coef = 0;
    p.slabs = jp_align(p.coef + mcus * 384 * sizeof(int16_t));
    p.lens = jp_align(p.slabs + mcus * JP_MCU_BOUND);
    p.row_off = jp_align(p.lens + intervals * sizeof(int32_t));
    p.frame_len = jp_align(p.row_off + intervals * sizeof(int32_t));
    p.total = jp_align(p.frame_len + (size_t)N * sizeof(int64_t));
    return p;
}

extern "C" size_t kpx_jpeg_scan_bound(int H, int W) {
    if (!jp_sizes_ok(1, H, W)) return 0;
    return (size_t)(H / 16) * (W / 16) * JP_MCU_BOUND + 2 * (size_t)(H / 16 - 1);
}

extern "C" size_t kpx_jpeg_workspace_bytes(int N, int H, int W) {
    return jp_sizes_ok(N, H, W) ? jp_plan(N, H, W).total : 0;
}

extern "C" int kpx_jpeg_encode_u8(const uint8_t* rgb, int N, int H, int W, const uint8_t* qtables, uint8_t* scans, int64_t* offsets,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (!rgb || !qtables || !scans || !offsets || !workspace || !jp_sizes_ok(N, H, W)) return KPX_EINVAL;
    if (((uintptr_t)offsets & 7) || ((uintptr_t)workspace & 7)) return KPX_EINVAL;
    const JpegPlan p = jp_plan(N, H, W);
    if (workspace_bytes < p.total) return KPX_EINVAL;
    JpegQuant qt;
    for (int i = 0; i < 128; ++i) {
        if (qtables[i] == 0) return KPX_EINVAL;
        qt.q[i >> 6][i & 63] = qtables[i];
    }
    hipStream_t st = kpx_stream(stream);
    uint8_t* ws = (uint8_t*)workspace;
    int16_t* coef = (int16_t*)(ws + p.coef);
    uint8_t* slabs = ws + p.slabs;
    int32_t *lens = (int32_t*)(ws + p.lens), *row_off = (int32_t*)(ws + p.row_off);
    int64_t* frame_len = (int64_t*)(ws + p.frame_len);
    const int rows = H / 16, cols = W / 16;
    const unsigned mcus = (unsigned)((size_t)N * rows * cols), intervals = (unsigned)((size_t)N * rows);       // < 2^23: N H W < 2^31
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3(mcus), dim3(256), 0, st, rgb, H, W, ((uintptr_t)rgb & 3) == 0 ? 1 : 0, qt, coef);
    int rc = kpx_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(intervals), dim3(64), 0, st, coef, cols, slabs, lens);
    if ((rc = kpx_launch_status())) return rc;
    hipLaunchKernelGGL(jpeg_frame_kernel, dim3((N + 255) / 256), dim3(256), 0, st, lens, N, rows, row_off, frame_len);
    if ((rc = kpx_launch_status())) return rc;
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, st, frame_len, N, offsets);
    if ((rc = kpx_launch_status())) return rc;
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(intervals), dim3(256), 0, st, slabs, lens, row_off, offsets, rows, cols, scans);
    return kpx_launch_status();
}
