// Animated GIFs of rollouts (evaluate.py --gif): colour statistics and the nearest-palette-colour search on the device, LZW on the host.
// DESIGN.md section 4.4.  All arithmetic is integer: every result is the same bits in any order of execution.
//
// kpx_color_hist_add_u32: hist[g, cell] += (count, sum r, sum g, sum b) over the pixels of group g, cell = the 5-5-5 cell of the pixel.
//   A group's histogram is 512 KB, a CU has 160 KB of LDS: a workgroup keeps the QUARTER of the cells with cell & 3 == blockIdx.y (8192 cells
//   of two 64-bit words, count | sum r << 32 and sum g | sum b << 32: 128 KB) and reads its chunk of the pixels whole, adding those of its
//   quarter with two 64-bit LDS atomics; the low bits of blue pick the quarter, so dark and bright images alike spread over the four.  A step
//   in which all 64 pixels of a wavefront fall into one cell -- the black background of a key-point canvas, flat areas -- touches no memory:
//   each lane adds into registers, and the run is reduced across the wavefront and added once when the cell changes.  At the end the
//   workgroup adds its occupied cells to hist with global integer atomics: at most 4 x 8192 per workgroup, a few per cent of them in practice.
//
// kpx_palette_map_u8: idx = the first nearest palette entry of every pixel.  The squared distance |c|^2 - 2 c.p + |p|^2 has the same
//   argmin as k_j = 256 (|p_j|^2 - 2 c.p_j) + j, whose minimum also carries the lowest j among equal distances in its low byte.  The
//   workgroup puts (-512 pr, -512 pg, -512 pb, 256 |p|^2 + j) of its group's palette into LDS once; a candidate is then one 16-byte LDS
//   read, the same address in every lane (a broadcast), and per pixel three 24-bit multiply-adds and a minimum.  A lane holds 8 pixels, so
//   the read is shared by 32 VALU instructions.  Pixels are read and indices written byte by byte (any base address, any width): 32 byte
//   accesses against 8 x 4 x P arithmetic instructions per lane.
#include "kpx_common.h"
#include "gif_lzw.h"

namespace {

constexpr int CH_THREADS = 1024;
constexpr int CH_SLOTS = 8192;                                         // cells of one quarter
constexpr int CH_LDS_BYTES = CH_SLOTS * 2 * 8;                         // 128 KB
constexpr unsigned CH_MAX_PIXELS = 1u << 24;                           // 255 * 2^24 < 2^32: the sums cannot overflow
constexpr unsigned CH_CHUNK = 65536;                                   // pixels a workgroup reads, unless that makes too many workgroups
constexpr int CH_TARGET_BLOCKS = 1024;
constexpr int CH_UNROLL = 4;                                          // pixels of a lane per step

__device__ __forceinline__ unsigned ch_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

__global__ __launch_bounds__(CH_THREADS) void color_hist_kernel(const uint8_t* __restrict__ rgb, unsigned n, unsigned chunk,
                                                                uint32_t* __restrict__ hist) {
    extern __shared__ unsigned long long ch_lds[];                     // [CH_SLOTS][2]
    const int quarter = blockIdx.y, grp = blockIdx.z;
    for (int i = threadIdx.x; i < CH_SLOTS * 2; i += CH_THREADS) ch_lds[i] = 0ull;
    __syncthreads();
    const uint8_t* src = rgb + (size_t)grp * n * 3;
    const unsigned long long begin64 = (unsigned long long)blockIdx.x * chunk;
    const unsigned begin = begin64 < n ? (unsigned)begin64 : n;
    const unsigned end = n - begin < chunk ? n : begin + chunk;
    const unsigned lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63u;
    int run_cell = -1;                                                 // wave-uniform: the cell the registers below belong to
    unsigned run_n = 0, run_r = 0, run_g = 0, run_b = 0;
    auto flush = [&]() {                                               // wave-uniform control flow
        if (run_cell < 0) return;
        const unsigned cn = ch_wave_sum(run_n), cr = ch_wave_sum(run_r), cg = ch_wave_sum(run_g), cb = ch_wave_sum(run_b);
        if (lane == 0 && cn) {
            atomicAdd(&ch_lds[(run_cell >> 2) * 2], (unsigned long long)cn | ((unsigned long long)cr << 32));
            atomicAdd(&ch_lds[(run_cell >> 2) * 2 + 1], (unsigned long long)cg | ((unsigned long long)cb << 32));
        }
        run_n = run_r = run_g = run_b = 0;
    };
    for (unsigned base = begin + wave0; base < end; base += CH_UNROLL * CH_THREADS) {   // base is wave-uniform, and base + 4 * 1024 < 2^25
        unsigned r[CH_UNROLL], g[CH_UNROLL], b[CH_UNROLL];
#pragma unroll
        for (int u = 0; u < CH_UNROLL; ++u) {                          // every load of the step in flight before the first is used
            const unsigned p = base + u * CH_THREADS + lane;
            r[u] = g[u] = b[u] = 0;
            if (p < end) {
                const uint8_t* s = src + (size_t)p * 3;
                r[u] = s[0]; g[u] = s[1]; b[u] = s[2];
            }
        }
#pragma unroll
        for (int u = 0; u < CH_UNROLL; ++u) {
            if (base + u * CH_THREADS >= end) break;                   // wave-uniform; below it lane 0 is valid
            const bool valid = base + u * CH_THREADS + lane < end;
            const int cell = (int)(((r[u] >> 3) << 10) | ((g[u] >> 3) << 5) | (b[u] >> 3));
            const int first = __builtin_amdgcn_readfirstlane(cell);
            if (__all(valid && cell == first)) {
                if ((first & 3) == quarter) {
                    if (first != run_cell) {
                        flush();
                        run_cell = first;
                    }
                    run_n += 1; run_r += r[u]; run_g += g[u]; run_b += b[u];
                }
            } else if (valid && (cell & 3) == quarter) {
                atomicAdd(&ch_lds[(cell >> 2) * 2], 1ull | ((unsigned long long)r[u] << 32));
                atomicAdd(&ch_lds[(cell >> 2) * 2 + 1], (unsigned long long)g[u] | ((unsigned long long)b[u] << 32));
            }
        }
    }
    flush();
    __syncthreads();
    uint32_t* h = hist + (size_t)grp * 32768 * 4;
    for (int i = threadIdx.x; i < CH_SLOTS; i += CH_THREADS) {
        const unsigned long long a = ch_lds[2 * i], c = ch_lds[2 * i + 1];
        if ((uint32_t)a) {
            uint32_t* o = h + (size_t)((i << 2) | quarter) * 4;
            atomicAdd(o, (uint32_t)a);
            atomicAdd(o + 1, (uint32_t)(a >> 32));
            atomicAdd(o + 2, (uint32_t)c);
            atomicAdd(o + 3, (uint32_t)(c >> 32));
        }
    }
}

constexpr int PM_THREADS = 256;
constexpr int PM_PIX = 8;                                              // pixels of a lane
constexpr int PM_MAX_BLOCKS_X = 4096;
constexpr unsigned long long PM_BAYER = 0x5D7F91B36E4CA280ull;         // nibble 4 y + x = M[y][x], M = [[0,8,2,10],[12,4,14,6],[3,11,1,9],[15,7,13,5]]

__global__ __launch_bounds__(PM_THREADS) void palette_map_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ palette,
                                                                 const int* __restrict__ sizes, int pmax, size_t npix, int H, int Wc, int amp,
                                                                 uint8_t* __restrict__ idx) {
    __shared__ int4 tab[256];
    const int grp = blockIdx.y;
    int P = sizes[grp];
    P = P < 1 ? 1 : P > pmax ? pmax : P;                               // never past the table, whatever the buffer holds
    if ((int)threadIdx.x < P) {
        const uint8_t* e = palette + ((size_t)grp * 256 + threadIdx.x) * 3;
        const int pr = e[0], pg = e[1], pb = e[2];
        tab[threadIdx.x] = make_int4(-512 * pr, -512 * pg, -512 * pb, (pr * pr + pg * pg + pb * pb) * 256 + (int)threadIdx.x);
    }
    __syncthreads();
    const uint8_t* src = rgb + (size_t)grp * npix * 3;
    uint8_t* dst = idx + (size_t)grp * npix;
    constexpr unsigned TILE = PM_THREADS * PM_PIX;
    const unsigned np = (unsigned)npix;                                // < 2^31 (the entry checks): t0 + TILE never wraps
    for (unsigned t0 = blockIdx.x * TILE; t0 < np; t0 += gridDim.x * TILE) {
        const unsigned p0 = t0 + threadIdx.x * PM_PIX;
        int r[PM_PIX], g[PM_PIX], b[PM_PIX], best[PM_PIX];
        unsigned x = 0, y = 0;                                         // ordered dither: x the column of the canvas, y the row of the frame
        if (amp) {
            const unsigned line = p0 / (unsigned)Wc;
            x = p0 - line * (unsigned)Wc;
            y = line % (unsigned)H;
        }
#pragma unroll
        for (int e = 0; e < PM_PIX; ++e) {
            r[e] = g[e] = b[e] = 0;
            best[e] = 0x7fffffff;
            if (p0 + e < np) {
                const uint8_t* s = src + (size_t)(p0 + e) * 3;
                r[e] = s[0]; g[e] = s[1]; b[e] = s[2];
                if (amp) {
                    const int m = (int)((PM_BAYER >> (4 * (((y & 3) << 2) | (x & 3)))) & 15);
                    const int d = ((2 * m - 15) * amp + 16) >> 5;      // arithmetic shift
                    r[e] = min(max(r[e] + d, 0), 255);
                    g[e] = min(max(g[e] + d, 0), 255);
                    b[e] = min(max(b[e] + d, 0), 255);
                    if (++x == (unsigned)Wc) {
                        x = 0;
                        if (++y == (unsigned)H) y = 0;
                    }
                }
            }
        }
#pragma unroll 4
        for (int j = 0; j < P; ++j) {
            const int4 t = tab[j];
#pragma unroll
            for (int e = 0; e < PM_PIX; ++e) {
                const int k = __mul24(r[e], t.x) + (__mul24(g[e], t.y) + (__mul24(b[e], t.z) + t.w));
                best[e] = min(best[e], k);
            }
        }
#pragma unroll
        for (int e = 0; e < PM_PIX; ++e)
            if (p0 + e < np) dst[p0 + e] = (uint8_t)(best[e] & 255);
    }
}

std::atomic<unsigned long long> ch_attr_mask{0};

}  // namespace

extern "C" int kpx_color_hist_add_u32(const uint8_t* rgb, int G, size_t n, uint32_t* hist, void* stream) {
    if (!rgb || !hist || (((uintptr_t)hist) & 3) || G < 1 || G > 65535 || n < 1 || n > CH_MAX_PIXELS) return KPX_EINVAL;
    if (kpx_first_use_on_device(&ch_attr_mask)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(color_hist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CH_LDS_BYTES);
        if (e != hipSuccess) return -(int)e;
    }
    const unsigned nn = (unsigned)n;
    unsigned splits = (nn + CH_CHUNK - 1) / CH_CHUNK;
    const unsigned cap = CH_TARGET_BLOCKS / (4 * G) > 0 ? CH_TARGET_BLOCKS / (4 * G) : 1;
    if (splits > cap) splits = cap;
    const unsigned chunk = (nn + splits - 1) / splits;                 // splits * chunk >= n
    hipLaunchKernelGGL(color_hist_kernel, dim3(splits, 4, G), dim3(CH_THREADS), CH_LDS_BYTES, kpx_stream(stream), rgb, nn, chunk, hist);
    return kpx_launch_status();
}

extern "C" int kpx_palette_map_u8(const uint8_t* rgb, int G, int T, int H, int Wc, const uint8_t* palette, const int* sizes, int pmax, int dither,
                                  uint8_t* idx, void* stream) {
    if (!rgb || !palette || !sizes || !idx || (((uintptr_t)sizes) & 3) || G < 1 || G > 65535 || T < 1 || H < 1 || Wc < 1 || pmax < 1 || pmax > 256 ||
        dither < 0 || dither > 64)
        return KPX_EINVAL;
    if ((unsigned long long)T * H > 0x7fffffffULL || (unsigned long long)T * H * Wc > 0x7fffffffULL) return KPX_EINVAL;   // no overflow: T H < 2^31 first
    const unsigned long long npix = (unsigned long long)T * H * Wc;
    const unsigned long long tiles = (npix + PM_THREADS * PM_PIX - 1) / (PM_THREADS * PM_PIX);
    const unsigned bx = tiles > PM_MAX_BLOCKS_X ? PM_MAX_BLOCKS_X : (unsigned)tiles;
    hipLaunchKernelGGL(palette_map_kernel, dim3(bx, G), dim3(PM_THREADS), 0, kpx_stream(stream), rgb, palette, sizes, pmax, (size_t)npix, H, Wc, dither,
                       idx);
    return kpx_launch_status();
}

extern "C" size_t kpx_gif_lzw_bound(size_t n) { return kpx_lzw_bound(n); }

extern "C" int kpx_gif_lzw_u8(const uint8_t* idx, size_t n, int min_code_size, uint8_t* out, size_t out_bytes) {
    if (n > (size_t)1 << 30) return KPX_EINVAL;                        // the stream's size is returned as an int
    const long long w = kpx_lzw_encode(idx, n, min_code_size, out, out_bytes);
    return w < 0 ? KPX_EINVAL : (int)w;
}
