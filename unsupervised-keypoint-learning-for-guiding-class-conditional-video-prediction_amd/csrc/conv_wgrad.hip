// fp32 weight gradients of the convolutions for gfx950 (MI355X) on v_mfma_f32_32x32x2_f32 (exact f32 fma chain), and the entries that
// choose among every weight-gradient kernel of the library: kpx_conv2d_wgrad_f32 / kpx_conv2d_wgrad_bf16 / kpx_conv_image_wgrad_bf16.
// Replaces the TF-generated filter gradients of tf.layers.conv2d / tf.nn.conv2d of the reference (models/networks/layers.py:6-9,
// models/networks/vgg.py:51).  Four kernels live here, each with its plan:
//   conv_wgrad_kernel              any shape (scalar or 16-B loads, row-merged taps for image inputs)
//   conv_wgrad_tap_rows_kernel     Wo % 32 == 0: a K chunk is 32 consecutive pixels of one image row, so its addresses are wave-uniform
//   conv_wgrad_rows_kernel         small channel counts at high resolution: all taps of a row chunk from one LDS halo
//   conv_wgrad_rows_merged_kernel  the same for image inputs (Cin = 3)
// All of them split the pixel range over workgroups into partial slabs, summed in a fixed order by the reduce kernels below (finish_wgrad).
// wgrad_plan() below chooses among these four, conv_wsmall.hip, conv_wino.hip and conv_gemm3.hip (kpx_internal.h), for the entries and the host queries alike.
#include "kpx_internal.h"
#include "kpx_bf16.h"
#include <cassert>

// 16 zero bytes in the code object: invalid 16-B units are loaded from here.  Each translation unit that needs it has its own; the host
// side of the library already has conv_igemm.hip's shadow symbol of that name, so this one is defined for the device only.
#ifdef __HIP_DEVICE_COMPILE__
__device__ __attribute__((aligned(16))) float kpx_zero16[4] = {0.f, 0.f, 0.f, 0.f};
#else
extern __device__ float kpx_zero16[4];
#endif

// ------------------------------------------------------------------------------------------ wgrad, any shape
// dw[tap][c][k] = sum_p x[p shifted by tap][c] * dy[p][k]: GEMM with M = Cin, N = Cout, K = pixels.
// Both operands are pixel-major in memory, so the LDS tiles are plain [pixel][channel] copies of NHWC
// and the MFMA operands are ds_read_b32 (32 consecutive channels per half-wave, conflict-free).
// The pixel range is split over blocks (split-K); partial slabs are summed by wgrad_reduce_kernel in a
// fixed order, so the result is bitwise reproducible (no float atomics).

template <int BMc, int BNk, int WM, int WN, bool VEC, bool MERGE>
__global__ __launch_bounds__(WM * WN * 64) void conv_wgrad_kernel(const WgradGeom g) {
    constexpr int NT = WM * WN * 64;
    constexpr int BKP = 32;                          // pixels per K chunk
    constexpr int TM = BMc / (WM * 32), TN = BNk / (WN * 32);
    constexpr int RA = (BKP * BMc / 4) / NT, RB = (BKP * BNk / 4) / NT;     // float4 units per thread
    static_assert(RA >= 1 && RB >= 1 && TM >= 1 && TN >= 1, "tile/wave shape");
    __shared__ __attribute__((aligned(16))) float As[2][BKP * BMc];
    __shared__ __attribute__((aligned(16))) float Bs[2][BKP * BNk];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    int L = kpx_xcd_remap(blockIdx.x, gridDim.x);
    const int taps = g.KH * g.KW;
    const int kti = L % g.kt; L /= g.kt;
    const int cti = L % g.ct; L /= g.ct;
    const int tap = L % taps; L /= taps;
    const int split = L;
    const int r = tap / g.KW, q = tap - r * g.KW;
    const int cbase = cti * BMc, kbase = kti * BNk;
    const int pbeg = split * g.pps;
    const int pend = min(g.P, pbeg + g.pps);

    // per-thread loader coordinates: A unit -> (pixel-in-chunk, channel group)
    int apx[RA], ac[RA], an[RA], aho[RA], awo[RA], aq[RA][4];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int u = t + NT * i;
        apx[i] = u / (BMc / 4);
        ac[i] = cbase + (u % (BMc / 4)) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) aq[i][j] = MERGE ? (ac[i] + j) / g.merge : 0;
        const int p = pbeg + apx[i];
        an[i] = p / (g.Ho * g.Wo);
        const int rem = p - an[i] * g.Ho * g.Wo;
        aho[i] = rem / g.Wo;
        awo[i] = rem - aho[i] * g.Wo;
    }
    int bpx[RB], bk[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int u = t + NT * i;
        bpx[i] = u / (BNk / 4);
        bk[i] = kbase + (u % (BNk / 4)) * 4;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4 ra[RA], rb[RB];
    unsigned am[RA], bm[RB];
    int p0 = pbeg;
    auto tail4 = [](int c, int lim) -> unsigned {
        const int r_ = lim - c;
        return r_ >= 4 ? 15u : (r_ <= 0 ? 0u : (15u >> (4 - r_)));
    };
    // unconditional loads from a clamped address, masked when written to LDS (see conv_igemm_kernel)
    auto load_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int p = p0 + apx[i];
            const int ih = aho[i] * g.stride + r - g.pad_t, iw = awo[i] * g.stride + q - g.pad_l;
            const int c = ac[i];
            unsigned mask = 0;
            const float* ptr = g.x + ((ptrdiff_t)(an[i] * g.Hi + ih) * g.Wi + iw) * g.ldx + c;
            if (p < pend && (unsigned)ih < (unsigned)g.Hi) {
                if (MERGE) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c + j < g.Cin && (unsigned)(iw + aq[i][j]) < (unsigned)g.Wi) mask |= 1u << j;
                } else if ((unsigned)iw < (unsigned)g.Wi) {
                    mask = tail4(c, g.Cin);
                }
            }
            am[i] = mask;
            f32x4 v;
            if (VEC) {
                v = *reinterpret_cast<const f32x4*>(mask ? ptr : g.x);
            } else {
                v[0] = *((mask & 1u) ? ptr : g.x);
                v[1] = *((mask & 2u) ? ptr + 1 : g.x);
                v[2] = *((mask & 4u) ? ptr + 2 : g.x);
                v[3] = *((mask & 8u) ? ptr + 3 : g.x);
            }
            ra[i] = v;
            awo[i] += BKP;
            while (awo[i] >= g.Wo) {
                awo[i] -= g.Wo;
                if (++aho[i] == g.Ho) { aho[i] = 0; ++an[i]; }
            }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int p = p0 + bpx[i];
            const int k = bk[i];
            const unsigned mask = p < pend ? tail4(k, g.Cout) : 0u;
            const float* ptr = g.dy + (size_t)p * g.lddy + k;
            bm[i] = mask;
            f32x4 v;
            if (VEC) {
                v = *reinterpret_cast<const f32x4*>(mask ? ptr : g.dy);
            } else {
                v[0] = *((mask & 1u) ? ptr : g.dy);
                v[1] = *((mask & 2u) ? ptr + 1 : g.dy);
                v[2] = *((mask & 4u) ? ptr + 2 : g.dy);
                v[3] = *((mask & 8u) ? ptr + 3 : g.dy);
            }
            rb[i] = v;
        }
        p0 += BKP;
    };
    auto masked = [](f32x4 v, unsigned m) -> f32x4 {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (m >> j) & 1u ? v[j] : 0.f;
        return o;
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(&As[buf][(t + NT * i) * 4]) = masked(ra[i], am[i]);
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(&Bs[buf][(t + NT * i) * 4]) = masked(rb[i], bm[i]);
    };

    const int nchunks = pend > pbeg ? (pend - pbeg + BKP - 1) / BKP : 0;
    if (nchunks > 0) { load_chunk(); store_chunk(0); }
    __syncthreads();
    const int wrow = wm * TM * 32, wcol = wn * TN * 32;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < nchunks;
        if (more) load_chunk();
        const float* Ab = As[buf];
        const float* Bb = Bs[buf];
#pragma unroll
        for (int s2 = 0; s2 < BKP / 2; ++s2) {
            const int kp = 2 * s2 + lh;
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = Ab[kp * BMc + wrow + i * 32 + li];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bb[kp * BNk + wcol + j * 32 + li];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
    }

    float* out = g.out + (size_t)split * g.slab + (size_t)tap * g.Cin * g.Cout;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int k = kbase + wcol + j * 32 + li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = cbase + wrow + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (c < g.Cin && k < g.Cout) out[(size_t)c * g.Cout + k] = acc[i][j][e];
            }
    }
}

// Fast path of the per-tap wgrad for Wo % 32 == 0 (every generator layer at 32/64/128 pixels): a K chunk is 32 consecutive
// output pixels of ONE image row, so (n, ho, row validity, base addresses) are wave-uniform scalars and each thread only adds
// a fixed offset; invalid units read the zero page; chunk loop unrolled by two for immediate LDS buffer offsets.
struct WgradTapGeom {
    const float* x; const float* dy; float* out;
    int N, Hi, Wi, Cin, ldx;
    int Ho, Wo, Cout, lddy;
    int KH, KW, stride, pad_t, pad_l;
    int total_chunks, cpb, S, ct, kt;
    size_t slab;
};

template <int BMc, int BNk, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void conv_wgrad_tap_rows_kernel(const WgradTapGeom g) {
    constexpr int NT = WM * WN * 64, CW = 32;
    constexpr int TM = BMc / (WM * 32), TN = BNk / (WN * 32);
    constexpr int RA = (CW * BMc / 4) / NT, RB = (CW * BNk / 4) / NT;
    constexpr int ASZ = CW * BMc, BSZ = CW * BNk;
    static_assert(RA >= 1 && RB >= 1 && TM >= 1 && TN >= 1, "tile/wave shape");
    __shared__ __attribute__((aligned(16))) float As[2 * ASZ];
    __shared__ __attribute__((aligned(16))) float Bs[2 * BSZ];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    int L = kpx_xcd_remap(blockIdx.x, gridDim.x);
    const int taps = g.KH * g.KW;
    const int kti = L % g.kt; L /= g.kt;
    const int cti = L % g.ct; L /= g.ct;
    const int tap = L % taps; L /= taps;
    const int split = L;
    const int r = tap / g.KW, q = tap - r * g.KW;
    const int cbase = cti * BMc, kbase = kti * BNk;
    const int wpr = g.Wo / CW;
    const int cbeg = split * g.cpb, cend = min(g.total_chunks, cbeg + g.cpb);
    const int nch = cend > cbeg ? cend - cbeg : 0;

    // fixed per-thread parts
    int a_off[RA], a_px[RA];
    bool a_cok[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int u = t + NT * i;
        const int px = u / (BMc / 4), c = cbase + (u % (BMc / 4)) * 4;
        a_px[i] = px * g.stride;
        a_off[i] = px * g.stride * g.ldx + c;
        a_cok[i] = c < g.Cin;
    }
    int b_off[RB];
    bool b_kok[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int u = t + NT * i;
        const int px = u / (BNk / 4), kk = kbase + (u % (BNk / 4)) * 4;
        b_off[i] = px * g.lddy + kk;
        b_kok[i] = kk < g.Cout;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // wave-uniform chunk cursor
    int wc = cbeg % wpr, ho = (cbeg / wpr) % g.Ho, n = cbeg / (wpr * g.Ho);
    f32x4 ra[RA], rb[RB];
    auto load_chunk = [&]() {
        const int ih = ho * g.stride + r - g.pad_t;
        const int iwb = wc * CW * g.stride + q - g.pad_l;
        const bool rowok = (unsigned)ih < (unsigned)g.Hi;
        const float* xb = g.x + ((ptrdiff_t)(n * g.Hi + ih) * g.Wi + iwb) * g.ldx;
        const float* yb = g.dy + ((size_t)(n * g.Ho + ho) * g.Wo + wc * CW) * g.lddy;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const bool v = rowok && a_cok[i] && (unsigned)(iwb + a_px[i]) < (unsigned)g.Wi;
            ra[i] = *reinterpret_cast<const f32x4*>(v ? xb + a_off[i] : kpx_zero16);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i)
            rb[i] = *reinterpret_cast<const f32x4*>(b_kok[i] ? yb + b_off[i] : kpx_zero16);
        if (++wc == wpr) { wc = 0; if (++ho == g.Ho) { ho = 0; ++n; } }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(&As[buf * ASZ + (t + NT * i) * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(&Bs[buf * BSZ + (t + NT * i) * 4]) = rb[i];
    };
    const int wrow = wm * TM * 32, wcol = wn * TN * 32;
    const int a_rd = lh * BMc + wrow + li, b_rd = lh * BNk + wcol + li;
    auto mfma_steps = [&](int buf, int s0, int s1) {
#pragma unroll
        for (int s2 = s0; s2 < s1; ++s2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[buf * ASZ + a_rd + 2 * s2 * BMc + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[buf * BSZ + b_rd + 2 * s2 * BNk + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };
    auto chunk = [&](auto bufc, bool more) {
        constexpr int buf = decltype(bufc)::value;
        mfma_steps(buf, 0, 4);
        if (more) load_chunk();
        mfma_steps(buf, 4, 12);
        if (more) store_chunk(buf ^ 1);
        mfma_steps(buf, 12, 16);
        __syncthreads();
    };
    if (nch > 0) { load_chunk(); store_chunk(0); }
    __syncthreads();
    int ch = 0;
    for (; ch + 1 < nch; ch += 2) {
        chunk(kpx_ic<0>{}, true);
        chunk(kpx_ic<1>{}, ch + 2 < nch);
    }
    if (ch < nch) chunk(kpx_ic<0>{}, false);

    float* out = g.out + (size_t)split * g.slab + (size_t)tap * g.Cin * g.Cout;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int kk = kbase + wcol + j * 32 + li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = cbase + wrow + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (c < g.Cin && kk < g.Cout) out[(size_t)c * g.Cout + kk] = acc[i][j][e];
            }
    }
}

// dw[i] = sum_s ws[s][i] in a fixed order.  Two shapes of the same sum:
//  * few slabs (S <= 16: the discriminator's large filters, 8-34 M elements): a thread owns four consecutive elements (16-B accesses) and walks
//    the slabs in order with all loads of a group of eight in flight -- the 64-elements-per-workgroup form below moved 168 MB at 1.5 TB/s;
//  * many slabs: a workgroup owns 256 consecutive elements (four per lane), its 4 wavefronts stride over the slabs (1 KB per slab and wave),
//    8 loads in flight per lane, then a 4-way LDS combine in fixed order.
__global__ __launch_bounds__(256) void wgrad_reduce_few_kernel(const float* __restrict__ ws, float* __restrict__ dw, size_t n4, size_t n, int S) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 acc = *reinterpret_cast<const f32x4*>(ws + i * 4);
        int k = 1;
        for (; k + 7 < S; k += 8) {
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const f32x4*>(ws + (size_t)(k + j) * n + i * 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];
        }
        for (; k < S; ++k) acc += *reinterpret_cast<const f32x4*>(ws + (size_t)k * n + i * 4);
        *reinterpret_cast<f32x4*>(dw + i * 4) = acc;
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, size_t n, int S) {
    constexpr int W = VEC ? 4 : 1;
    typedef float vecw __attribute__((ext_vector_type(W)));
    const int e = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const size_t i = ((size_t)blockIdx.x * 64 + e) * W;
    vecw acc = 0.f;
    if (i < n) {
        int k = sg;
        for (; k + 28 < S; k += 32) {
            vecw v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const vecw*>(ws + (size_t)(k + 4 * j) * n + i);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];
        }
        for (; k < S; k += 4) acc += *reinterpret_cast<const vecw*>(ws + (size_t)k * n + i);
    }
    __shared__ vecw sm[4][64];
    sm[sg][e] = acc;
    __syncthreads();
    if (sg == 0 && i < n) *reinterpret_cast<vecw*>(dw + i) = (sm[0][e] + sm[1][e]) + (sm[2][e] + sm[3][e]);
}

static inline void launch_wgrad_reduce(const float* ws, float* dw, size_t n, int S, hipStream_t s) {
    const bool vec = n % 4 == 0 && (((uintptr_t)ws | (uintptr_t)dw) & 15) == 0;
    if (vec && S <= 16) {
        size_t nb = (n / 4 + 255) / 256; if (nb > 8192) nb = 8192;
        hipLaunchKernelGGL(wgrad_reduce_few_kernel, dim3((unsigned)nb), dim3(256), 0, s, ws, dw, n / 4, n, S);
    } else if (vec) {
        hipLaunchKernelGGL(wgrad_reduce_kernel<true>, dim3((unsigned)((n / 4 + 63) / 64)), dim3(256), 0, s, ws, dw, n, S);
    } else {
        hipLaunchKernelGGL(wgrad_reduce_kernel<false>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, ws, dw, n, S);
    }
}

// The tail of every weight-gradient launch.  rc: the status of the kernel that wrote dw itself (S == 1) or S partial slabs of n floats into
// the workspace ws, which the fixed-order reduce then sums into dw.
static int finish_wgrad(int rc, const void* ws, float* dw, size_t n, int S, hipStream_t s) {
    if (rc || S <= 1) return rc;
    launch_wgrad_reduce((const float*)ws, dw, n, S, s);
    return kpx_launch_status();
}

// ------------------------------------------------------------------------------------------ wgrad, small channel counts
// High-resolution layers with <= 64 input and <= 32 output channels (pose_encoder tail, translator head, encoder conv_2):
// the generic kernel above gives every filter tap its own workgroups, so x and dy are re-read KH*KW times and most of each
// 64x64 MFMA tile is padding.  Here one workgroup walks chunks of 32 consecutive output pixels of one image row, stages
// the KH x (32+KW-1) input halo and the 32 dy pixels ONCE in LDS, and its 4 wavefronts split the taps (wave w owns taps
// w, w+4, w+8), each tap a 32*CT x 32 accumulator.  Partial slabs per workgroup, same fixed-order reduce.
struct WgradRowsGeom {
    const float* x; const float* dy; float* out;
    int N, Hi, Wi, Cin, ldx;
    int Ho, Wo, Cout, lddy;
    int KH, KW, pad_t, pad_l;
    int total_chunks, cpb, ct;
    size_t slab;
};

template <int CT>
__global__ __launch_bounds__(256) void conv_wgrad_rows_kernel(const WgradRowsGeom g) {
    constexpr int CW = 32, HALO = CW + 2, CinT = 32 * CT, CoutT = 32;
    constexpr int XU = 3 * HALO * (CinT / 4);          // x float4 units per chunk (3 rows max)
    constexpr int RX = (XU + 255) / 256;
    constexpr int RY = (CW * CoutT / 4) / 256;         // = 1
    __shared__ __attribute__((aligned(16))) float xs[2][3 * HALO * CinT];
    __shared__ __attribute__((aligned(16))) float dys[2][CW * CoutT];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int L = kpx_xcd_remap(blockIdx.x, gridDim.x);
    const int cti = L % g.ct; L /= g.ct;
    const int split = L;
    const int cbase = cti * CinT;
    const int T = g.KH * g.KW;
    const int wpr = g.Wo / CW;                          // chunks per output row
    const int cbeg = split * g.cpb, cend = min(g.total_chunks, cbeg + g.cpb);

    f32x16 acc[3][CT];
#pragma unroll
    for (int sl = 0; sl < 3; ++sl)
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[sl][i][e] = 0.f;

    f32x4 rx[RX], ry[RY];
    unsigned mx[RX], my[RY];
    auto load_chunk = [&](int chunk) {
        const int wc = chunk % wpr, rest = chunk / wpr, ho = rest % g.Ho, n = rest / g.Ho;
#pragma unroll
        for (int i = 0; i < RX; ++i) {
            const int u = t + 256 * i;
            const int c4 = u % (CinT / 4), col = (u / (CinT / 4)) % HALO, r = u / ((CinT / 4) * HALO);
            const int ih = ho + r - g.pad_t, iw = wc * CW + col - g.pad_l, c = cbase + c4 * 4;
            unsigned mask = 0;
            if (u < XU && r < g.KH && (unsigned)ih < (unsigned)g.Hi && (unsigned)iw < (unsigned)g.Wi && c < g.Cin) {
                const int rem = g.Cin - c;
                mask = rem >= 4 ? 15u : (15u >> (4 - rem));
            }
            const float* p = g.x + ((ptrdiff_t)(n * g.Hi + ih) * g.Wi + iw) * g.ldx + c;
            mx[i] = mask;
            rx[i] = *reinterpret_cast<const f32x4*>(mask ? p : g.x);
        }
#pragma unroll
        for (int i = 0; i < RY; ++i) {
            const int u = t + 256 * i;
            const int k4 = u % (CoutT / 4), px = u / (CoutT / 4);
            const int k = k4 * 4;
            unsigned mask = 0;
            if (k < g.Cout) { const int rem = g.Cout - k; mask = rem >= 4 ? 15u : (15u >> (4 - rem)); }
            const float* p = g.dy + ((size_t)(n * g.Ho + ho) * g.Wo + wc * CW + px) * g.lddy + k;
            my[i] = mask;
            ry[i] = *reinterpret_cast<const f32x4*>(mask ? p : g.dy);
        }
    };
    auto masked = [](f32x4 v, unsigned m) -> f32x4 {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (m >> j) & 1u ? v[j] : 0.f;
        return o;
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < RX; ++i) {
            const int u = t + 256 * i;
            if (u < XU) *reinterpret_cast<f32x4*>(&xs[buf][u * 4]) = masked(rx[i], mx[i]);
        }
#pragma unroll
        for (int i = 0; i < RY; ++i) *reinterpret_cast<f32x4*>(&dys[buf][(t + 256 * i) * 4]) = masked(ry[i], my[i]);
    };

    const int nch = cend > cbeg ? cend - cbeg : 0;
    if (nch > 0) { load_chunk(cbeg); store_chunk(0); }
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < nch;
        if (more) load_chunk(cbeg + ch + 1);
        const float* X = xs[buf];
        const float* Y = dys[buf];
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) {
            const int tap = wave + 4 * sl;
            if (tap < T) {
                const int r = tap / g.KW, q = tap - r * g.KW;
                const float* Xr = X + (r * HALO + q) * CinT;
#pragma unroll
                for (int s2 = 0; s2 < CW / 2; ++s2) {
                    const int kp = 2 * s2 + lh;
                    const float b = Y[kp * CoutT + li];
#pragma unroll
                    for (int i = 0; i < CT; ++i)
                        acc[sl][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(Xr[kp * CinT + i * 32 + li], b, acc[sl][i], 0, 0, 0);
                }
            }
        }
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
    }

    float* out = g.out + (size_t)split * g.slab;
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
        const int tap = wave + 4 * sl;
        if (tap < T) {
#pragma unroll
            for (int i = 0; i < CT; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int c = cbase + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    if (c < g.Cin && li < g.Cout) out[((size_t)tap * g.Cin + c) * g.Cout + li] = acc[sl][i][e];
                }
        }
    }
}

// Same idea for the image-input convs (Cin = 3, 7x7): with dense NHWC the KW*Cin floats under one filter row are
// contiguous, so filter row r is ONE tap whose operand for output pixel p is the float window seg[r][p*Cin .. p*Cin+KW*Cin).
// The workgroup stages KH raw row segments of (32+KW-1)*Cin floats; wave w owns filter rows w and w+4.
template <int DUMMY>
__global__ __launch_bounds__(256) void conv_wgrad_rows_merged_kernel(const WgradRowsGeom g) {
    constexpr int CW = 32, SEG = 128, CoutT = 32, KHMAX = 8;
    constexpr int RX = KHMAX * SEG / 256;              // 4 scalar units per thread
    __shared__ float xs[2][KHMAX * SEG];
    __shared__ __attribute__((aligned(16))) float dys[2][CW * CoutT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int split = kpx_xcd_remap(blockIdx.x, gridDim.x);
    const int KWC = g.KW * g.Cin;                       // merged channels per filter row (<= 32)
    const int segf = (CW + g.KW - 1) * g.Cin;           // valid floats per staged row (<= SEG)
    const int wpr = g.Wo / CW;
    const int cbeg = split * g.cpb, cend = min(g.total_chunks, cbeg + g.cpb);

    f32x16 acc[2];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[sl][e] = 0.f;

    int xr[RX], xf[RX], xcol[RX];
#pragma unroll
    for (int i = 0; i < RX; ++i) {
        const int u = t + 256 * i;
        xr[i] = u / SEG; xf[i] = u % SEG; xcol[i] = xf[i] / g.Cin;
    }
    float rx[RX];
    f32x4 ry;
    unsigned my;
    auto load_chunk = [&](int chunk) {
        const int wc = chunk % wpr, rest = chunk / wpr, ho = rest % g.Ho, n = rest / g.Ho;
        const int iw0 = wc * CW - g.pad_l;
#pragma unroll
        for (int i = 0; i < RX; ++i) {
            const int ih = ho + xr[i] - g.pad_t;
            const bool ok = xr[i] < g.KH && xf[i] < segf && (unsigned)ih < (unsigned)g.Hi && (unsigned)(iw0 + xcol[i]) < (unsigned)g.Wi;
            const float* p = g.x + ((ptrdiff_t)(n * g.Hi + ih) * g.Wi + iw0) * g.Cin + xf[i];
            const float v = *(ok ? p : g.x);
            rx[i] = ok ? v : 0.f;
        }
        {
            const int k4 = t % (CoutT / 4), px = t / (CoutT / 4), k = k4 * 4;
            my = 0;
            if (k < g.Cout) { const int rem = g.Cout - k; my = rem >= 4 ? 15u : (15u >> (4 - rem)); }
            const float* p = g.dy + ((size_t)(n * g.Ho + ho) * g.Wo + wc * CW + px) * g.lddy + k;
            ry = *reinterpret_cast<const f32x4*>(my ? p : g.dy);
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < RX; ++i) xs[buf][t + 256 * i] = rx[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (my >> j) & 1u ? ry[j] : 0.f;
        *reinterpret_cast<f32x4*>(&dys[buf][t * 4]) = o;
    };
    const int nch = cend > cbeg ? cend - cbeg : 0;
    if (nch > 0) { load_chunk(cbeg); store_chunk(0); }
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < nch;
        if (more) load_chunk(cbeg + ch + 1);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            const int r = wave + 4 * sl;
            if (r < g.KH) {
                const float* Xr = &xs[buf][r * SEG];
#pragma unroll
                for (int s2 = 0; s2 < CW / 2; ++s2) {
                    const int kp = 2 * s2 + lh;
                    acc[sl] = __builtin_amdgcn_mfma_f32_32x32x2f32(Xr[kp * g.Cin + li], dys[buf][kp * CoutT + li], acc[sl], 0, 0, 0);
                }
            }
        }
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
    }
    float* out = g.out + (size_t)split * g.slab;
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        const int r = wave + 4 * sl;
        if (r < g.KH) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (c < KWC && li < g.Cout) out[((size_t)r * KWC + c) * g.Cout + li] = acc[sl][e];
            }
        }
    }
}

static bool wgrad_rows_merged_plan(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW, int* S, int* cpb) {
    if (Cin % 4 == 0 || KW * Cin > 32 || (32 + KW - 1) * Cin > 128 || KH > 8 || KW < 2 || Wo % 32 != 0 || Cout > 32 ||
        (long)N * Ho * Wo < 65536)
        return false;
    const long total = (long)N * Ho * (Wo / 32);
    long s = total < 768 ? total : 768;
    *cpb = (int)((total + s - 1) / s);
    *S = (int)((total + *cpb - 1) / *cpb);
    return true;
}

// shape-only eligibility + split plan of the rows kernel (alignment / stride are checked by the caller)
static bool wgrad_rows_plan(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW, int* S, int* cpb, int* CT) {
    if (KH > 3 || KW > 3 || KH * KW < 2 || Wo % 32 != 0 || Cout > 32 || Cin > 128 || (long)N * Ho * Wo < 65536) return false;
    *CT = Cin > 32 ? 2 : 1;
    const int ct = (Cin + 32 * *CT - 1) / (32 * *CT);
    const long total = (long)N * Ho * (Wo / 32);
    long want = 768 / ct;
    if (want < 1) want = 1;
    long s = total < want ? total : want;
    const size_t slab_bytes = (size_t)KH * KW * Cin * Cout * 4;
    const size_t cap = (size_t)256 << 20;
    if ((size_t)s * slab_bytes > cap) s = (long)(cap / slab_bytes);
    if (s < 1) s = 1;
    *cpb = (int)((total + s - 1) / s);
    *S = (int)((total + *cpb - 1) / *cpb);
    return true;
}

static void wgrad_tiles(int Cin, int Cout, int& bm, int& bn) {
    auto pick = [](int c) { return ((c + 127) / 128 * 128 == (c + 63) / 64 * 64) ? 128 : 64; };
    bm = pick(Cin); bn = pick(Cout);
    if (bm != bn) { bm = 64; bn = 64; }   // only the square tiles are instantiated
}

static inline bool wgrad_merge(int Cin, int ldx, int KW) { return Cin % 4 != 0 && ldx == Cin && KW > 1 && KW * Cin <= 64; }

static int wgrad_splits(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW) {
    int bm, bn;
    wgrad_tiles(Cin, Cout, bm, bn);
    long tiles = (long)KH * KW * ((Cin + bm - 1) / bm) * ((Cout + bn - 1) / bn);
    if (wgrad_merge(Cin, Cin, KW)) tiles = (long)KH * ((Cout + bn - 1) / bn);
    const long P = (long)N * Ho * Wo;
    const long target = bm == 128 ? 2560 : 4096;   // measured optimum: several short rounds balance better than one long one
    long S = target / tiles;                            // floor: never split a layer that already has enough tiles
    const long maxS_pix = P / 512 > 0 ? P / 512 : 1;   // >= 16 chunks of 32 pixels per split
    if (S > maxS_pix) S = maxS_pix;
    const size_t slab_bytes = (size_t)KH * KW * Cin * Cout * 4;
    const size_t cap = (size_t)256 << 20;
    if ((size_t)S * slab_bytes > cap) S = (long)(cap / slab_bytes);
    if (S < 1) S = 1;
    return (int)S;
}

// The plan: ONE decision, read by the three entries, by kpx_conv2d_wgrad_plan and by kpx_conv2d_wgrad_workspace_bytes: which kernel family takes a call,
// in how many partial slabs, and the few numbers its launch needs.  The families are asked in the order of enum KpxWgradFamily.
enum { WG_F32, WG_BF16, WG_IMAGE16 };       // operand types: x and dy fp32 / both bf16 / fp32 image with a bf16 gradient
// an entry's arguments: the leading fields of WgradGeom, x to pad_l (x, dy: bf16 tensors behind the float* type; the plan reads their alignment only)
struct WgradCall : WgradGeom { int arith, types; };

struct WgradPlan {
    int family = -1;                        // KPX_WGRAD_*; -1: no kernel for these operand types takes the call
    int S; size_t need;                     // partial slabs (1: the kernel writes dw itself) and the workspace bytes they take
    int cpb, CT, bm;                        // 32-pixel row chunks per workgroup (the three row kernels), 32-channel blocks per wavefront (rows), square channel tile
    WgradGeom g;                            // the call and its slab size; from the generic split plan on, the kernel arguments of gemm3 / generic
};

static bool wgrad_args_ok(const WgradCall& c) {
    if (!c.x || !c.dy || c.N <= 0 || c.Hi <= 0 || c.Wi <= 0 || c.Cin <= 0 || c.Cout <= 0 || c.Ho <= 0 || c.Wo <= 0 || c.KH <= 0 || c.KW <= 0 ||
        c.stride <= 0 || c.ldx < c.Cin || c.lddy < c.Cout || c.arith < 0 || c.arith > 1)
        return false;
    if (c.types == WG_BF16) return c.ldx % 8 == 0 && c.lddy % 8 == 0 && kpx_aligned16(c.x, c.dy);
    return c.types != WG_IMAGE16 || c.Cin <= 4;             // (image-input layers only)
}

// The fields that the kernel arguments of the three row-chunk kernels share
template <class G>
static G wgrad_fill(const WgradPlan& p) {
    const WgradGeom& c = p.g;
    G g{};
    g.x = c.x; g.dy = c.dy; g.out = c.out;
    g.N = c.N; g.Hi = c.Hi; g.Wi = c.Wi; g.Cin = c.Cin; g.ldx = c.ldx;
    g.Ho = c.Ho; g.Wo = c.Wo; g.Cout = c.Cout; g.lddy = c.lddy;
    g.KH = c.KH; g.KW = c.KW; g.pad_t = c.pad_t; g.pad_l = c.pad_l;
    g.total_chunks = c.N * c.Ho * (c.Wo / 32); g.cpb = p.cpb; g.ct = c.ct; g.slab = c.slab;
    return g;
}

// An entry's call ends at the first family that takes it.  The workspace query (c.x == nullptr) does not know the operands' layout, which
// can close any family to a call: for it every layout condition holds and the walk goes on to the end, `need` the largest it met.
static WgradPlan wgrad_plan(const WgradCall& c) {
    WgradPlan p{};
    WgradGeom& g = p.g = c;
    g.slab = (size_t)c.KH * c.KW * c.Cin * c.Cout;
    const bool any = !c.x;
    auto take = [&](int family, int S) {
        p.family = family; p.S = S;
        if (S > 1 && (size_t)S * g.slab * 4 > p.need) p.need = (size_t)S * g.slab * 4;
        return !any;
    };
    g.vecA = any || (c.ldx % 4 == 0 && kpx_aligned16(c.x)); g.vecB = any || (c.lddy % 4 == 0 && kpx_aligned16(c.dy));     // 16-B loads of x / dy
    const bool vec = g.vecA && g.vecB;
    const size_t px_in = (size_t)c.N * c.Hi * c.Wi, px_out = (size_t)c.N * c.Ho * c.Wo;
    int S, bn;

    // tiny filters over very many pixels (image-input layers, 16 -> 16 at full resolution, the 64 -> 4 head): conv_wsmall.hip, 16-B staging
    // units (dy always, x when it has a multiple of 4 channels) and 32-bit byte offsets at the PIXEL STRIDES (a channel slice has ldx > Cin)
    if (c.types != WG_BF16 && kpx_offsets_fit(px_in, c.ldx, 0x60000000ull) && kpx_offsets_fit(px_out, c.lddy, 0x60000000ull) &&
        (any || (c.Cout % 4 == 0 && g.vecB)) && (c.Cin % 4 != 0 || g.vecA)) {     // (any: the query has always counted this family for every Cout)
        S = kpx_wsmall_splits(c.N, c.Hi, c.Wi, c.Cin, c.Ho, c.Wo, c.Cout, c.KH, c.KW, c.stride);
        if (S >= 1 && take(KPX_WGRAD_WSMALL, S)) return p;
    }
    if (c.types == WG_IMAGE16) return p;                    // (the caller converts dy and uses the fp32 entry)
    if (c.types == WG_F32 && c.stride == 1) {
        // (the bf16x3 weight gradient of conv_gemm3.hip runs where the generic fp32 kernel would, and on the strided layers: measured ahead of the
        //  specialised fp32 kernels it loses -- 18.65 vs 17.9 ms per step in round 3)
        if (c.KH == 3 && c.KW == 3 && c.pad_t == 1 && c.pad_l == 1 && c.Ho == c.Hi && c.Wo == c.Wi && vec && (any || c.ldx >= ((c.Cin + 3) & ~3)) &&
            kpx_offsets_fit(px_in, c.ldx > c.lddy ? c.ldx : c.lddy, 0x60000000ull)) {
            S = kpx_wino_wgrad_splits(c.N, c.Hi, c.Wi, c.Cin, c.Cout);
            if (S >= 1 && take(KPX_WGRAD_WINO, S)) return p;
        }
        g.ct = 1;
        if (c.ldx == c.Cin && g.vecB && wgrad_rows_merged_plan(c.N, c.Ho, c.Wo, c.Cin, c.Cout, c.KH, c.KW, &S, &p.cpb) && take(KPX_WGRAD_ROWS_MERGED, S))
            return p;
        if (vec && c.Cin % 4 == 0 && wgrad_rows_plan(c.N, c.Ho, c.Wo, c.Cin, c.Cout, c.KH, c.KW, &S, &p.cpb, &p.CT)) {
            g.ct = (c.Cin + 32 * p.CT - 1) / (32 * p.CT);
            if (take(KPX_WGRAD_ROWS, S)) return p;
        }
    }
    // the generic split plan: conv_wgrad_kernel, and the two families that run on its grid
    wgrad_tiles(c.Cin, c.Cout, p.bm, bn);
    g.ct = (c.Cin + p.bm - 1) / p.bm; g.kt = (c.Cout + bn - 1) / bn; g.P = (int)px_out;
    g.S = S = wgrad_splits(c.N, c.Ho, c.Wo, c.Cin, c.Cout, c.KH, c.KW);
    g.pps = ((g.P + S - 1) / S + 31) / 32 * 32;
    g.io16 = c.types == WG_BF16;
    g.terms = g.io16 || c.arith == KPX_ARITH_BF16 ? 1 : 3;
    const bool tap = c.types == WG_F32 && vec && c.Cin % 4 == 0 && c.Cout % 4 == 0 && c.Wo % 32 == 0;
    // (strided layers: the bf16x3 kernel beats the fp32 tap-rows kernel -- encoder conv_3 at N = 64: 0.152 vs 0.198 ms; the stride-1
    //  layers that reach this point are faster on tap-rows / rows, and the 3x3 stride-1 layers on the Winograd weight gradient)
    if (kpx_wgrad3_eligible(&g) && (c.stride > 1 || !tap) && take(KPX_WGRAD_GEMM3, S)) return p;
    if (c.types == WG_BF16) return p;
    if (tap) {
        // chunk-aligned split: the generic plan's S in units of 32-pixel row chunks, which never comes out larger
        const int chunks = c.N * c.Ho * (c.Wo / 32);
        p.cpb = (chunks + S - 1) / S;
        const int St = (chunks + p.cpb - 1) / p.cpb;
        assert(St <= S);
        if (take(KPX_WGRAD_TAP_ROWS, St)) return p;
    }
    if (wgrad_merge(c.Cin, c.ldx, c.KW)) {                  // image inputs (Cin = 3, never a tap-rows layer): one tap per filter row, KW*Cin merged channels
        g.merge = c.Cin; g.Cin = c.KW * c.Cin; g.KW = 1; g.vecA = 0;
        g.ct = (g.Cin + p.bm - 1) / p.bm;
    }
    take(KPX_WGRAD_GENERIC, S);
    return p;
}

// Every entry: validate, plan, ONE workspace check (below the plan's need: refused, no other family is tried), fill the family's kernel arguments and launch, reduce.
static int wgrad_run(const WgradCall& c, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dw || !wgrad_args_ok(c)) return KPX_EINVAL;
    WgradPlan p = wgrad_plan(c);
    if (p.family < 0 || p.need > (workspace ? workspace_bytes : 0)) return KPX_EINVAL;
    float* const out = p.g.out = p.S > 1 ? (float*)workspace : dw;       // the slabs where the plan has them
    hipStream_t s = kpx_stream(stream);
    int rc = 0;                             // (of the launches made in other files; the kernels launched here are asked after the switch)
    switch (p.family) {
        case KPX_WGRAD_WSMALL:
            rc = kpx_wsmall_launch(c.x, c.N, c.Hi, c.Wi, c.Cin, c.ldx, c.dy, c.Ho, c.Wo, c.Cout, c.lddy, c.KH, c.KW, c.stride, c.pad_t, c.pad_l, out, p.S, s,
                                   c.types == WG_IMAGE16);
            break;
        case KPX_WGRAD_WINO:
            rc = kpx_wino_wgrad3x3(c.x, c.N, c.Hi, c.Wi, c.Cin, c.ldx, c.dy, c.Cout, c.lddy, out, p.S, s);
            break;
        case KPX_WGRAD_ROWS_MERGED:
        case KPX_WGRAD_ROWS: {
            const WgradRowsGeom r = wgrad_fill<WgradRowsGeom>(p);
            const dim3 grid((unsigned)(p.S * r.ct));
            if (p.family == KPX_WGRAD_ROWS_MERGED) hipLaunchKernelGGL((conv_wgrad_rows_merged_kernel<0>), grid, dim3(256), 0, s, r);
            else if (p.CT == 2) hipLaunchKernelGGL((conv_wgrad_rows_kernel<2>), grid, dim3(256), 0, s, r);
            else hipLaunchKernelGGL((conv_wgrad_rows_kernel<1>), grid, dim3(256), 0, s, r);
            break;
        }
        case KPX_WGRAD_TAP_ROWS: {
            WgradTapGeom r = wgrad_fill<WgradTapGeom>(p);
            r.stride = c.stride; r.S = p.S; r.kt = p.g.kt;
            const dim3 grid((unsigned)(r.S * r.KH * r.KW * r.ct * r.kt));
            if (p.bm == 128) hipLaunchKernelGGL((conv_wgrad_tap_rows_kernel<128, 128, 2, 4>), grid, dim3(512), 0, s, r);
            else hipLaunchKernelGGL((conv_wgrad_tap_rows_kernel<64, 64, 2, 2>), grid, dim3(256), 0, s, r);
            break;
        }
        default: {
            const WgradGeom& g = p.g;
            const dim3 grid((unsigned)(g.S * g.KH * g.KW * g.ct * g.kt));
            const bool vec = g.vecA && g.vecB;
            if (p.family == KPX_WGRAD_GEMM3) rc = kpx_wgrad3_launch(g, p.bm, g.terms, s);       // bf16x3 (fp32-equivalent) or bf16 operands on the bf16 matrix pipe
            else if (g.merge) hipLaunchKernelGGL((conv_wgrad_kernel<64, 64, 2, 2, false, true>), grid, dim3(256), 0, s, g);
            else if (p.bm == 128 && vec) hipLaunchKernelGGL((conv_wgrad_kernel<128, 128, 2, 4, true, false>), grid, dim3(512), 0, s, g);
            else if (p.bm == 128) hipLaunchKernelGGL((conv_wgrad_kernel<128, 128, 2, 4, false, false>), grid, dim3(512), 0, s, g);
            else if (vec) hipLaunchKernelGGL((conv_wgrad_kernel<64, 64, 2, 2, true, false>), grid, dim3(256), 0, s, g);
            else hipLaunchKernelGGL((conv_wgrad_kernel<64, 64, 2, 2, false, false>), grid, dim3(256), 0, s, g);
        }
    }
    return finish_wgrad(rc ? rc : kpx_launch_status(), workspace, dw, p.g.slab, p.S, s);
}

extern "C" int kpx_conv2d_wgrad_f32(const float* x, int N, int Hi, int Wi, int Cin, int ldx,
                                    const float* dy, int Ho, int Wo, int Cout, int lddy,
                                    float* dw, int KH, int KW, int stride, int pad_t, int pad_l, int arith,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return wgrad_run({{x, dy, nullptr, N, Hi, Wi, Cin, ldx, Ho, Wo, Cout, lddy, KH, KW, stride, pad_t, pad_l}, arith, WG_F32}, dw, workspace, workspace_bytes, stream);
}

// bf16 configuration: x and dy bf16 (pixel strides multiples of 8 elements), dw fp32; the bf16-pipe weight-gradient kernel of conv_gemm3.hip
// with the generic split plan.  KPX_EINVAL for shapes it does not take.
extern "C" int kpx_conv2d_wgrad_bf16(const void* x, int N, int Hi, int Wi, int Cin, int ldx, const void* dy, int Ho, int Wo, int Cout, int lddy,
                                     float* dw, int KH, int KW, int stride, int pad_t, int pad_l, void* workspace, size_t workspace_bytes, void* stream) {
    return wgrad_run({{(const float*)x, (const float*)dy, nullptr, N, Hi, Wi, Cin, ldx, Ho, Wo, Cout, lddy, KH, KW, stride, pad_t, pad_l}, 0, WG_BF16},
                     dw, workspace, workspace_bytes, stream);
}

// bf16 configuration, image-input layers (conv_igemm.hip has their forward and data gradient): x fp32 image, dy bf16 (pixel stride lddy
// elements, a multiple of 4) -> dw fp32 [KH, KW, Cin, Cout].  KPX_EINVAL for shapes conv_wsmall.hip does not take: the caller then converts
// and uses the fp32 entry.
extern "C" int kpx_conv_image_wgrad_bf16(const float* x, int N, int Hi, int Wi, int Cin, int ldx, const void* dy, int Ho, int Wo, int Cout, int lddy,
                                         float* dw, int KH, int KW, int stride, int pad_t, int pad_l, void* workspace, size_t workspace_bytes, void* stream) {
    return wgrad_run({{x, (const float*)dy, nullptr, N, Hi, Wi, Cin, ldx, Ho, Wo, Cout, lddy, KH, KW, stride, pad_t, pad_l}, 0, WG_IMAGE16},
                     dw, workspace, workspace_bytes, stream);
}

extern "C" int kpx_conv2d_wgrad_plan(const float* x, int N, int Hi, int Wi, int Cin, int ldx, const float* dy, int Ho, int Wo, int Cout, int lddy,
                                     int KH, int KW, int stride, int pad_t, int pad_l, int arith, int* family, int* splits, size_t* workspace_bytes) {
    const WgradCall c{{x, dy, nullptr, N, Hi, Wi, Cin, ldx, Ho, Wo, Cout, lddy, KH, KW, stride, pad_t, pad_l}, arith, WG_F32};
    if (!family || !splits || !workspace_bytes || !wgrad_args_ok(c)) return KPX_EINVAL;
    const WgradPlan p = wgrad_plan(c);
    *family = p.family; *splits = p.S; *workspace_bytes = p.need;
    return 0;
}

// The workspace of any of the three entries for a layer of this shape.  Unknown here: the operands' layout and the stride (1, or 2 with
// Hi = Ho * 2); 3x3 filters are asked with the SAME padding of the Winograd weight gradient.
extern "C" size_t kpx_conv2d_wgrad_workspace_bytes(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW) {
    auto need = [&](int st) { return wgrad_plan({{nullptr, nullptr, nullptr, N, Ho * st, Wo * st, Cin, Cin, Ho, Wo, Cout, Cout, KH, KW, st, 1, 1}, 0, WG_F32}).need; };
    return std::max(need(1), need(2));
}
