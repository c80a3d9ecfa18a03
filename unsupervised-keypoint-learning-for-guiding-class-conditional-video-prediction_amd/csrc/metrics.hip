// Video-prediction frame metrics: SSIM (TF 1.12 tf.image.ssim: 11-tap Gaussian window, sigma 1.5, VALID, k1 = 0.01, k2 = 0.03,
// compensation 1) and MSE / PSNR (tf.image.psnr) of frame pairs a[n], b[n] (fp32 NHWC, C in {1,3}).  DESIGN.md section 2 has the definition.
//
// One workgroup per frame.  The lanes cover (output column, channel) of a vertical strip of the frame (one strip at 128 x 128 x 3: 118 * 3 =
// 354 lanes in 6 waves) and walk down its rows:
//   - each input row of both images is staged in LDS (double-buffered; 16-byte loads when rows are 16-byte aligned), with D rows in flight
//     in registers ahead of the one being filtered;
//   - a lane filters its four moments (a, b, a*b, a^2 + b^2) horizontally from LDS in fp64 and pushes them into an 11-deep ring held in
//     registers (the row loop is unrolled by 11 so that every ring index is a constant);
//   - from row 10 on, the vertical filter over the ring gives mu_a, mu_b, S_ab, S_s of one output position, whose lum * cs is accumulated;
//   - (a - b)^2 of the staged row is accumulated in the same pass.
// fp64 moments: S_s - (mu_a^2 + mu_b^2) cancels against c2 = 9e-4 * L^2 on flat content, where fp32 sums miss 1e-5 in SSIM.
// The per-lane sums are reduced in a fixed order (wave butterflies, then waves in order): frame n's result depends on frame n alone.
// png8: both inputs are first quantised as evaluate.py writes PNGs, q = uint8(trunc(fl(fl(0.5 * fl(x + 1)) * 255))) clamped to [0, 255],
// and scored as q / 255 with L = 1 -- computed exactly as q with L = 255 (the same quantities up to fp64 rounding), mse scaled by 1/255^2.
//
// VGG feature-space metrics (kpx_feature_pair_metrics_f32, evaluate.py --vgg-metrics): per frame pair of one VGG19 layer's features fa, fb
// (fp32 NHWC, C a multiple of 4), the mean over positions of the channel cosine and the mean of |a - b|.  G = the largest power of two
// <= min(C / 4, 64) lanes share one position, each with 16-byte loads of both sides (a wave reads 64 / G consecutive positions: one
// contiguous run); the three channel sums of a position are fp32 lane partials folded by a butterfly inside the group, the ratio and every
// sum across positions are fp64.  A frame is cut into S slabs of positions, S a function of (H, W, C) alone: one workgroup per (slab, frame)
// writes its two fp64 partials to `work`, a second launch folds a frame's slabs in order.  No atomics; frame n depends on frame n alone.
// kpx_vgg_prep_png8_f32 is the VGG input of those frames: q - mean, BGR, of the same 8-bit quantisation.
//
// Motion metrics (evaluate.py --motion-metrics): how far the D draws of z of one sample lie apart, and the key-point error of each.
//   - kpx_draw_moments_add_f32: per value of a rollout, sum += q and sumsq += q * q of its 8-bit value q (kpx_png8_unit), uint32, one call per
//     draw: element-wise, 16 bytes per lane and array when the three pointers allow it.
//   - kpx_draw_diversity_f32: V = D * sumsq - sum^2 = the sum over the D (D - 1) / 2 pairs of draws of (q_i - q_j)^2, an integer; one
//     workgroup per frame sums V in uint64 (order-free, so exact and the same for every batch) and writes floor(2 sqrt(mean_c variance)) per
//     pixel with an integer square root.
//   - kpx_keypoint_draw_metrics_f32: one lane per (draw, sample, frame) for the error against the labels and one per (sample, frame) for the
//     mean pairwise distance of the draws, each a single fp64 chain in a fixed order.
#include "kpx_common.h"
#include <cmath>

namespace {

constexpr int FM_TAPS = 11;
constexpr int FM_MAX_THREADS = 512;
constexpr int FM_PREFETCH = 3;                                        // staged rows in flight (registers) ahead of the filtered row
constexpr int FM_MAX_LF = FM_MAX_THREADS + 10 * 3 + 8;                // floats of one staged image row: strip columns + halo, rounded to 4

struct FmParams {
    double w[FM_TAPS];                // separable Gaussian window
    double c1, c2;                    // (k1 L)^2, (k2 L)^2
    double npos;                      // (H - 10) (W - 10) C
    double npix;                      // H W C
    double mse_scale;                 // 1, or 1 / 255^2 for png8
    double psnr_l;                    // 20 log10(L) of the reported scale
};

// lum * cs of one position and channel, in TF's order of operations.  Not contracted: for a == b the numerator and the denominator are
// the same roundings, so the term is exactly 1.
__device__ __forceinline__ double fm_ssim_term(double ma, double mb, double sab, double ss, double c1, double c2) {
#pragma clang fp contract(off)
    const double p = ma * mb, q = ma * ma, s = mb * mb;
    const double num0 = p + p, den0 = q + s;
    const double lum_n = num0 + c1, lum_d = den0 + c1;
    const double cs_n = ((sab + sab) - num0) + c2, cs_d = (ss - den0) + c2;
    return (lum_n * cs_n) / (lum_d * cs_d);
}

template <bool VEC>
__device__ __forceinline__ f32x4 fm_load(const float* __restrict__ src, int j, int lf) {
    f32x4 v;
    if (VEC) {
        v = *reinterpret_cast<const f32x4*>(src + j);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j + e < lf ? src[j + e] : 0.0f;
    }
    return v;
}

template <int C, bool VEC, bool PNG8>
__global__ __launch_bounds__(FM_MAX_THREADS) void frame_metrics_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                                       int SC, FmParams p, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float stage[2][2][FM_MAX_LF];   // [buffer][image][staged floats]
    __shared__ double red[2][FM_MAX_THREADS / KPX_WAVE];
    const int n = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const int Wo = W - 10;
    const int x = tid / C, c = tid - x * C;
    const size_t row_floats = (size_t)W * C;
    double ssim_acc = 0.0, mse_acc = 0.0;

    for (int x0 = 0; x0 < Wo; x0 += SC) {
        const int sc = min(SC, Wo - x0);                              // output columns of this strip
        const int lf = (sc + 10) * C;                                  // staged floats per image row
        const int own = x0 + sc == Wo ? lf : sc * C;                   // floats this strip adds to the MSE (the last one takes the halo)
        const int slots = (lf + 3) >> 2;                               // 4-float slots per image row; 2 * slots <= T
        const bool loader = tid < 2 * slots;
        const int img = tid < slots ? 0 : 1;
        const int j4 = 4 * (tid - img * slots);
        const float* src = (img ? b : a) + (size_t)n * H * row_floats + (size_t)x0 * C;
        const bool active = x < sc;

        auto put = [&](int buf, f32x4 v) {
            if (PNG8) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = kpx_png8_unit(v[e]);
            }
            *reinterpret_cast<f32x4*>(&stage[buf][img][j4]) = v;
        };
        f32x4 g[FM_PREFETCH];                                          // g[i] holds row r + 1 + i at the top of iteration r
        if (loader) {
            put(0, fm_load<VEC>(src, j4, lf));
#pragma unroll
            for (int i = 0; i < FM_PREFETCH; ++i)
                if (1 + i < H) g[i] = fm_load<VEC>(src + (size_t)(1 + i) * row_floats, j4, lf);
        }
        __syncthreads();

        double h[FM_TAPS][4];                                          // ring: horizontal moments of rows r-10..r, slot = row % 11
        for (int r0 = 0; r0 < H; r0 += FM_TAPS) {
#pragma unroll
            for (int k = 0; k < FM_TAPS; ++k) {
                const int r = r0 + k;
                if (r >= H) continue;                                  // (wave-uniform; a break would keep the loop from unrolling)
                if (loader && r + 1 < H) {                             // stage row r + 1 (its buffer was last read in iteration r - 1)
                    put((r + 1) & 1, g[0]);
#pragma unroll
                    for (int i = 0; i + 1 < FM_PREFETCH; ++i) g[i] = g[i + 1];
                    if (r + 1 + FM_PREFETCH < H) g[FM_PREFETCH - 1] = fm_load<VEC>(src + (size_t)(r + 1 + FM_PREFETCH) * row_floats, j4, lf);
                }
                const float* sa = stage[r & 1][0];
                const float* sb = stage[r & 1][1];
                for (int j = tid; j < own; j += T) {
                    const double d = (double)sa[j] - (double)sb[j];
                    mse_acc = fma(d, d, mse_acc);
                }
                if (active) {
                    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
#pragma unroll
                    for (int i = 0; i < FM_TAPS; ++i) {
                        const double da = sa[(x + i) * C + c], db = sb[(x + i) * C + c];
                        const double w = p.w[i];
                        m0 = fma(w, da, m0);
                        m1 = fma(w, db, m1);
                        m2 = fma(w, da * db, m2);
                        m3 = fma(w, fma(da, da, db * db), m3);
                    }
                    h[k][0] = m0; h[k][1] = m1; h[k][2] = m2; h[k][3] = m3;
                    if (r >= FM_TAPS - 1) {
                        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
#pragma unroll
                        for (int i = 0; i < FM_TAPS; ++i) {                // row r - 10 + i sits in slot (k + 1 + i) % 11
                            const int s = (k + 1 + i) % FM_TAPS;
                            const double w = p.w[i];
                            v0 = fma(w, h[s][0], v0);
                            v1 = fma(w, h[s][1], v1);
                            v2 = fma(w, h[s][2], v2);
                            v3 = fma(w, h[s][3], v3);
                        }
                        ssim_acc += fm_ssim_term(v0, v1, v2, v3, p.c1, p.c2);
                    }
                }
                __syncthreads();
            }
        }
    }

    ssim_acc = kpx_wave_sum_d(ssim_acc);
    mse_acc = kpx_wave_sum_d(mse_acc);
    const int wave = tid / KPX_WAVE, nwaves = T / KPX_WAVE;
    if ((tid & (KPX_WAVE - 1)) == 0) { red[0][wave] = ssim_acc; red[1][wave] = mse_acc; }
    __syncthreads();
    if (tid == 0) {
        double s = red[0][0], m = red[1][0];
        for (int i = 1; i < nwaves; ++i) { s += red[0][i]; m += red[1][i]; }
        const double ssim = s / p.npos;                                 // exactly 1 when every term is
        const double mse = m / p.npix * p.mse_scale;
        const double psnr = p.psnr_l - 10.0 * log10(mse);               // +inf for mse == 0
        out[3 * (size_t)n + 0] = (float)ssim;
        out[3 * (size_t)n + 1] = (float)mse;
        out[3 * (size_t)n + 2] = (float)psnr;
    }
}

template <int C, bool PNG8>
int fm_launch(const float* a, const float* b, int N, int H, int W, bool vec, int T, int SC, const FmParams& p, float* out, hipStream_t s) {
    if (vec)
        hipLaunchKernelGGL((frame_metrics_kernel<C, true, PNG8>), dim3(N), dim3(T), 0, s, a, b, H, W, SC, p, out);
    else
        hipLaunchKernelGGL((frame_metrics_kernel<C, false, PNG8>), dim3(N), dim3(T), 0, s, a, b, H, W, SC, p, out);
    return kpx_launch_status();
}

// ---------------------------------------------------------------------------------------------- VGG feature-space metrics
constexpr int FP_THREADS = 256;
constexpr int FP_SLAB_BYTES = 32768;                                  // of one side per workgroup: 8 passes of 256 lanes x 16 bytes
constexpr int FP_MAX_SLABS = 128;

int fp_slabs(int H, int W, int C) {
    const long long bytes = (long long)H * W * C * 4;                  // >= 16; a slab never holds less than one position (C * 4 <= 2048)
    const long long s = (bytes + FP_SLAB_BYTES - 1) / FP_SLAB_BYTES;
    return (int)(s > FP_MAX_SLABS ? FP_MAX_SLABS : s);
}

// cosine of one position from its channel sums: 1 where both sides are zero, 0 where one is, else min(1, dot / sqrt(saa sbb)) in fp64.
// saa == sbb == dot (identical sides) gives exactly 1: the product of two floats and its root are exact in fp64.  NaN stays NaN.
__device__ __forceinline__ double fp_cos(float saa, float sbb, float dot) {
    if (saa == 0.0f && sbb == 0.0f) return 1.0;
    if (saa == 0.0f || sbb == 0.0f) return 0.0;
    const double c = (double)dot / sqrt((double)saa * (double)sbb);
    return c > 1.0 ? 1.0 : c;
}

template <int G>
__global__ __launch_bounds__(FP_THREADS) void feature_pair_kernel(const float* __restrict__ fa, const float* __restrict__ fb, int N, int P, int C4,
                                                                   int S, double* __restrict__ work) {
    constexpr int PPB = FP_THREADS / G;                                // positions per pass of the workgroup
    __shared__ double red[2][FP_THREADS / KPX_WAVE];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int l = tid % G, g = tid / G;
    const int p0 = (int)((long long)P * s / S), p1 = (int)((long long)P * (s + 1) / S);
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const f32x4* an = reinterpret_cast<const f32x4*>(fa) + (size_t)n * P * C4;
        const f32x4* bn = reinterpret_cast<const f32x4*>(fb) + (size_t)n * P * C4;
        double cos_acc = 0.0, l1_acc = 0.0;
        for (int pb = p0; pb < p1; pb += PPB) {                        // uniform over the workgroup: every lane takes part in the butterflies
            const int p = pb + g;
            const bool valid = p < p1;
            float saa = 0.0f, sbb = 0.0f, dot = 0.0f, l1 = 0.0f;
            if (valid) {
                const f32x4* pa = an + (size_t)p * C4;
                const f32x4* pq = bn + (size_t)p * C4;
                for (int j = l; j < C4; j += G) {                      // at most 2 rounds (C4 < 2 G, or G = 64 and C4 <= 128): 8 elements per lane
                    const f32x4 va = pa[j], vb = pq[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        saa = fmaf(va[e], va[e], saa);
                        sbb = fmaf(vb[e], vb[e], sbb);
                        dot = fmaf(va[e], vb[e], dot);
                        l1 += fabsf(va[e] - vb[e]);
                    }
                }
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
                saa += __shfl_xor(saa, o, 64);
                sbb += __shfl_xor(sbb, o, 64);
                dot += __shfl_xor(dot, o, 64);
            }
            if (valid) {
                l1_acc += (double)l1;
                if (l == 0) cos_acc += fp_cos(saa, sbb, dot);
            }
        }
        cos_acc = kpx_wave_sum_d(cos_acc);
        l1_acc = kpx_wave_sum_d(l1_acc);
        if ((tid & (KPX_WAVE - 1)) == 0) { red[0][tid / KPX_WAVE] = cos_acc; red[1][tid / KPX_WAVE] = l1_acc; }
        __syncthreads();
        if (tid == 0) {
            double c = red[0][0], d = red[1][0];
            for (int i = 1; i < FP_THREADS / KPX_WAVE; ++i) { c += red[0][i]; d += red[1][i]; }
            double* o = work + ((size_t)n * S + s) * 2;
            o[0] = c;
            o[1] = d;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(KPX_WAVE) void feature_pair_finalize_kernel(const double* __restrict__ work, int N, int S, double npos, double nelem,
                                                                         float* __restrict__ out) {
    const int n = blockIdx.x * KPX_WAVE + threadIdx.x;
    if (n >= N) return;
    const double* w = work + (size_t)n * S * 2;
    double c = w[0], d = w[1];
    for (int i = 1; i < S; ++i) { c += w[2 * i]; d += w[2 * i + 1]; }
    out[2 * (size_t)n + 0] = (float)(c / npos);                        // exactly 1 when every position's cosine is
    out[2 * (size_t)n + 1] = (float)(d / nelem);
}

template <int G>
void fp_launch(const float* fa, const float* fb, int N, int P, int C4, int S, double* work, hipStream_t s) {
    hipLaunchKernelGGL((feature_pair_kernel<G>), dim3(S, N > 65535 ? 65535 : N), dim3(FP_THREADS), 0, s, fa, fb, N, P, C4, S, work);
}

__global__ __launch_bounds__(256) void vgg_prep_png8_kernel(const float* __restrict__ rgb, size_t P, float* __restrict__ bgr) {
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (size_t)gridDim.x * 256) {
        const float r = kpx_png8_unit(rgb[p * 3 + 0]), g = kpx_png8_unit(rgb[p * 3 + 1]), b = kpx_png8_unit(rgb[p * 3 + 2]);
        bgr[p * 3 + 0] = b - 103.939f; bgr[p * 3 + 1] = g - 116.779f; bgr[p * 3 + 2] = r - 123.68f;
    }
}

// ---------------------------------------------------------------------------------------------- motion metrics: draws of z
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int DM_THREADS = 256;
constexpr int DM_MAX_BLOCKS = 4096;                                   // 16 workgroups per CU: grid-stride beyond that
constexpr int DM_MAX_DRAWS = 4096;                                    // 255^2 * 4096 < 2^32: the accumulators cannot wrap

template <bool VEC>
__global__ __launch_bounds__(DM_THREADS) void draw_moments_add_kernel(const float* __restrict__ x, size_t n, uint32_t* __restrict__ sum,
                                                                      uint32_t* __restrict__ sumsq) {
    const size_t t0 = (size_t)blockIdx.x * DM_THREADS + threadIdx.x, stride = (size_t)gridDim.x * DM_THREADS;
    const size_t nv = VEC ? n >> 2 : 0;                                // 16-byte groups; the rest (everything without VEC) is the scalar tail
    for (size_t i = t0; i < nv; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        u32x4 s = reinterpret_cast<const u32x4*>(sum)[i], ss = reinterpret_cast<const u32x4*>(sumsq)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t q = (uint32_t)kpx_png8_unit(v[e]);
            s[e] += q;
            ss[e] += q * q;
        }
        reinterpret_cast<u32x4*>(sum)[i] = s;
        reinterpret_cast<u32x4*>(sumsq)[i] = ss;
    }
    for (size_t i = 4 * nv + t0; i < n; i += stride) {
        const uint32_t q = (uint32_t)kpx_png8_unit(x[i]);
        sum[i] += q;
        sumsq[i] += q * q;
    }
}

// floor(sqrt(m)), exactly: the fp64 estimate is off by at most one either way, the integer comparisons settle it (m < 2^62)
__device__ __forceinline__ uint64_t dm_isqrt(uint64_t m) {
    uint64_t r = (uint64_t)sqrt((double)m);
    while (r * r > m) --r;
    while ((r + 1) * (r + 1) <= m) ++r;
    return r;
}

template <int C>
__global__ __launch_bounds__(DM_THREADS) void draw_diversity_kernel(const uint32_t* __restrict__ sum, const uint32_t* __restrict__ sumsq, int P,
                                                                    uint32_t D, double denom, float* __restrict__ div_mse,
                                                                    uint8_t* __restrict__ std_map) {
    __shared__ uint64_t red[DM_THREADS];
    const int n = blockIdx.x, tid = threadIdx.x;
    const uint32_t* s = sum + (size_t)n * P * C;
    const uint32_t* ss = sumsq + (size_t)n * P * C;
    const uint64_t per_pixel = (uint64_t)C * D * D;
    uint64_t acc = 0;
    for (int p = tid; p < P; p += DM_THREADS) {
        uint64_t v = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint64_t a = s[(size_t)p * C + c];
            v += (uint64_t)D * ss[(size_t)p * C + c] - a * a;
        }
        acc += v;
        if (std_map) {
            const uint64_t r = dm_isqrt(4 * v / per_pixel);
            std_map[(size_t)n * P + p] = (uint8_t)(r > 255 ? 255 : r);
        }
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int o = DM_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) div_mse[n] = (float)((double)red[0] / denom);
}

// |a - b| of two points in fp64, each operation rounded once (no fma: the float64 restatement has none)
__device__ __forceinline__ double kd_dist(const float* __restrict__ a, const float* __restrict__ b) {
#pragma clang fp contract(off)
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1];
    return sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(DM_THREADS) void keypoint_draw_metrics_kernel(const float* __restrict__ pts, const float* __restrict__ real, int D,
                                                                           size_t NT, int K, float* __restrict__ l2, float* __restrict__ div) {
    const size_t idx = (size_t)blockIdx.x * DM_THREADS + threadIdx.x;
    const size_t roles = (size_t)D + (div ? 1 : 0);
    if (idx >= roles * NT) return;
    const size_t role = idx / NT, f = idx - role * NT;               // role < D: the error of draw `role`; role == D: the draws' diversity
    const size_t frame = (size_t)K * 2;
    if (role < (size_t)D) {
        const float* p = pts + (role * NT + f) * frame;
        const float* r = real + f * frame;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += kd_dist(p + 2 * k, r + 2 * k);
        l2[role * NT + f] = (float)(acc / (double)K);
        return;
    }
    double acc = 0.0;
    for (int i = 0; i < D; ++i)
        for (int j = i + 1; j < D; ++j) {
            const float* a = pts + ((size_t)i * NT + f) * frame;
            const float* b = pts + ((size_t)j * NT + f) * frame;
            for (int k = 0; k < K; ++k) acc += kd_dist(a + 2 * k, b + 2 * k);
        }
    div[f] = (float)(acc * 2.0 / ((double)D * (double)(D - 1) * (double)K));
}

}  // namespace

extern "C" int kpx_draw_moments_add_f32(const float* x, size_t n, uint32_t* sum, uint32_t* sumsq, void* stream) {
    if (!x || !sum || !sumsq || ((((uintptr_t)x) | ((uintptr_t)sum) | ((uintptr_t)sumsq)) & 3)) return KPX_EINVAL;
    if (n == 0) return 0;
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)sum) | ((uintptr_t)sumsq)) & 15) == 0;
    const size_t items = vec ? (n + 3) >> 2 : n;                       // one per lane and pass (the tail of the 16-byte form has < 4 values)
    const size_t blocks = (items + DM_THREADS - 1) / DM_THREADS;
    const dim3 grid((unsigned)(blocks > DM_MAX_BLOCKS ? DM_MAX_BLOCKS : blocks));
    hipStream_t s = kpx_stream(stream);
    if (vec)
        hipLaunchKernelGGL(draw_moments_add_kernel<true>, grid, dim3(DM_THREADS), 0, s, x, n, sum, sumsq);
    else
        hipLaunchKernelGGL(draw_moments_add_kernel<false>, grid, dim3(DM_THREADS), 0, s, x, n, sum, sumsq);
    return kpx_launch_status();
}

extern "C" int kpx_draw_diversity_f32(const uint32_t* sum, const uint32_t* sumsq, int N, int H, int W, int C, int D, float* div_mse,
                                      uint8_t* std_map, void* stream) {
    if (!sum || !sumsq || !div_mse || N < 1 || H < 1 || H > 1024 || W < 1 || W > 1024 || !(C == 1 || C == 3) || D < 2 || D > DM_MAX_DRAWS ||
        ((((uintptr_t)sum) | ((uintptr_t)sumsq) | ((uintptr_t)div_mse)) & 3))
        return KPX_EINVAL;
    const int P = H * W;
    const double pairs = (double)((long long)D * (D - 1) / 2);
    const double denom = (pairs * 65025.0) * (double)((long long)P * C);   // pairs * 255^2 is exact; at most one rounding in the product
    hipStream_t s = kpx_stream(stream);
    if (C == 1)
        hipLaunchKernelGGL(draw_diversity_kernel<1>, dim3(N), dim3(DM_THREADS), 0, s, sum, sumsq, P, (uint32_t)D, denom, div_mse, std_map);
    else
        hipLaunchKernelGGL(draw_diversity_kernel<3>, dim3(N), dim3(DM_THREADS), 0, s, sum, sumsq, P, (uint32_t)D, denom, div_mse, std_map);
    return kpx_launch_status();
}

extern "C" int kpx_keypoint_draw_metrics_f32(const float* pts, const float* real, int D, int N, int T, int K, float* l2, float* div,
                                             void* stream) {
    if (!pts || !real || !l2 || D < 1 || D > DM_MAX_DRAWS || N < 1 || T < 1 || K < 1 || (D == 1 && div) ||
        ((((uintptr_t)pts) | ((uintptr_t)real) | ((uintptr_t)l2) | ((uintptr_t)div)) & 3))
        return KPX_EINVAL;
    const size_t NT = (size_t)N * T;
    const size_t blocks = (((size_t)D + (div ? 1 : 0)) * NT + DM_THREADS - 1) / DM_THREADS;
    if (blocks > 0x7fffffffULL) return KPX_EINVAL;
    hipLaunchKernelGGL(keypoint_draw_metrics_kernel, dim3((unsigned)blocks), dim3(DM_THREADS), 0, kpx_stream(stream), pts, real, D, NT, K, l2, div);
    return kpx_launch_status();
}

extern "C" size_t kpx_feature_pair_metrics_workspace_bytes(int N, int H, int W, int C) {
    if (N < 1 || H < 1 || H > 1024 || W < 1 || W > 1024 || C < 4 || C > 512 || C % 4) return 0;
    return (size_t)N * fp_slabs(H, W, C) * 2 * sizeof(double);
}

extern "C" int kpx_feature_pair_metrics_f32(const float* fa, const float* fb, int N, int H, int W, int C, float* work, float* out, void* stream) {
    if (!fa || !fb || !work || !out || N < 1 || H < 1 || H > 1024 || W < 1 || W > 1024 || C < 4 || C > 512 || C % 4 ||
        ((((uintptr_t)fa) | ((uintptr_t)fb)) & 15) || (((uintptr_t)work) & 7) || (((uintptr_t)out) & 3))
        return KPX_EINVAL;
    const int P = H * W, C4 = C / 4, S = fp_slabs(H, W, C);
    double* wk = reinterpret_cast<double*>(work);
    hipStream_t s = kpx_stream(stream);
    const int lanes = C4 > 64 ? 64 : C4;                               // lanes of one position: the largest power of two <= min(C / 4, 64)
    if (lanes >= 64) fp_launch<64>(fa, fb, N, P, C4, S, wk, s);
    else if (lanes >= 32) fp_launch<32>(fa, fb, N, P, C4, S, wk, s);
    else if (lanes >= 16) fp_launch<16>(fa, fb, N, P, C4, S, wk, s);
    else if (lanes >= 8) fp_launch<8>(fa, fb, N, P, C4, S, wk, s);
    else if (lanes >= 4) fp_launch<4>(fa, fb, N, P, C4, S, wk, s);
    else if (lanes >= 2) fp_launch<2>(fa, fb, N, P, C4, S, wk, s);
    else fp_launch<1>(fa, fb, N, P, C4, S, wk, s);
    int rc = kpx_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(feature_pair_finalize_kernel, dim3((N + KPX_WAVE - 1) / KPX_WAVE), dim3(KPX_WAVE), 0, s, (const double*)wk, N, S,
                       (double)P, (double)P * C, out);
    return kpx_launch_status();
}

extern "C" int kpx_vgg_prep_png8_f32(const float* rgb, size_t P, float* bgr, void* stream) {
    if (!rgb || !bgr) return KPX_EINVAL;
    if (P == 0) return 0;
    const size_t blocks = (P + 255) / 256;
    hipLaunchKernelGGL(vgg_prep_png8_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, kpx_stream(stream), rgb, P, bgr);
    return kpx_launch_status();
}

extern "C" int kpx_frame_metrics_f32(const float* a, const float* b, int N, int H, int W, int C, float L, int png8, float* out, void* stream) {
    if (!a || !b || !out || N < 1 || H < 11 || H > 1024 || W < 11 || W > 1024 || !(C == 1 || C == 3) || !(png8 == 0 || png8 == 1) ||
        !(L > 0.0f) || !std::isfinite(L))
        return KPX_EINVAL;
    FmParams p;
    double ws = 0.0;
    for (int i = 0; i < FM_TAPS; ++i) ws += p.w[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    for (int i = 0; i < FM_TAPS; ++i) p.w[i] /= ws;
    const double l = png8 ? 255.0 : (double)L;                        // png8 scores q (integers) at L = 255, i.e. q / 255 at L = 1
    p.c1 = (0.01 * l) * (0.01 * l);
    p.c2 = (0.03 * l) * (0.03 * l);
    p.npos = (double)(H - 10) * (W - 10) * C;
    p.npix = (double)H * W * C;
    p.mse_scale = png8 ? 1.0 / (255.0 * 255.0) : 1.0;
    p.psnr_l = png8 ? 0.0 : 20.0 * std::log10((double)L);
    // workgroup: one lane per (output column, channel) of a strip, up to FM_MAX_THREADS; strips of SC columns (a multiple of 4, so that
    // every strip starts on a 16-byte boundary when the rows do)
    const int Wo = W - 10;
    int T = (Wo * C + KPX_WAVE - 1) / KPX_WAVE * KPX_WAVE;
    T = T > FM_MAX_THREADS ? FM_MAX_THREADS : T;
    const int SC = (T / C) & ~3;
    const bool vec = (W * C) % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
    hipStream_t s = kpx_stream(stream);
    if (C == 1) return png8 ? fm_launch<1, true>(a, b, N, H, W, vec, T, SC, p, out, s) : fm_launch<1, false>(a, b, N, H, W, vec, T, SC, p, out, s);
    return png8 ? fm_launch<3, true>(a, b, N, H, W, vec, T, SC, p, out, s) : fm_launch<3, false>(a, b, N, H, W, vec, T, SC, p, out, s);
}
