// Key-point resampling in time (FinalModel.run(rate=...), animate.py / evaluate.py --rate) and the per-frame speed of a key-point sequence
// (evaluate.py --frames: the seam diagnostic of a chained rollout).  DESIGN.md sections 2 and 4.4.
//
// kpx_points_resample_f32: the knots P_0 = first [B,K,2] and P_1..P_N = seq [B,N,K,2] stand at the times 0..N; output frame j = 1..N*F
// stands at the time j / F and is stored at index j - 1 of out [B,N*F,K,2].  With i = j div F and r = j mod F:
//   r == 0   out = P_i                                                                  (bit copy)
//   LINEAR   out = fl32(P_i + s * (P_{i+1} - P_i)),  s = (double)r / (double)F
//   CUBIC    out = fl32(h00 * P_i + h10 * m_i + h01 * P_{i+1} + h11 * m_{i+1}), added from the left, with
//            s2 = s * s, s3 = s2 * s, h00 = (2 s3 - 3 s2) + 1, h10 = (s3 - 2 s2) + s, h01 = -2 s3 + 3 s2, h11 = s3 - s2,
//            m_i = (P_{i+1} - P_{i-1}) / 2 for 0 < i < N, m_0 = P_1 - P_0, m_N = P_N - P_{N-1}
// in fp64 from the fp32 knots, every operation rounded once (no fma), one rounding to fp32 at the store, no clamp.
//
// kpx_points_speed_f64: speed[b,t] = scale * ((sum_k sqrt(dx * dx + dy * dy)) / K), d = P_t[k] - P_{t-1}[k], the sum in the order k = 0..K-1.
//
// Both are a few hundred KB at the most: one thread per output item, no LDS, no atomics.  An output of the resampler reads the knots of its
// own sample, point and stencil alone (2 knots LINEAR, up to 4 CUBIC), so a non-finite knot stays in the frames whose stencil holds it.
// 16-byte accesses when K is even (a row of 2K floats is then whole 16-byte items) and every base is 16-byte aligned, 4-byte accesses
// otherwise: the same values either way.
#include "kpx_common.h"
#include <type_traits>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_BLOCKS = 4096;

struct rs_basis {
    double s, h00, h10, h01, h11;
};

__device__ __forceinline__ rs_basis rs_make_basis(int r, int F) {
#pragma clang fp contract(off)
    rs_basis h;
    h.s = (double)r / (double)F;
    const double s2 = h.s * h.s, s3 = s2 * h.s;
    h.h00 = (2.0 * s3 - 3.0 * s2) + 1.0;
    h.h10 = (s3 - 2.0 * s2) + h.s;
    h.h01 = -2.0 * s3 + 3.0 * s2;
    h.h11 = s3 - s2;
    return h;
}

// pm, p0, p1, p2 = P_{i-1}, P_i, P_{i+1}, P_{i+2}; lo: i == 0 (pm is not a knot), hi: i + 1 == N (p2 is not a knot)
template <int MODE>
__device__ __forceinline__ float rs_value(const rs_basis& h, float pm, float p0, float p1, float p2, bool lo, bool hi) {
#pragma clang fp contract(off)
    const double a = (double)p0, b = (double)p1;
    if constexpr (MODE == KPX_RESAMPLE_LINEAR) {
        return (float)(a + h.s * (b - a));
    } else {
        const double m0 = lo ? b - a : (b - (double)pm) / 2.0;
        const double m1 = hi ? b - a : ((double)p2 - a) / 2.0;
        return (float)(((h.h00 * a + h.h10 * m0) + h.h01 * b) + h.h11 * m1);
    }
}

// One item = V consecutive floats of one output frame (V = 4: row % 4 == 0).  items = B * N * F * row / V < 2^31.
template <int MODE, bool VEC>
__global__ __launch_bounds__(RS_THREADS) void points_resample_kernel(const float* __restrict__ first, const float* __restrict__ seq, int N,
                                                                     int K, int F, int items, float* __restrict__ out) {
    constexpr int V = VEC ? 4 : 1;
    typedef typename std::conditional<VEC, f32x4, float>::type item_t;
    const int row = 2 * K, per_row = row / V, frames = N * F;
    for (long long it = blockIdx.x * RS_THREADS + threadIdx.x; it < items; it += gridDim.x * RS_THREADS) {   // 64-bit: the stride may pass 2^31
        const int c = (int)(it % per_row) * V, fr = (int)(it / per_row);           // column inside the row; output frame over all samples
        const int b = fr / frames, j = fr % frames + 1;                // j = 1..N*F
        const int i = j / F, r = j % F;                                // i = 0..N; r != 0 implies i < N
        const float* f0 = first + (size_t)b * row + c;                 // knot 0 of this sample and column
        const float* sq = seq + (size_t)b * N * row + c;               // knot n >= 1 at sq + (n - 1) * row
        auto knot = [&](int n) { return *reinterpret_cast<const item_t*>(n == 0 ? f0 : sq + (size_t)(n - 1) * row); };
        item_t v;
        if (r == 0) {
            v = knot(i);
        } else {
            const rs_basis h = rs_make_basis(r, F);
            const bool lo = i == 0, hi = i + 1 == N;
            const item_t p0 = knot(i), p1 = knot(i + 1);
            item_t pm = p0, p2 = p1;                                   // placeholders where the stencil ends: rs_value does not read them
            if constexpr (MODE == KPX_RESAMPLE_CUBIC) {
                if (!lo) pm = knot(i - 1);
                if (!hi) p2 = knot(i + 2);
            }
            if constexpr (VEC) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = rs_value<MODE>(h, pm[q], p0[q], p1[q], p2[q], lo, hi);
            } else {
                v = rs_value<MODE>(h, pm, p0, p1, p2, lo, hi);
            }
        }
        *reinterpret_cast<item_t*>(out + (size_t)it * V) = v;
    }
}

template <int MODE>
void rs_launch(const float* first, const float* seq, int N, int K, int F, long long total, float* out, bool vec, hipStream_t s) {
    const int items = (int)(vec ? total / 4 : total);
    const int need = (items + RS_THREADS - 1) / RS_THREADS;
    const dim3 grid(need > RS_MAX_BLOCKS ? RS_MAX_BLOCKS : need), block(RS_THREADS);
    if (vec)
        hipLaunchKernelGGL((points_resample_kernel<MODE, true>), grid, block, 0, s, first, seq, N, K, F, items, out);
    else
        hipLaunchKernelGGL((points_resample_kernel<MODE, false>), grid, block, 0, s, first, seq, N, K, F, items, out);
}

// one thread per (b, t): K sequential terms
__global__ __launch_bounds__(RS_THREADS) void points_speed_kernel(const float* __restrict__ first, const float* __restrict__ seq, int T, int K,
                                                                  int frames, double scale, double* __restrict__ speed) {
#pragma clang fp contract(off)
    const int row = 2 * K;
    for (int fr = blockIdx.x * RS_THREADS + threadIdx.x; fr < frames; fr += gridDim.x * RS_THREADS) {
        const int b = fr / T, t = fr % T;                              // t = 0: frame 1, whose predecessor is `first`
        const float* cur = seq + (size_t)fr * row;
        const float* prev = t == 0 ? first + (size_t)b * row : cur - row;
        double sum = 0.0;
        for (int k = 0; k < K; ++k) {
            const double dx = (double)cur[2 * k] - (double)prev[2 * k], dy = (double)cur[2 * k + 1] - (double)prev[2 * k + 1];
            const double term = sqrt(dx * dx + dy * dy);
            sum = k == 0 ? term : sum + term;
        }
        speed[fr] = scale * (sum / (double)K);
    }
}

}  // namespace

extern "C" int kpx_points_resample_f32(const float* first, const float* seq, int B, int N, int K, int F, int mode, float* out, void* stream) {
    if (B < 1 || N < 1 || K < 1 || K > KPX_RESAMPLE_MAX_POINTS || F < 1 || F > KPX_RESAMPLE_MAX_RATE || !first || !seq || !out ||
        (mode != KPX_RESAMPLE_LINEAR && mode != KPX_RESAMPLE_CUBIC) || (mode == KPX_RESAMPLE_CUBIC && N < 2))
        return KPX_EINVAL;
    if ((long long)B * N > 0x7fffffffLL / (2LL * K * F)) return KPX_EINVAL;
    const long long total = (long long)B * N * F * K * 2;
    const uintptr_t used = (uintptr_t)first | (uintptr_t)seq | (uintptr_t)out;
    if (used & 3) return KPX_EINVAL;
    const bool vec = K % 2 == 0 && (used & 15) == 0;
    hipStream_t s = kpx_stream(stream);
    if (mode == KPX_RESAMPLE_LINEAR)
        rs_launch<KPX_RESAMPLE_LINEAR>(first, seq, N, K, F, total, out, vec, s);
    else
        rs_launch<KPX_RESAMPLE_CUBIC>(first, seq, N, K, F, total, out, vec, s);
    return kpx_launch_status();
}

extern "C" int kpx_points_speed_f64(const float* first, const float* seq, int B, int T, int K, double scale, double* speed, void* stream) {
    if (B < 1 || T < 1 || K < 1 || K > KPX_RESAMPLE_MAX_POINTS || !first || !seq || !speed) return KPX_EINVAL;
    if ((long long)B * T > 0x7fffffffLL / (2LL * K)) return KPX_EINVAL;
    if ((((uintptr_t)first | (uintptr_t)seq) & 3) || ((uintptr_t)speed & 7)) return KPX_EINVAL;
    const int frames = B * T, need = (frames + RS_THREADS - 1) / RS_THREADS;
    const dim3 grid(need > RS_MAX_BLOCKS ? RS_MAX_BLOCKS : need), block(RS_THREADS);
    hipLaunchKernelGGL(points_speed_kernel, grid, block, 0, kpx_stream(stream), first, seq, T, K, frames, scale, speed);
    return kpx_launch_status();
}
