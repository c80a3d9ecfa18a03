// Key-point retargeting (FinalModel.run(drive=...), evaluate.py --drive): the [B,T,K,2] sequence a driven rollout feeds the translator,
// built from the source images' detected constellation src_first [B,K,2] and a driver (drv_first [B,K,2], drv_seq [B,T,K,2]); sample b is
// driven by sample j = (b + shift) mod B.  DESIGN.md sections 2 and 4.4.
//   HOLD             out[b,t,k] = src_first[b,k]                                              (bit copy)
//   ABSOLUTE         out[b,t,k] = drv_seq[j,t,k]                                              (bit copy)
//   RELATIVE         out[b,t,k] = fl32(src_first[b,k] + (drv_seq[j,t,k] - drv_first[j,k]))
//   RELATIVE_SCALED  out[b,t,k] = fl32(src_first[b,k] + s_b * (drv_seq[j,t,k] - drv_first[j,k])),  s_b = sqrt(v_src / v_drv)
// with v = sum_k |p_k - mean_k p|^2 of the two frame-0 constellations (s_b = 1 unless both are finite and > 0).  The last two in fp64, every
// operation rounded once (no fma), the sums in the order k = 0..K-1, one rounding to fp32 at the store.
//
// A few KB per call: one workgroup per sample (grid-strided), its T*K*2 values strided over the lanes.  The two spreads of a sample are
// K <= 1024 sequential fp64 terms each: lane 0 of the first wavefront folds the source's, lane 0 of the second the driver's, side by side,
// and the workgroup reads s_b from LDS.  A sample reads its own source and its own driver alone, so a non-finite value stays in the
// outputs that read it.  16-byte accesses when K is even (a row of 2K floats is then whole 16-byte items) and every base is 16-byte
// aligned, 4-byte accesses otherwise: the same values either way.
#include "kpx_common.h"

namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_MAX_BLOCKS = 2048;

// sum_k |p_k - c|^2, c = (sum_k p_k) / K, of one constellation p [K,2]
__device__ double rt_spread(const float* __restrict__ p, int K) {
#pragma clang fp contract(off)
    double sx = 0.0, sy = 0.0;
    for (int k = 0; k < K; ++k) {
        sx += (double)p[2 * k];
        sy += (double)p[2 * k + 1];
    }
    const double cx = sx / (double)K, cy = sy / (double)K;
    double v = 0.0;
    for (int k = 0; k < K; ++k) {
        const double dx = (double)p[2 * k] - cx, dy = (double)p[2 * k + 1] - cy;
        v += dx * dx + dy * dy;
    }
    return v;
}

template <int MODE>
__device__ __forceinline__ float rt_value(float src, float first, float seq, double s) {
#pragma clang fp contract(off)
    if constexpr (MODE == KPX_RETARGET_HOLD) return src;
    else if constexpr (MODE == KPX_RETARGET_ABSOLUTE) return seq;
    else if constexpr (MODE == KPX_RETARGET_RELATIVE) return (float)((double)src + ((double)seq - (double)first));
    else return (float)((double)src + s * ((double)seq - (double)first));
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(RT_THREADS) void points_retarget_kernel(const float* __restrict__ src_first, const float* __restrict__ drv_first,
                                                                     const float* __restrict__ drv_seq, int B, int T, int K, int shift,
                                                                     float* __restrict__ out) {
    constexpr bool SRC = MODE != KPX_RETARGET_ABSOLUTE, DRV = MODE != KPX_RETARGET_HOLD;
    constexpr bool FIRST = MODE == KPX_RETARGET_RELATIVE || MODE == KPX_RETARGET_RELATIVE_SCALED;
    __shared__ double spread[2];
    const int row = 2 * K, n = T * row;                                // values per frame and per sample (B*T*K*2 < 2^31)
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        int j = b + shift;                                             // shift < B
        if (j >= B) j -= B;
        const float* sf = src_first + (size_t)b * row;
        const float* df = DRV ? drv_first + (size_t)j * row : nullptr;
        const float* ds = DRV ? drv_seq + (size_t)j * n : nullptr;
        float* o = out + (size_t)b * n;
        double s = 1.0;
        if constexpr (MODE == KPX_RETARGET_RELATIVE_SCALED) {
            __syncthreads();                                           // the previous sample's readers are done with spread[]
            if (threadIdx.x == 0) spread[0] = rt_spread(sf, K);
            if (threadIdx.x == KPX_WAVE) spread[1] = rt_spread(df, K);
            __syncthreads();
            const double vs = spread[0], vd = spread[1];
            if (vs > 0.0 && vd > 0.0 && vs < __builtin_inf() && vd < __builtin_inf()) s = sqrt(vs / vd);   // NaN fails every comparison
        }
        if constexpr (VEC) {
            for (int e = 4 * threadIdx.x; e < n; e += 4 * RT_THREADS) {     // row % 4 == 0: an item stays inside one frame
                const int r = e % row;
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, f = a, q = a, v;
                if constexpr (SRC) a = *reinterpret_cast<const f32x4*>(sf + r);
                if constexpr (FIRST) f = *reinterpret_cast<const f32x4*>(df + r);
                if constexpr (DRV) q = *reinterpret_cast<const f32x4*>(ds + e);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = rt_value<MODE>(a[i], f[i], q[i], s);
                *reinterpret_cast<f32x4*>(o + e) = v;
            }
        } else {
            for (int e = threadIdx.x; e < n; e += RT_THREADS) {
                const int r = e % row;
                o[e] = rt_value<MODE>(SRC ? sf[r] : 0.f, FIRST ? df[r] : 0.f, DRV ? ds[e] : 0.f, s);
            }
        }
    }
}

template <int MODE>
void rt_launch(const float* src_first, const float* drv_first, const float* drv_seq, int B, int T, int K, int shift, float* out, bool vec,
               hipStream_t s) {
    const dim3 grid(B > RT_MAX_BLOCKS ? RT_MAX_BLOCKS : B), block(RT_THREADS);
    if (vec)
        hipLaunchKernelGGL((points_retarget_kernel<MODE, true>), grid, block, 0, s, src_first, drv_first, drv_seq, B, T, K, shift, out);
    else
        hipLaunchKernelGGL((points_retarget_kernel<MODE, false>), grid, block, 0, s, src_first, drv_first, drv_seq, B, T, K, shift, out);
}

}  // namespace

extern "C" int kpx_points_retarget_f32(const float* src_first, const float* drv_first, const float* drv_seq, int B, int T, int K, int shift,
                                       int mode, float* out, void* stream) {
    if (B < 1 || T < 1 || K < 1 || K > 1024 || shift < 0 || shift >= B || (long long)B * T > 0x7fffffffLL / (2 * K) || !out ||
        mode < KPX_RETARGET_HOLD || mode > KPX_RETARGET_RELATIVE_SCALED)
        return KPX_EINVAL;
    const bool need_src = mode != KPX_RETARGET_ABSOLUTE, need_seq = mode != KPX_RETARGET_HOLD;
    const bool need_first = mode == KPX_RETARGET_RELATIVE || mode == KPX_RETARGET_RELATIVE_SCALED;
    if ((need_src && !src_first) || (need_seq && !drv_seq) || (need_first && !drv_first)) return KPX_EINVAL;
    uintptr_t used = (uintptr_t)out;                                   // the pointers this mode reads or writes
    if (need_src) used |= (uintptr_t)src_first;
    if (need_seq) used |= (uintptr_t)drv_seq;
    if (need_first) used |= (uintptr_t)drv_first;
    if (used & 3) return KPX_EINVAL;
    const bool vec = K % 2 == 0 && (used & 15) == 0;
    hipStream_t s = kpx_stream(stream);
    switch (mode) {
        case KPX_RETARGET_HOLD: rt_launch<KPX_RETARGET_HOLD>(src_first, drv_first, drv_seq, B, T, K, shift, out, vec, s); break;
        case KPX_RETARGET_ABSOLUTE: rt_launch<KPX_RETARGET_ABSOLUTE>(src_first, drv_first, drv_seq, B, T, K, shift, out, vec, s); break;
        case KPX_RETARGET_RELATIVE: rt_launch<KPX_RETARGET_RELATIVE>(src_first, drv_first, drv_seq, B, T, K, shift, out, vec, s); break;
        default: rt_launch<KPX_RETARGET_RELATIVE_SCALED>(src_first, drv_first, drv_seq, B, T, K, shift, out, vec, s); break;
    }
    return kpx_launch_status();
}
