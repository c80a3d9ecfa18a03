// The averaged generator (train.py --ema): an exponential moving average of a bucket's parameters, kept beside training and read only
// for inference.
//   ema  : ema += (p - ema) * rate over one flat bucket, rate read from device memory; nothing when the step guard's record counts a
//          non-finite gradient value (the update was skipped, so the average does not take a step either)
//   swap : exchange two flat ranges word for word (BaseModel.ema_weights(): parameters <-> averages, in place, no address changes)
// Both follow guard.hip: the scalars the step changes live in device memory and are read by the launch itself, so the launch is part of
// the captured step; no atomics, no allocation, no synchronisation; every result is a function of the operands alone.
#include "kpx_common.h"

// tf.train.ExponentialMovingAverage / assign_moving_average with rate = 1 - decay: e -= (e - p) * rate.  THE definition of the arithmetic:
// d = p - e rounds once, then e' = fma(d, rate, e) rounds once (the uncontracted form, d * rate then the sum, has three roundings; either
// stays within 3 * 2^-24 * (|e| + |p|) of the exact value, tests/ema_ref.py).  e == p gives d = +0 and e' = e bit for bit (e != -0).
__device__ __forceinline__ float kpx_ema_element(float e, float p, float rate) {
    const float d = __fsub_rn(p, e);
    return __fmaf_rn(d, rate, e);
}

// The streaming walk of kpx_adam.h: 256 lanes, one f32x4 per lane and pass, grid stride, then the scalar tail.  Every lane reads
// health->nonfinite, which no lane of this launch writes: the branch is uniform across the launch.  health is only read.
__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n,
                                                       const float* __restrict__ rate_dev, const KpxGuardHealth* __restrict__ health) {
    if (health != nullptr && health->nonfinite != 0u) return;
    const float rate = *rate_dev;
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
        const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) ee[j] = kpx_ema_element(ee[j], pp[j], rate);
        reinterpret_cast<f32x4*>(ema)[i] = ee;
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        ema[i] = kpx_ema_element(ema[i], p[i], rate);
}

// One f32x4 per lane and pass, at most 2048 workgroups (the geometry of kpx_adam_tf_blocks).
static inline unsigned ema_blocks(size_t n) {
    size_t nb = (n / 4 + 255) / 256;
    if (nb < 1) nb = 1;
    if (nb > 2048) nb = 2048;
    return (unsigned)nb;
}

extern "C" int kpx_ema_flat_f32(float* ema, const float* p, size_t n, const float* rate_dev, const KpxGuardHealth* health, void* stream) {
    if (!ema || !p || !rate_dev || n == 0) return KPX_EINVAL;
    if (((((uintptr_t)ema) | ((uintptr_t)p)) & 15) || (((uintptr_t)rate_dev) & 3) || (((uintptr_t)health) & 7)) return KPX_EINVAL;
    hipLaunchKernelGGL(ema_flat_kernel, dim3(ema_blocks(n)), dim3(256), 0, kpx_stream(stream), ema, p, n, rate_dev, health);
    return kpx_launch_status();
}

// Each element is read and written by one lane only, and the two ranges do not overlap: no ordering between lanes is needed.
__global__ __launch_bounds__(256) void swap_flat_kernel(float* __restrict__ a, float* __restrict__ b, size_t n) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 x = reinterpret_cast<const f32x4*>(a)[i], y = reinterpret_cast<const f32x4*>(b)[i];
        reinterpret_cast<f32x4*>(a)[i] = y;
        reinterpret_cast<f32x4*>(b)[i] = x;
    }
    unsigned* a32 = reinterpret_cast<unsigned*>(a);                   // bit for bit: the tail moves words, not floats
    unsigned* b32 = reinterpret_cast<unsigned*>(b);
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned x = a32[i], y = b32[i];
        a32[i] = y;
        b32[i] = x;
    }
}

extern "C" int kpx_swap_flat_f32(float* a, float* b, size_t n, void* stream) {
    if (!a || !b || a == b || n == 0 || ((((uintptr_t)a) | ((uintptr_t)b)) & 15)) return KPX_EINVAL;
    hipLaunchKernelGGL(swap_flat_kernel, dim3(ema_blocks(n)), dim3(256), 0, kpx_stream(stream), a, b, n);
    return kpx_launch_status();
}
