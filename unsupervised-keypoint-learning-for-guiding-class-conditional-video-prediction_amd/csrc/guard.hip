// The step guard (train.py --guard): a non-finite gradient costs one skipped update instead of the run.
//   health  : one read pass over a bucket's flat gradient -> count of NaN / +-Inf values, sum of squares (fp64) and max |g| of the finite ones
//   adam    : the fused Adam update of loss_optim.hip (kpx_adam.h), taken only when the health record counts no non-finite value
//   clipped : the same update with the gradient scaled to a global norm of at most clip_norm, from the record's sum of squares (--clip-norm)
//   restore : dst = src when the record counts one (the batch-norm moving statistics the forward already overwrote)
// The verdict lives in device memory (KpxGuardHealth) and is read by the launches themselves, like the step size of the device-alpha
// Adam: the step is one captured HIP graph and the host never learns of a skip.  No atomics; every result is bitwise reproducible.
#include "kpx_common.h"
#include "kpx_adam.h"
#include "kpx_health.h"

static_assert(sizeof(KpxGuardHealth) == 32, "KpxGuardHealth is 32 bytes");
static_assert(sizeof(KpxClipState) == 16, "KpxClipState is 16 bytes");

// The gradient is cut into slabs of HEALTH_SLAB elements by element index alone: lane t of the workgroup that takes a slab owns the elements
// base + k*1024 + 4*t + j (k < 16, j < 4) and adds them in ascending (k, j).  Which workgroup takes a slab, and whether the four elements
// arrive as one 16-byte load or four 4-byte loads, changes no operand and no order: the partials are a function of (g[0:n], n) alone.
#define HEALTH_LANES 256
#define HEALTH_ITERS 16
#define HEALTH_SLAB (HEALTH_LANES * 4 * HEALTH_ITERS)      // 16384 elements = 64 KiB

template <bool VEC>
__device__ __forceinline__ void health_slab(const float* __restrict__ g, size_t base, size_t n, HealthAcc& a) {
    const size_t lane0 = base + 4 * (size_t)threadIdx.x;
    if (base + HEALTH_SLAB <= n) {                                // a full slab: no bound to check (uniform over the workgroup)
#pragma unroll 4
        for (int k = 0; k < HEALTH_ITERS; ++k) {
            const size_t i = lane0 + (size_t)k * (HEALTH_LANES * 4);
            float x0, x1, x2, x3;
            if (VEC) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(g + i);
                x0 = x[0]; x1 = x[1]; x2 = x[2]; x3 = x[3];
            } else {
                x0 = g[i]; x1 = g[i + 1]; x2 = g[i + 2]; x3 = g[i + 3];
            }
            health_add(a, x0); health_add(a, x1); health_add(a, x2); health_add(a, x3);
        }
    } else {                                                      // the last slab: 16-byte loads while all four lie inside, then the scalar tail
        for (int k = 0; k < HEALTH_ITERS; ++k) {
            const size_t i = lane0 + (size_t)k * (HEALTH_LANES * 4);
            if (i >= n) break;
            if (VEC && i + 4 <= n) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(g + i);
                health_add(a, x[0]); health_add(a, x[1]); health_add(a, x[2]); health_add(a, x[3]);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (i + j < n) health_add(a, g[i + j]);
            }
        }
    }
}

// work = [S] fp64 sums of squares, then [S] fp32 maxima, then [S] uint32 counts, S = number of slabs
template <bool VEC>
__global__ __launch_bounds__(HEALTH_LANES) void grad_health_partial_kernel(const float* __restrict__ g, size_t n, size_t slabs,
                                                                           double* __restrict__ wsum, float* __restrict__ wmax,
                                                                           unsigned* __restrict__ wbad) {
    __shared__ double sm_s[4];
    __shared__ float sm_m[4];
    __shared__ unsigned sm_b[4];
    for (size_t slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
        HealthAcc a = {0.0, 0.0f, 0u};
        health_slab<VEC>(g, slab * (size_t)HEALTH_SLAB, n, a);
        double s = kpx_wave_sum_d(a.s);
        float mx = kpx_wave_max(a.mx);
        unsigned bad = a.bad;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += (unsigned)__shfl_xor((int)bad, o, 64);
        if ((threadIdx.x & 63) == 0) { sm_s[threadIdx.x >> 6] = s; sm_m[threadIdx.x >> 6] = mx; sm_b[threadIdx.x >> 6] = bad; }
        __syncthreads();
        if (threadIdx.x == 0) {
            wsum[slab] = (sm_s[0] + sm_s[1]) + (sm_s[2] + sm_s[3]);
            wmax[slab] = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
            wbad[slab] = sm_b[0] + sm_b[1] + sm_b[2] + sm_b[3];
        }
        __syncthreads();                                          // the next slab's waves overwrite sm_*
    }
}

// One workgroup folds the slabs in an order that depends on their number alone: lane t adds slabs t, t+256, ... in ascending order, then
// the butterfly over the wavefront and the four wavefronts in order.  The count is carried in fp64 (exact to 2^53) and saturates at 2^32-1.
__global__ __launch_bounds__(HEALTH_LANES) void grad_health_fold_kernel(const double* __restrict__ wsum, const float* __restrict__ wmax,
                                                                        const unsigned* __restrict__ wbad, size_t slabs,
                                                                        KpxGuardHealth* __restrict__ health) {
    double s = 0.0, bad = 0.0;
    float mx = 0.0f;
    for (size_t i = threadIdx.x; i < slabs; i += HEALTH_LANES) {
        s += wsum[i];
        mx = fmaxf(mx, wmax[i]);
        bad += (double)wbad[i];
    }
    s = kpx_wave_sum_d(s); bad = kpx_wave_sum_d(bad); mx = kpx_wave_max(mx);
    __shared__ double sm_s[4], sm_b[4];
    __shared__ float sm_m[4];
    if ((threadIdx.x & 63) == 0) { sm_s[threadIdx.x >> 6] = s; sm_b[threadIdx.x >> 6] = bad; sm_m[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double b = (sm_b[0] + sm_b[1]) + (sm_b[2] + sm_b[3]);
        health->nonfinite = b >= 4294967295.0 ? 0xffffffffu : (unsigned)b;
        health->sumsq = (sm_s[0] + sm_s[1]) + (sm_s[2] + sm_s[3]);
        health->maxabs = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
    }
}

static inline size_t health_slabs(size_t n) { return (n + HEALTH_SLAB - 1) / HEALTH_SLAB; }

extern "C" size_t kpx_grad_health_workspace_bytes(size_t n) { return health_slabs(n) * 16; }

extern "C" int kpx_grad_health_f32(const float* g, size_t n, void* work, KpxGuardHealth* health, void* stream) {
    if (!g || !work || !health || n == 0 || (((uintptr_t)g) & 3) || (((uintptr_t)work) & 7) || (((uintptr_t)health) & 7)) return KPX_EINVAL;
    const size_t slabs = health_slabs(n);
    double* wsum = (double*)work;
    float* wmax = (float*)(wsum + slabs);
    unsigned* wbad = (unsigned*)(wmax + slabs);
    const unsigned nb = (unsigned)(slabs < 2048 ? slabs : 2048);
    hipStream_t s = kpx_stream(stream);
    if ((((uintptr_t)g) & 15) == 0)
        hipLaunchKernelGGL(grad_health_partial_kernel<true>, dim3(nb), dim3(HEALTH_LANES), 0, s, g, n, slabs, wsum, wmax, wbad);
    else
        hipLaunchKernelGGL(grad_health_partial_kernel<false>, dim3(nb), dim3(HEALTH_LANES), 0, s, g, n, slabs, wsum, wmax, wbad);
    int rc = kpx_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(grad_health_fold_kernel, dim3(1), dim3(HEALTH_LANES), 0, s, (const double*)wsum, (const float*)wmax,
                       (const unsigned*)wbad, slabs, health);
    return kpx_launch_status();
}

// Every lane reads health->nonfinite, which no lane of this launch writes: the branch is uniform across the launch.  Lane 0 of workgroup 0
// alone reads and writes the three counters.
__global__ __launch_bounds__(256) void adam_tf_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, size_t n, const float* __restrict__ alpha_dev,
                                                              float omb1, float omb2, float eps, float gs, KpxGuardHealth* health) {
    const bool skip = health->nonfinite != 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        health->updates += 1u;
        if (skip) { health->skipped_total += 1u; health->skipped_run += 1u; }
        else health->skipped_run = 0u;
    }
    if (skip) return;
    kpx_adam_tf_walk(p, g, m, v, n, *alpha_dev, omb1, omb2, eps, gs);
}
extern "C" int kpx_adam_tf_flat_guarded_f32(float* p, const float* g, float* m, float* v, size_t n, const float* alpha_dev,
                                            float beta1, float beta2, float eps, float gscale, KpxGuardHealth* health, void* stream) {
    if (!p || !g || !m || !v || !alpha_dev || !health || n == 0) return KPX_EINVAL;
    if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) || (((uintptr_t)alpha_dev) & 3) || (((uintptr_t)health) & 7))
        return KPX_EINVAL;
    hipLaunchKernelGGL(adam_tf_guarded_kernel, dim3(kpx_adam_tf_blocks(n)), dim3(256), 0, kpx_stream(stream), p, g, m, v, n, alpha_dev,
                       1.0f - beta1, 1.0f - beta2, eps, gscale, health);
    return kpx_launch_status();
}

// The guarded update with tf.clip_by_global_norm over the bucket (train.py --clip-norm).  Every lane derives the norm and the scale from
// health->sumsq and the launch's own arguments, none of which this launch writes: the two branches and gs are uniform across the launch.
// With N <= clip_norm the walk gets gscale itself, the guarded kernel's operand.  Lane 0 of workgroup 0 alone writes the counters and *clip.
__global__ __launch_bounds__(256) void adam_tf_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, size_t n, const float* __restrict__ alpha_dev,
                                                              float omb1, float omb2, float eps, float gscale, float clip_norm,
                                                              KpxGuardHealth* health, KpxClipState* clip) {
    const bool skip = health->nonfinite != 0u;
    const double norm = (double)gscale * sqrt(health->sumsq);
    const bool clipped = norm > (double)clip_norm;
    const double ratio = clipped ? (double)clip_norm / norm : 1.0;
    const float gs = clipped ? (float)((double)gscale * ratio) : gscale;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        health->updates += 1u;
        if (skip) { health->skipped_total += 1u; health->skipped_run += 1u; }
        else {
            health->skipped_run = 0u;
            clip->norm = (float)norm;
            clip->scale = (float)ratio;
            if (clipped) clip->clipped_total += 1u;
        }
    }
    if (skip) return;
    kpx_adam_tf_walk(p, g, m, v, n, *alpha_dev, omb1, omb2, eps, gs);
}
extern "C" int kpx_adam_tf_flat_clipped_f32(float* p, const float* g, float* m, float* v, size_t n, const float* alpha_dev,
                                            float beta1, float beta2, float eps, float gscale, float clip_norm,
                                            KpxGuardHealth* health, KpxClipState* clip, void* stream) {
    if (!p || !g || !m || !v || !alpha_dev || !health || !clip || n == 0 || !(clip_norm > 0.0f)) return KPX_EINVAL;      // (a NaN fails the comparison)
    if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) || ((((uintptr_t)alpha_dev) | ((uintptr_t)clip)) & 3) ||
        (((uintptr_t)health) & 7))
        return KPX_EINVAL;
    hipLaunchKernelGGL(adam_tf_clipped_kernel, dim3(kpx_adam_tf_blocks(n)), dim3(256), 0, kpx_stream(stream), p, g, m, v, n, alpha_dev,
                       1.0f - beta1, 1.0f - beta2, eps, gscale, clip_norm, health, clip);
    return kpx_launch_status();
}

template <bool VEC>
__global__ __launch_bounds__(256) void guard_restore_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n,
                                                            const KpxGuardHealth* __restrict__ health) {
    if (health->nonfinite == 0u) return;
    const size_t n4 = VEC ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
        reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
    const unsigned* s32 = reinterpret_cast<const unsigned*>(src);     // bit for bit: the tail moves words, not floats
    unsigned* d32 = reinterpret_cast<unsigned*>(dst);
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) d32[i] = s32[i];
}
extern "C" int kpx_guard_restore_f32(float* dst, const float* src, size_t n, const KpxGuardHealth* health, void* stream) {
    if (!dst || !src || !health || n == 0 || ((((uintptr_t)dst) | ((uintptr_t)src)) & 3) || (((uintptr_t)health) & 7)) return KPX_EINVAL;
    const bool vec = ((((uintptr_t)dst) | ((uintptr_t)src)) & 15) == 0;
    size_t nb = ((vec ? n / 4 : n) + 255) / 256;
    if (nb < 1) nb = 1;
    if (nb > 2048) nb = 2048;
    if (vec) hipLaunchKernelGGL(guard_restore_kernel<true>, dim3((unsigned)nb), dim3(256), 0, kpx_stream(stream), dst, src, n, health);
    else hipLaunchKernelGGL(guard_restore_kernel<false>, dim3((unsigned)nb), dim3(256), 0, kpx_stream(stream), dst, src, n, health);
    return kpx_launch_status();
}
