// The approximate posterior of the sequence VAE at inference (evaluate.py --posterior, animate.py --interpolate / --motion-from,
// kpx_amd/posterior.py).  DESIGN.md sections 2 and 4.4; the definitions, to the bit, in include/kpx.h.
//
// All three entries read logit = [mu | sigma] fp32 [B, 2V] as kpx_vae_sample_kl_fwd_f32 does (csrc/rollout.hip).
//
// kpx_latent_stats_add_f64: ONE workgroup, thread v owns the columns (g, v) of every group g.  The rows go by in ascending b; a row is
//   judged by the whole workgroup (its group, then its 2V values), and where it counts thread v adds its eight fields to state[g][v] in
//   global memory, read back by the same thread at the next row of that group.  So a column is summed in ascending b from what `state`
//   held, whatever B is: pieces of any sizes leave the bits of one call.  No atomics.  The launch is latency-bound (a few us per row at the
//   B <= 64 of evaluate.py) and nothing here tries to be faster.
// kpx_latent_sample_f32: one thread per element.
// kpx_latent_path_f32: one wavefront per row for the three dot products, then its lanes write the S steps of that row.
#include "kpx_common.h"

namespace {

constexpr int LS_FIELDS = KPX_LATENT_STATE_FIELDS;

// kl of one (mu, sigma) in fp64 from the fp32 values: every operation rounded once, in this order
__device__ __forceinline__ double ls_kl(float mu, float sd) {
#pragma clang fp contract(off)
    const double m = (double)mu, s = (double)sd;
    const double s2 = s * s;                                            // exact: 24 x 24 bits
    return 0.5 * ((((m * m) + s2) - log((double)1e-8f + s2)) - 1.0);
}

__device__ __forceinline__ bool ls_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN and +-Inf

// threads = V rounded up to whole wavefronts (<= 1024); dynamic LDS: none
__global__ __launch_bounds__(1024) void latent_stats_add_kernel(const float* __restrict__ logit, int B, int V, const int32_t* __restrict__ group,
                                                                int G, double* __restrict__ state, long long* __restrict__ counts,
                                                                double* __restrict__ kl_rows) {
#pragma clang fp contract(off)
    __shared__ double wave_kl[16];
    const int v = threadIdx.x, lane = v & 63, wave = v >> 6, waves = blockDim.x >> 6;
    const bool mine = v < V;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int b = 0; b < B; ++b) {
        const int g = group ? group[b] : 0;                            // the same value in every thread
        if (g < 0 || g >= G) {
            if (v == 0) {
                counts[2] += 1;                                        // group 0's third field
                if (kl_rows) kl_rows[b] = nan;
            }
            continue;
        }
        float mu = 0.f, sd = 0.f;
        if (mine) {
            mu = logit[(size_t)b * 2 * V + v];
            sd = logit[(size_t)b * 2 * V + V + v];
        }
        const int ok = __syncthreads_and(ls_finite(mu) && ls_finite(sd));
        if (!ok) {
            if (v == 0) {
                counts[(size_t)g * 3 + 1] += 1;
                if (kl_rows) kl_rows[b] = nan;
            }
            continue;
        }
        const double kl = mine ? ls_kl(mu, sd) : 0.0;
        if (mine) {
            double* st = state + ((size_t)g * V + v) * LS_FIELDS;
            const double m = (double)mu, s = (double)sd;
            st[0] += m;
            st[1] += m * m;
            st[2] += s;
            st[3] += s * s;
            st[4] += kl;
            st[5] += mu == 0.f ? 1.0 : 0.0;
            st[6] += sd == 0.f ? 1.0 : 0.0;
            st[7] += 1.0;
        }
        if (kl_rows) {                                                 // sum_v kl: the xor butterfly inside a wavefront, the wavefronts in ascending order
            const double w = kpx_wave_sum_d(kl);
            if (lane == 0) wave_kl[wave] = w;
            __syncthreads();
            if (v == 0) {
                double s = wave_kl[0];
                for (int i = 1; i < waves; ++i) s += wave_kl[i];
                kl_rows[b] = s;
            }
            __syncthreads();                                           // wave_kl is written again at the next row
        }
        if (v == 0) counts[(size_t)g * 3] += 1;
    }
}

__global__ __launch_bounds__(256) void latent_sample_kernel(const float* __restrict__ logit, const float* __restrict__ eps, float tau,
                                                            float* __restrict__ z, int B, int V) {
    const int n = B * V;
    const bool mean_only = eps == nullptr || tau == 0.f;
    for (long long idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / V), v = (int)(idx - (long long)b * V);
        const float mu = logit[(size_t)b * 2 * V + v];
        if (mean_only) {
            z[idx] = mu;                                               // mu's bits: sigma and eps are not read
        } else {
            const float sd = logit[(size_t)b * 2 * V + V + v];
            z[idx] = fmaf(kpx_mul_rn(tau, sd), eps[idx], mu);
        }
    }
}

// grid = B workgroups of one wavefront; lane l takes v = l, l + 64, ...
__global__ __launch_bounds__(64) void latent_path_kernel(const float* __restrict__ za, const float* __restrict__ zb, int S, int mode,
                                                         float* __restrict__ out, int B, int V) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* a = za + (size_t)b * V;
    const float* c = zb + (size_t)b * V;
    bool lerp = mode == KPX_LATENT_PATH_LERP;
    double omega = 0.0, sin_omega = 1.0;
    if (!lerp) {
        double aa = 0.0, cc = 0.0, ac = 0.0;
        for (int v = lane; v < V; v += 64) {
            const double x = (double)a[v], y = (double)c[v];
            aa += x * x;                                               // the products are exact in fp64
            cc += y * y;
            ac += x * y;
        }
        aa = kpx_wave_sum_d(aa);
        cc = kpx_wave_sum_d(cc);
        ac = kpx_wave_sum_d(ac);
        if (aa > 0.0 && cc > 0.0) {                                    // false for a zero row and for a NaN
            double cosine = ac / (sqrt(aa) * sqrt(cc));
            cosine = fmin(fmax(cosine, -1.0), 1.0);
            omega = acos(cosine);
            sin_omega = sin(omega);
            lerp = !(sin_omega >= KPX_LATENT_PATH_MIN_SIN);            // a = b, a = -b, or a NaN in the row
        } else {
            lerp = true;
        }
    }
    const size_t step = (size_t)B * V;
    for (int v = lane; v < V; v += 64) {
        const float x = a[v], y = c[v];
        float* o = out + (size_t)b * V + v;
        o[0] = x;
        o[(size_t)(S - 1) * step] = y;
        for (int s = 1; s < S - 1; ++s) {
            const double t = (double)s / (double)(S - 1);
            double ca, cb;
            if (lerp) {
                ca = 1.0 - t;
                cb = t;
            } else {
                ca = sin((1.0 - t) * omega) / sin_omega;
                cb = sin(t * omega) / sin_omega;
            }
            o[(size_t)s * step] = (float)(ca * (double)x + cb * (double)y);
        }
    }
}

bool latent_sizes_ok(int B, int V) {
    return B >= 1 && V >= 1 && V <= KPX_LATENT_MAX_DIM && (long long)B * 2 * V <= 0x7fffffffLL;
}

}  // namespace

extern "C" int kpx_latent_stats_add_f64(const float* logit, int B, int V, const int32_t* group, int G, double* state, int64_t* counts,
                                        double* kl_rows, void* stream) {
    if (!logit || !state || !counts || !latent_sizes_ok(B, V) || G < 1 || (!group && G != 1)) return KPX_EINVAL;
    if ((long long)G * V * LS_FIELDS > 0x7fffffffLL) return KPX_EINVAL;
    if ((((uintptr_t)logit | (uintptr_t)group) & 3) || (((uintptr_t)state | (uintptr_t)counts | (uintptr_t)kl_rows) & 7)) return KPX_EINVAL;
    const int threads = (V + 63) / 64 * 64;
    hipLaunchKernelGGL(latent_stats_add_kernel, dim3(1), dim3(threads), 0, kpx_stream(stream), logit, B, V, group, G, state,
                       reinterpret_cast<long long*>(counts), kl_rows);
    return kpx_launch_status();
}

extern "C" int kpx_latent_sample_f32(const float* logit, const float* eps, float tau, float* z, int B, int V, void* stream) {
    if (!logit || !z || !latent_sizes_ok(B, V) || tau != tau) return KPX_EINVAL;
    if (((uintptr_t)logit | (uintptr_t)eps | (uintptr_t)z) & 3) return KPX_EINVAL;
    const int n = B * V, need = (n + 255) / 256;
    hipLaunchKernelGGL(latent_sample_kernel, dim3(need > 4096 ? 4096 : need), dim3(256), 0, kpx_stream(stream), logit, eps, tau, z, B, V);
    return kpx_launch_status();
}

extern "C" int kpx_latent_path_f32(const float* za, const float* zb, int S, int mode, float* out, int B, int V, void* stream) {
    if (!za || !zb || !out || !latent_sizes_ok(B, V) || S < 2 || S > KPX_LATENT_PATH_MAX_STEPS ||
        (mode != KPX_LATENT_PATH_LERP && mode != KPX_LATENT_PATH_SLERP))
        return KPX_EINVAL;
    if ((long long)S * B * V > 0x7fffffffLL) return KPX_EINVAL;
    if (((uintptr_t)za | (uintptr_t)zb | (uintptr_t)out) & 3) return KPX_EINVAL;
    hipLaunchKernelGGL(latent_path_kernel, dim3(B), dim3(64), 0, kpx_stream(stream), za, zb, S, mode, out, B, V);
    return kpx_launch_status();
}
