// The fused TF-style Adam update of one flat bucket: the ONE definition of its arithmetic and of its walk over the bucket, shared by the
// host-alpha, device-alpha (loss_optim.hip) and guarded (guard.hip) kernels, which must stay bit-identical to each other (graph replay
// against the eager step, and the guarded step against the plain one, rest on that).
#pragma once
#include "kpx_common.h"

// ApplyAdam (TF 1.12): m += (g-m)(1-b1); v += (g*g-v)(1-b2); p -= m*alpha/(sqrt(v)+eps), with g = gs * gradient.
// Not op-for-op ApplyAdam rounding, whatever the _rn intrinsics suggest: for gfx950 the chain is contracted into fused multiply-adds
// (gs*g - m, m + (..)(1-b1), g*g - v and v + (..)(1-b2) round once each) and the square root is the hardware's 1-ulp one.  What holds is
// a bound around the exact step (tests/loss_optim_ref.py): m' within 16 ulps of |m|+|g|, v' of |v|+g*g, p' within 2 ulps of |p| plus 16
// of the update's magnitude alpha(|m|+|g|)/(sqrt(v')+eps); and g = m = v = 0 leaves p, m and v bit-unchanged.
__device__ __forceinline__ void kpx_adam_tf_element(float& p, float g, float& m, float& v, float alpha, float omb1, float omb2, float eps, float gs) {
    const float gr = g * gs;
    m = __fadd_rn(m, __fmul_rn(__fsub_rn(gr, m), omb1));
    v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(gr, gr), v), omb2));
    p = __fsub_rn(p, __fdiv_rn(__fmul_rn(m, alpha), __fadd_rn(__fsqrt_rn(v), eps)));
}

// One workgroup's share of the bucket (256 lanes, grid stride): 16-byte accesses over n/4*4 elements, then the scalar tail.
// p, g, m, v 16-byte aligned.
__device__ __forceinline__ void kpx_adam_tf_walk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                 size_t n, float alpha, float omb1, float omb2, float eps, float gs) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i], mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pp[j], mj = mm[j], vj = vv[j];
            kpx_adam_tf_element(pj, gg[j], mj, vj, alpha, omb1, omb2, eps, gs);
            pp[j] = pj; mm[j] = mj; vv[j] = vj;
        }
        reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(m)[i] = mm; reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        kpx_adam_tf_element(pi, g[i], mi, vi, alpha, omb1, omb2, eps, gs);
        m[i] = mi; v[i] = vi; p[i] = pi;
    }
}

// Launch geometry of the walk: one f32x4 per lane and pass, at most 2048 workgroups.
static inline unsigned kpx_adam_tf_blocks(size_t n) {
    size_t nb = (n / 4 + 255) / 256;
    if (nb < 1) nb = 1;
    if (nb > 2048) nb = 2048;
    return (unsigned)nb;
}
