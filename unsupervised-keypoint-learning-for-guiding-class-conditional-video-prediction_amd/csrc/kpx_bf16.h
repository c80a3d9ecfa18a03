// bf16 helpers shared by the kernels of the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16) and the bf16-storage streaming kernels: vector
// types, bit casts, packing / unpacking of bf16 pairs, and the exact three-term split the fp32 configuration's arithmetic rests on.
//
// Arithmetic of the bf16x3 kernels (conv_gemm3.hip, conv_wino43b.hip).  Every fp32 operand is split EXACTLY into three bf16 terms:
//     a = a0 + a1 + a2,   a0 = trunc16(a),  a1 = trunc16(a - a0),  a2 = a - a0 - a1
// (a - a0 has at most 16 significant bits and a - a0 - a1 at most 8, so both subtractions are exact and a2 is a bf16 number: no bit of
// the fp32 value is lost).  The product a*b = sum_ij ai*bj is accumulated with the six terms of weight >= 2^-16,
//     a0*b0 + (a0*b1 + a1*b0) + (a1*b1 + a0*b2 + a2*b0),
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; each bf16 x bf16 product is exact in fp32.  The dropped terms (a1*b2, a2*b1, a2*b2)
// are below 2^-23 |a*b| -- smaller than the rounding of one fp32 accumulation.  Measured against a float64 convolution the result is as
// close as the v_mfma_f32_32x32x2_f32 kernel's (tests/test_ops_gpu.py::test_gemm3_*): this is the fp32 configuration's arithmetic, not the
// bf16 mode.  Six bf16 MFMAs cost 6 x 32 = 192 cycles per 32x32x16 block against 8 x 64 = 512 for the fp32 MFMA, and -- unlike the fp32
// MFMA, which holds its SIMD's issue port -- the bf16 MFMA lets the splitting VALU work and the LDS traffic issue beside it.
// TERMS = 1 keeps only a0*b0: the bf16 configuration's arithmetic (BASELINE configs[2]).
#pragma once
#include "kpx_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

#define KPX_BUF_OOB 0x7ffffff0     // voffset beyond any buffer: the load returns / lands as zeros (out-of-image taps, channel tails, chunks past the end)

// compile-time integer handed to a generic lambda (the double-buffered K loops pick their stage with it)
template <int V> struct kpx_ic { static constexpr int value = V; };

static inline bool kpx_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
}

__device__ __forceinline__ unsigned kpx_bits(float v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ float kpx_float(unsigned v) { return __builtin_bit_cast(float, v); }
// {hi16(b), hi16(a)}: two TRUNCATED bf16 values in one dword, a in the low half
__device__ __forceinline__ unsigned kpx_pack_hi(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
// two floats ROUNDED to bf16 in one dword, a in the low half
__device__ __forceinline__ unsigned kpx_pack2(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 p = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, p);
}
// the two bf16 values of a dword as floats
__device__ __forceinline__ float kpx_bf_lo(unsigned v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float kpx_bf_hi(unsigned v) { return __builtin_bit_cast(float, v & 0xffff0000u); }

// exact three-way split of two floats (see the header); p[t] = packed (term t of a, term t of b), t < TERMS
template <int TERMS>
__device__ __forceinline__ void kpx_split2(float a, float b, unsigned* p) {
    const unsigned ua = kpx_bits(a), ub = kpx_bits(b);
    p[0] = kpx_pack_hi(ua, ub);
    if (TERMS > 1) {
        const float ra = a - kpx_float(ua & 0xffff0000u), rb = b - kpx_float(ub & 0xffff0000u);
        const unsigned va = kpx_bits(ra), vb = kpx_bits(rb);
        p[1] = kpx_pack_hi(va, vb);
        if (TERMS > 2) {
            const float sa = ra - kpx_float(va & 0xffff0000u), sb = rb - kpx_float(vb & 0xffff0000u);
            p[2] = kpx_pack_hi(kpx_bits(sa), kpx_bits(sb));
        }
    }
}
