// Functions one kernel file of libkpx_hip.so calls in another: hidden (not part of the C ABI of include/kpx.h), declared HERE ONLY and
// included by the callers and by the defining files alike, so a definition that drifts from its declaration is a compile error -- they are
// extern "C", a mismatch would otherwise link and pass garbage.  The default arguments live here and nowhere else.
#pragma once
#include "conv_geom.h"

// 32-bit byte offsets into an fp32 tensor: `pixels` pixels at a stride of `ld` floats end below `limit`, which each kernel family keeps as it was written.
static inline bool kpx_offsets_fit(size_t pixels, size_t ld, size_t limit) { return pixels * ld * 4 < limit; }

// conv_gemm3.hip: the gather convolution / weight gradient on the bf16 matrix pipe with fp32 operands split into three bf16 terms
extern "C" __attribute__((visibility("hidden"))) int kpx_gemm3_eligible(const ConvGeom* g);
extern "C" __attribute__((visibility("hidden"))) int kpx_gemm3_launch(ConvGeom g, int bt, int terms, hipStream_t s);
extern "C" __attribute__((visibility("hidden"))) int kpx_wgrad3_eligible(const WgradGeom* g);
extern "C" __attribute__((visibility("hidden"))) int kpx_wgrad3_launch(WgradGeom g, int bm, int terms, hipStream_t s);

// conv_wino.hip: fused Winograd F(2x2,3x3) for the stride-1 3x3 SAME layers, and their weight gradient (S = 0: not eligible)
extern "C" __attribute__((visibility("hidden"))) int kpx_wino_eligible(int N, int H, int W, int K, int Nn, int ldin, const void* in_ptr);
extern "C" __attribute__((visibility("hidden"))) int kpx_wino_conv3x3(const float* in, int N, int H, int W, int K, int ldin, const float* w_hwio, int Cin, int Cout, int dgrad,
                                const float* bias, int act, float* out, int Nn, int ldout, float* U_ws, hipStream_t s);
extern "C" __attribute__((visibility("hidden"))) int kpx_wino_wgrad_splits(int N, int H, int W, int Cin, int Cout);
extern "C" __attribute__((visibility("hidden"))) int kpx_wino_wgrad3x3(const float* x, int N, int H, int W, int Cin, int ldx, const float* dy, int Cout, int lddy,
                                 float* slabs, int S, hipStream_t s);

// conv_rgb.hip: LDS-resident image-input kernels (Cin <= 4), few-output-channels forward; -2 = shape not taken; y16 / dy16: y / dy is bf16
extern "C" __attribute__((visibility("hidden"))) int kpx_conv_rgb_fwd(const float* x, int N, int Hi, int Wi, int Cin, const float* w, int KH, int KW,
                                const float* bias, float* y, int Ho, int Wo, int Cout, int ldy,
                                int stride, int pad_t, int pad_l, int act, hipStream_t s, int y16 = 0);
extern "C" __attribute__((visibility("hidden"))) int kpx_conv_rgb_dgrad(const float* dy, int N, int Ho, int Wo, int Cout, int lddy, const float* w, int KH, int KW,
                                  float* dx, int Hi, int Wi, int Cin, int lddx, int stride, int pad_t, int pad_l, hipStream_t s, int dy16 = 0);
extern "C" __attribute__((visibility("hidden"))) int kpx_conv_few_fwd(const float* x, int N, int Hi, int Wi, int Cin, int ldx, const float* w, int KH, int KW,
                                const float* bias, float* y, int Ho, int Wo, int Cout, int ldy,
                                int stride, int pad_t, int pad_l, int act, hipStream_t s);

// conv_wsmall.hip: weight gradient of the image-input layers (S = 0: not eligible)
extern "C" __attribute__((visibility("hidden"))) int kpx_wsmall_splits(int N, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride);
extern "C" __attribute__((visibility("hidden"))) int kpx_wsmall_launch(const float* x, int N, int Hi, int Wi, int Cin, int ldx, const float* dy, int Ho, int Wo, int Cout, int lddy,
                                 int KH, int KW, int stride, int pad_t, int pad_l, float* slabs, int S, hipStream_t s, int dy16 = 0);
