// Image summaries: TF 1.12 SummaryImageOp's float -> uint8 conversion (NormalizeFloatImage, core/kernels/summary_image_op.cc) with the
// reference's pre-map ((x+1)/2*255, its clipped form, mask*255: detector_translator_model.py:206-222, motion_generator_model.py:253-266)
// fused into both passes.  An image is walked in groups of 4 pixels; the groups are cut into `slices` contiguous slices, one workgroup each:
//   pass 1  (slices x N workgroups)  finite min / max of the slice -> work[n][s] = {min, max}
//   pass 2  (slices x N workgroups)  every workgroup reduces its image's partials (the same values in the same order: same scale in all of
//                                    them), then converts its slice; a full group of 4 pixels is C 32-bit stores when the image is aligned.
// Min and max of finite values are exact and order-free, so the result does not depend on the slicing; the affine goes through the
// non-contractable kpx_*_rn helpers (an fma would round once where TF rounds twice) and the cast truncates.
#include "kpx_common.h"

namespace {

__device__ __forceinline__ bool sm_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// std::min / std::max as TF calls them: (b < a) ? b : a and (a < b) ? b : a
__device__ __forceinline__ float sm_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float sm_max(float a, float b) { return a < b ? b : a; }

template <int PREMAP>
__device__ __forceinline__ float premap(float x) {
    if (PREMAP == KPX_PREMAP_X255) return kpx_mul_rn(x, 255.0f);                                    // mask * 255.0
    if (PREMAP == KPX_PREMAP_UNIT255 || PREMAP == KPX_PREMAP_UNIT255_CLIP) {
        float v = kpx_mul_rn(kpx_mul_rn(kpx_add_rn(x, 1.0f), 0.5f), 255.0f);                          // (x + 1) / 2.0 * 255.0 (/2 == *0.5 exactly)
        if (PREMAP == KPX_PREMAP_UNIT255_CLIP) v = sm_max(sm_min(v, 255.0f), 0.0f);                // clip_by_value: minimum, then maximum
        return v;
    }
    return x;
}

// The C channels of pixel p, pre-mapped; returns whether all are finite.
template <int PREMAP, int C>
__device__ __forceinline__ bool load_pixel(const float* __restrict__ x, size_t p, float v[C]) {
    bool fin = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        v[c] = premap<PREMAP>(x[p * C + c]);
        fin = fin && sm_finite(v[c]);
    }
    return fin;
}

__device__ __forceinline__ void slice_range(int groups, int slices, int s, int& g0, int& g1) {
    g0 = (int)((long long)groups * s / slices);
    g1 = (int)((long long)groups * (s + 1) / slices);
}

template <int PREMAP, int C>
__global__ __launch_bounds__(256) void summary_minmax_kernel(const float* __restrict__ x, int P, int slices, float* __restrict__ work) {
    const int s = blockIdx.x, n = blockIdx.y, groups = (P + 3) / 4;
    int g0, g1;
    slice_range(groups, slices, s, g0, g1);
    const float* xn = x + (size_t)n * P * C;
    float mn = __int_as_float(0x7f800000), mx = -mn;
    for (int g = g0 + (int)threadIdx.x; g < g1; g += 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = 4 * g + j;
            if (p < P) {
                float v[C];
                if (load_pixel<PREMAP, C>(xn, p, v)) {
#pragma unroll
                    for (int c = 0; c < C; ++c) { mn = sm_min(mn, v[c]); mx = sm_max(mx, v[c]); }
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = sm_min(mn, __shfl_xor(mn, o, 64));
        mx = sm_max(mx, __shfl_xor(mx, o, 64));
    }
    __shared__ float red[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = mn; red[1][wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = red[0][0]; mx = red[1][0];
        for (int w = 1; w < 4; ++w) { mn = sm_min(mn, red[0][w]); mx = sm_max(mx, red[1][w]); }
        float* o = work + ((size_t)n * slices + s) * 2;
        o[0] = mn;
        o[1] = mx;
    }
}

__device__ __forceinline__ uint32_t pack4(const uint8_t* b) {
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

template <int PREMAP, int C, bool VEC>
__global__ __launch_bounds__(256) void summary_convert_kernel(const float* __restrict__ x, int P, int slices, const float* __restrict__ work,
                                                              uint8_t* __restrict__ out) {
    const int s = blockIdx.x, n = blockIdx.y, groups = (P + 3) / 4;
    // the image's min / max: every workgroup of image n folds the same partials in the same order
    const float* wn = work + (size_t)n * slices * 2;
    float mn = wn[0], mx = wn[1];
    for (int i = 1; i < slices; ++i) { mn = sm_min(mn, wn[2 * i]); mx = sm_max(mx, wn[2 * i + 1]); }
    float scale, offset;
    if (mn < 0.0f) {
        const float m = sm_max(fabsf(mn), fabsf(mx));
        scale = m < 1e-6f ? 0.0f : __fdiv_rn(127.0f, m);
        offset = 128.0f;
    } else {
        scale = mx < 1e-6f ? 0.0f : __fdiv_rn(255.0f, mx);
        offset = 0.0f;
    }
    int g0, g1;
    slice_range(groups, slices, s, g0, g1);
    const float* xn = x + (size_t)n * P * C;
    uint8_t* on = out + (size_t)n * P * C;
    for (int g = g0 + (int)threadIdx.x; g < g1; g += 256) {
        uint8_t b[4 * C];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = 4 * g + j;
            float v[C];
            const bool fin = p < P && load_pixel<PREMAP, C>(xn, p, v);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                // finite pixel: uint8(trunc(fl(fl(x*scale) + offset))), in [0, 256); otherwise the bad colour (255,0,0,255)[:C]
                b[j * C + c] = fin ? (uint8_t)(uint32_t)kpx_add_rn(kpx_mul_rn(v[c], scale), offset) : (uint8_t)(c == 0 || c == 3 ? 255 : 0);
            }
        }
        if (VEC && 4 * g + 3 < P) {                     // the group's 4*C bytes start on a 4-byte boundary: C dword stores
            uint32_t* o = reinterpret_cast<uint32_t*>(on + (size_t)4 * g * C);
#pragma unroll
            for (int q = 0; q < C; ++q) o[q] = pack4(b + 4 * q);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * g + j < P)
#pragma unroll
                    for (int c = 0; c < C; ++c) on[(size_t)(4 * g + j) * C + c] = b[j * C + c];
        }
    }
}

template <int PREMAP, int C>
int summary_launch(const float* x, int N, int P, float* work, uint8_t* out, hipStream_t s) {
    const int groups = (P + 3) / 4;
    int slices = (groups + 255) / 256;                  // one group per thread in a full slice ...
    slices = slices < 1 ? 1 : slices > KPX_SUMMARY_SLICES ? KPX_SUMMARY_SLICES : slices;   // ... up to KPX_SUMMARY_SLICES per image
    const dim3 grid(slices, N), block(256);
    hipLaunchKernelGGL((summary_minmax_kernel<PREMAP, C>), grid, block, 0, s, x, P, slices, work);
    int rc = kpx_launch_status();
    if (rc) return rc;
    const bool vec = P % 4 == 0 && (((uintptr_t)out) & 3) == 0;     // every image, and every group in it, starts on a 4-byte boundary
    if (vec)
        hipLaunchKernelGGL((summary_convert_kernel<PREMAP, C, true>), grid, block, 0, s, x, P, slices, (const float*)work, out);
    else
        hipLaunchKernelGGL((summary_convert_kernel<PREMAP, C, false>), grid, block, 0, s, x, P, slices, (const float*)work, out);
    return kpx_launch_status();
}

template <int PREMAP>
int summary_dispatch_c(const float* x, int N, int P, int C, float* work, uint8_t* out, hipStream_t s) {
    if (C == 1) return summary_launch<PREMAP, 1>(x, N, P, work, out, s);
    if (C == 3) return summary_launch<PREMAP, 3>(x, N, P, work, out, s);
    return summary_launch<PREMAP, 4>(x, N, P, work, out, s);
}

}  // namespace

extern "C" int kpx_summary_image_u8_f32(const float* x, int N, int H, int W, int C, int premap, float* work, uint8_t* out, void* stream) {
    if (!x || !work || !out || N < 1 || N > 65535 || H < 1 || W < 1 || !(C == 1 || C == 3 || C == 4) || premap < KPX_PREMAP_IDENTITY ||
        premap > KPX_PREMAP_UNIT255_CLIP || (size_t)H * W > 0x1fffffff)
        return KPX_EINVAL;
    const int P = H * W;
    hipStream_t s = kpx_stream(stream);
    switch (premap) {
        case KPX_PREMAP_X255: return summary_dispatch_c<KPX_PREMAP_X255>(x, N, P, C, work, out, s);
        case KPX_PREMAP_UNIT255: return summary_dispatch_c<KPX_PREMAP_UNIT255>(x, N, P, C, work, out, s);
        case KPX_PREMAP_UNIT255_CLIP: return summary_dispatch_c<KPX_PREMAP_UNIT255_CLIP>(x, N, P, C, work, out, s);
        default: return summary_dispatch_c<KPX_PREMAP_IDENTITY>(x, N, P, C, work, out, s);
    }
}
