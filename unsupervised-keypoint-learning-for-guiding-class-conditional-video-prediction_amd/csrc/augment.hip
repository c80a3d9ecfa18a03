// The image-pair augmentation of data/image_pair_dataloader.py:71-165 + utils/data.py:8-35 on frames that are resident in HBM
// (kpx_amd/resident.py): what ImagePairDataLoader.render does with PIL, restated in integer and strictly ordered float32 arithmetic so
// that every byte equals Pillow's.  Two launches per batch:
//
//   geometry  rotate (NEAREST gather, 16.16 fixed point) -> bicubic resize, horizontal pass then vertical pass, each rounding to uint8
//             (22-bit integer coefficients from the host) -> crop -> flip.  One workgroup per (16-row band of the side x side tile, frame):
//             it computes the rows of the horizontally resized frame that its band needs into LDS (side columns only: the crop window),
//             runs the vertical pass out of LDS and writes the uint8 band and the band's sum of luminances.
//   filter    the ten filters of utils/data.py on the uint8 tile (3x3 / 5x5 kernels, the four ImageEnhance blends), then the
//             uint8 -> [-1,1] conversion of kpx_u8_to_unit_f32.  One thread per pixel, side * side / 256 workgroups per frame.
//
// Both kernels are templates on the tile side: SIDE = 128 is the reference's size with every index a shift (kpx_augment_geometry_u8 /
// kpx_augment_filter_f32), SIDE = 0 takes the side as an argument (the *_sq_* entries: any multiple of 16 in [32, 256]).  A workgroup walks
// its items 256 at a time; the (row, column) of an item advances by (256 / side, 256 % side) with one carry, so no loop divides.
//
// Every decision and every constant that involves double precision comes from the host in the row table (include/kpx.h): the kernels
// only do 32-bit integer arithmetic and float32 operations with one rounding each (kpx_*_rn: no fma).
#include "kpx_common.h"

enum { R_FRAME = 0, R_W, R_H, R_X0, R_Y0, R_FLAGS, R_FILT, R_FVAL, R_A0, R_A1, R_A2, R_A3, R_A4, R_A5, R_HTAB, R_HSTRIDE, R_VTAB, R_VSTRIDE };

#define AUG_REF_TILE 128                                          // the side of the entries without a `side` argument

__device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <int SIDE>
__global__ __launch_bounds__(256) void augment_geometry_kernel(const unsigned char* __restrict__ frames, const int64_t* __restrict__ frame_off,
                                                               const int32_t* __restrict__ rows, const int32_t* __restrict__ tabs, int cap,
                                                               int side_arg, unsigned char* __restrict__ tiles, int32_t* __restrict__ lsum) {
    extern __shared__ unsigned char inter[];                     // [<= cap][side][3]: rows ir0.. of the horizontally resized frame, crop columns only
    __shared__ int red[4];
    const int side = SIDE ? SIDE : side_arg;
    const int step_r = 256 / side, step_c = 256 % side;          // 256 items further: step_r rows and step_c columns (side >= 32: step_c < side)
    const int n = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const int32_t* row = rows + (size_t)n * KPX_AUG_ROW_INTS;
    const int w = row[R_W], h = row[R_H], x0 = row[R_X0], flags = row[R_FLAGS];
    const int a0 = row[R_A0], a1 = row[R_A1], a2 = row[R_A2], a3 = row[R_A3], a4 = row[R_A4], a5 = row[R_A5];
    const int hs = row[R_HSTRIDE], vs = row[R_VSTRIDE];
    const int32_t* ht = tabs + row[R_HTAB];
    const int32_t* vt = tabs + row[R_VTAB];
    const unsigned char* src = frames + frame_off[row[R_FRAME]];
    const bool rot = (flags & KPX_AUG_ROTATE) != 0;
    const int yo0 = row[R_Y0] + band * KPX_AUG_BAND;             // first row of the band in the resized frame

    const int ir0 = vt[yo0 * vs];
    int ir1 = ir0;
    for (int r = 0; r < KPX_AUG_BAND; ++r) ir1 = max(ir1, vt[(yo0 + r) * vs] + vt[(yo0 + r) * vs + 1]);
    const int ni = min(ir1 - ir0, cap);                          // the host has checked ir1 - ir0 <= cap; never write past the LDS block

    // horizontal pass (Pillow: ImagingResampleHorizontal_8bpc) on the rotated frame; the rotation is a gather folded into the loads
    int ri = tid / side, ci = tid - ri * side;
    for (int item = tid; item < ni * side; item += 256) {
        const int y = ir0 + ri;
        const int32_t* e = ht + (x0 + ci) * hs;
        const int xm = e[0], cnt = e[1];
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int t = 0; t < cnt; ++t) {
            const int x = xm + t;
            int xi = x, yi = y;
            if (rot) { xi = (a2 + a1 * y + a0 * x) >> 16; yi = (a5 + a4 * y + a3 * x) >> 16; }
            if ((unsigned)xi < (unsigned)w && (unsigned)yi < (unsigned)h) {      // outside: fill 0
                const unsigned char* p = src + ((size_t)yi * w + xi) * 3;
                const int k = e[2 + t];
                s0 += k * p[0]; s1 += k * p[1]; s2 += k * p[2];
            }
        }
        inter[item * 3 + 0] = (unsigned char)aug_clip8(s0 >> 22);
        inter[item * 3 + 1] = (unsigned char)aug_clip8(s1 >> 22);
        inter[item * 3 + 2] = (unsigned char)aug_clip8(s2 >> 22);
        ri += step_r; ci += step_c;
        if (ci >= side) { ci -= side; ++ri; }
    }
    __syncthreads();

    // vertical pass out of LDS, crop (the band's rows / the side columns are the crop window), flip, luminance sum
    int lpart = 0;
    int r = tid / side, j = tid - r * side;
    for (int item = tid; item < KPX_AUG_BAND * side; item += 256) {
        const int32_t* e = vt + (yo0 + r) * vs;
        const int xm = e[0] - ir0;
        const int cnt = min(e[1], ni - xm);
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int t = 0; t < cnt; ++t) {
            const unsigned char* p = inter + ((xm + t) * side + j) * 3;
            const int k = e[2 + t];
            s0 += k * p[0]; s1 += k * p[1]; s2 += k * p[2];
        }
        const int v0 = aug_clip8(s0 >> 22), v1 = aug_clip8(s1 >> 22), v2 = aug_clip8(s2 >> 22);
        const int jo = (flags & KPX_AUG_FLIP) ? side - 1 - j : j;
        unsigned char* q = tiles + (size_t)n * side * side * 3 + ((band * KPX_AUG_BAND + r) * side + jo) * 3;
        q[0] = (unsigned char)v0; q[1] = (unsigned char)v1; q[2] = (unsigned char)v2;
        lpart += (19595 * v0 + 38470 * v1 + 7471 * v2 + 32768) >> 16;          // Pillow's L of an RGB pixel
        r += step_r; j += step_c;
        if (j >= side) { j -= side; ++r; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lpart += __shfl_xor(lpart, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = lpart;
    __syncthreads();
    if (tid == 0) lsum[n * gridDim.x + band] = red[0] + red[1] + red[2] + red[3];      // gridDim.x = side / KPX_AUG_BAND bands
}

// ImageFilter kernel of size s x s on one channel of an interior pixel: offset + 0.5, then the kernel rows from the bottom one up, each row
// summed left to right on its own before it joins the accumulator; every product and every sum rounds to float32.
__device__ __forceinline__ int aug_kernel_filter(const unsigned char* __restrict__ t, const float* __restrict__ k, int size, int side, int y, int x, int c) {
    const int r = size >> 1;
    float acc = k[1];
    for (int ky = size - 1; ky >= 0; --ky) {
        const unsigned char* p = t + (((y + ky - r) * side) + x - r) * 3 + c;
        const float* kr = k + 2 + ky * size;
        float rowsum = kpx_mul_rn((float)p[0], kr[0]);
        for (int kx = 1; kx < size; ++kx) rowsum = kpx_add_rn(rowsum, kpx_mul_rn((float)p[kx * 3], kr[kx]));
        acc = kpx_add_rn(acc, rowsum);
    }
    return acc <= 0.0f ? 0 : (acc >= 255.0f ? 255 : (int)acc);
}

template <int SIDE>
__global__ __launch_bounds__(256) void augment_filter_kernel(const unsigned char* __restrict__ tiles, const int32_t* __restrict__ lsum,
                                                             const int32_t* __restrict__ rows, const float* __restrict__ kernels,
                                                             int side_arg, float* __restrict__ out) {
    const int side = SIDE ? SIDE : side_arg;
    const int n = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;           // side * side is a multiple of 256: every thread owns a pixel
    const int y = pix / side, x = pix - y * side;
    const int32_t* row = rows + (size_t)n * KPX_AUG_ROW_INTS;
    const int filt = row[R_FILT], flags = row[R_FLAGS];
    const unsigned char* t = tiles + (size_t)n * side * side * 3;
    int v[3], o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = v[c] = t[pix * 3 + c];

    if (filt >= 0 && filt < 6) {
        const float* k = kernels + filt * KPX_AUG_KERNEL_FLOATS;
        const int size = (int)k[0], r = size >> 1;
        if (y >= r && y < side - r && x >= r && x < side - r) {        // the outer r rows / columns are copied
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = aug_kernel_filter(t, k, size, side, y, x, c);
        }
    } else if (filt >= 6 && !(flags & KPX_AUG_IDENTITY)) {                      // ImageEnhance: blend(degenerate, image, f)
        const float f = __int_as_float(row[R_FVAL]);
        int d[3] = {0, 0, 0};                                                    // Brightness: black
        if (filt == 6) {                                                         // Sharpness: the SMOOTH filter of the tile
            const float* k = kernels + 2 * KPX_AUG_KERNEL_FLOATS;
            const int size = (int)k[0], r = size >> 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = v[c];
            if (y >= r && y < side - r && x >= r && x < side - r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = aug_kernel_filter(t, k, size, side, y, x, c);
            }
        } else if (filt == 8) {                                                  // Color: the pixel's luminance
            d[0] = d[1] = d[2] = (19595 * v[0] + 38470 * v[1] + 7471 * v[2] + 32768) >> 16;
        } else if (filt == 9) {                                                  // Contrast: int(mean luminance of the tile + 0.5)
            // Pillow: int(sum / side^2 + 0.5) in double.  (2 * sum + side^2) / (2 * side^2) in integers is that value for every side: where
            // sum / side^2 + 0.5 is no integer it lies at least 1 / (2 * side^2) >= 2^-17 from one, far above the rounding of a double
            // (2^-45 at 255), and where it is one, sum / side^2 is a multiple of 0.5, which the division delivers exactly.
            const int bands = side / KPX_AUG_BAND, area = side * side;
            int s = 0;
            for (int b = 0; b < bands; ++b) s += lsum[n * bands + b];
            d[0] = d[1] = d[2] = (2 * s + area) / (2 * area);                  // sum <= 255 * 2^16: 2 * sum + area < 2^26
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float df = (float)d[c];
            const float tt = kpx_add_rn(df, kpx_mul_rn(f, kpx_sub_rn((float)v[c], df)));
            o[c] = tt <= 0.0f ? 0 : (tt >= 255.0f ? 255 : (int)tt);            // inside [0,255] for 0 <= f <= 1: the clip is the truncation there
        }
    }
    float* q = out + ((size_t)n * side * side + pix) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = kpx_u8_to_unit((unsigned char)o[c]);
}

static bool aug_side_ok(int side) { return side >= KPX_AUG_TILE_MIN && side <= KPX_AUG_TILE_MAX && side % KPX_AUG_BAND == 0; }

extern "C" int kpx_augment_geometry_u8(const unsigned char* frames, const int64_t* frame_off, const int32_t* rows, int n_rows,
                                       const int32_t* resize_tabs, int band_rows_cap, unsigned char* tiles, int32_t* lsum, void* stream) {
    if (!frames || !frame_off || !rows || !resize_tabs || !tiles || !lsum) return KPX_EINVAL;
    if (n_rows < 0 || n_rows > KPX_AUG_MAX_ROWS || band_rows_cap < KPX_AUG_BAND || band_rows_cap > KPX_AUG_MAX_BAND_ROWS) return KPX_EINVAL;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(augment_geometry_kernel<AUG_REF_TILE>, dim3(KPX_AUG_BANDS, n_rows), dim3(256), (size_t)band_rows_cap * AUG_REF_TILE * 3,
                       kpx_stream(stream), frames, frame_off, rows, resize_tabs, band_rows_cap, AUG_REF_TILE, tiles, lsum);
    return kpx_launch_status();
}

extern "C" int kpx_augment_filter_f32(const unsigned char* tiles, const int32_t* lsum, const int32_t* rows, int n_rows, const float* kernels,
                                      float* out, void* stream) {
    if (!tiles || !lsum || !rows || !kernels || !out) return KPX_EINVAL;
    if (n_rows < 0 || n_rows > KPX_AUG_MAX_ROWS) return KPX_EINVAL;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(augment_filter_kernel<AUG_REF_TILE>, dim3(AUG_REF_TILE * AUG_REF_TILE / 256, n_rows), dim3(256), 0, kpx_stream(stream),
                       tiles, lsum, rows, kernels, AUG_REF_TILE, out);
    return kpx_launch_status();
}

static std::atomic<unsigned long long> aug_attr_mask{0};

extern "C" int kpx_augment_geometry_sq_u8(const unsigned char* frames, const int64_t* frame_off, const int32_t* rows, int n_rows,
                                          const int32_t* resize_tabs, int band_rows_cap, int side, unsigned char* tiles, int32_t* lsum,
                                          void* stream) {
    if (!frames || !frame_off || !rows || !resize_tabs || !tiles || !lsum) return KPX_EINVAL;
    if (!aug_side_ok(side) || n_rows < 0 || n_rows > KPX_AUG_MAX_ROWS || band_rows_cap < KPX_AUG_BAND) return KPX_EINVAL;
    if ((long long)band_rows_cap * side * 3 > KPX_AUG_LDS_BYTES) return KPX_EINVAL;      // more than a workgroup can have: nothing is launched
    if (n_rows == 0) return 0;
    const size_t lds = (size_t)band_rows_cap * side * 3;
    if (lds > 64 * 1024 && kpx_first_use_on_device(&aug_attr_mask)) {                     // above the default limit: opt in once per device
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(augment_geometry_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           KPX_AUG_LDS_BYTES);
        if (e != hipSuccess) return -(int)e;
    }
    hipLaunchKernelGGL(augment_geometry_kernel<0>, dim3(side / KPX_AUG_BAND, n_rows), dim3(256), lds, kpx_stream(stream),
                       frames, frame_off, rows, resize_tabs, band_rows_cap, side, tiles, lsum);
    return kpx_launch_status();
}

extern "C" int kpx_augment_filter_sq_f32(const unsigned char* tiles, const int32_t* lsum, const int32_t* rows, int n_rows, const float* kernels,
                                         int side, float* out, void* stream) {
    if (!tiles || !lsum || !rows || !kernels || !out) return KPX_EINVAL;
    if (!aug_side_ok(side) || n_rows < 0 || n_rows > KPX_AUG_MAX_ROWS) return KPX_EINVAL;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(augment_filter_kernel<0>, dim3(side * side / 256, n_rows), dim3(256), 0, kpx_stream(stream),
                       tiles, lsum, rows, kernels, side, out);
    return kpx_launch_status();
}
