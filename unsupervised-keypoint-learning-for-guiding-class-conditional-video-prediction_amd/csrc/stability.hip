// The detector's equivariance score (make_pseudo_labels.py --stability, kpx_amd/stability.py): move every frame by a
// known affine map, detect again, and measure how far the detected points are from where the map sends the original ones.
//
//   kpx_affine_warp_f32          out[r] = frame rows[r] of `in` resampled through the inverse map coef[r] (pixel units): bilinear, edges
//                                replicated.  Per output pixel (x, y), all in fp64, every product and sum rounded once (no fma), one rounding
//                                to fp32 at the store:
//                                  sx = (c0*x + c1*y) + c2, sy = (c3*x + c4*y) + c5, clamped to [0, W-1] and [0, H-1] (NaN -> 0)
//                                  x0 = floor(sx), lowered to max(W-2, 0) when it exceeds W-2; fx = sx - x0; x1 = min(x0 + 1, W-1); y alike
//                                  top = (1-fx)*v00 + fx*v01, bot = (1-fx)*v10 + fx*v11, out = (1-fy)*top + fy*bot
//                                so a numpy float64 restatement gives the same bits, and maps that send pixels to pixels (identity, integer
//                                shifts, flips, quarter turns of a square frame) copy the input's bits (fx and fy are then 0 or 1).
//   kpx_equivariance_scores_f32  per row and point the distance between the point detected on the warped frame and the mapped original,
//                                and the distance the map moved the original; per row their means over the valid points.
//
// The warp: a workgroup owns a 16-row output tile of one row of the table, so the slanted source footprint of a tile stays in L1 / L2, and
// the tiles of one frame run on one XCD (kpx_xcd_remap).  A lane computes four neighbouring pixels and stores them as 16-byte items when
// W % 4 == 0 and `out` is 16-byte aligned, one pixel with 4-byte stores otherwise: the same arithmetic per pixel, the same bits.  The taps
// are 4-byte loads at any alignment.  The clamp keeps every tap inside the frame whatever the coefficients are; the frame number is trusted
// (kpx_amd.ops.affine_warp checks the table on the host).
//
// The scores: one wavefront per row; a lane computes point k0 + lane of each group of 64 points, and the row's sums are folded lane by lane
// in ascending k (every lane holds the same chain), so the order of the additions does not depend on the launch.  No LDS, no atomics.
#include "kpx_common.h"

namespace {

constexpr int AW_THREADS = 256, AW_TILE = 16;                          // 16 x 16 lanes; 16 rows of 16 (or 64) pixels
constexpr int EQ_THREADS = 256, EQ_ROWS = EQ_THREADS / KPX_WAVE;

template <int C>
__device__ __forceinline__ void aw_pixel(const float* __restrict__ src, int H, int W, const double (&c)[6], int x, int y, float* __restrict__ o) {
#pragma clang fp contract(off)
    const double xd = (double)x, yd = (double)y, xmax = (double)(W - 1), ymax = (double)(H - 1);
    double sx = (c[0] * xd + c[1] * yd) + c[2];
    double sy = (c[3] * xd + c[4] * yd) + c[5];
    sx = !(sx >= 0.0) ? 0.0 : (sx > xmax ? xmax : sx);                 // edge replication; a NaN (overflowing coefficients) reads pixel 0
    sy = !(sy >= 0.0) ? 0.0 : (sy > ymax ? ymax : sy);
    int x0 = (int)floor(sx), y0 = (int)floor(sy);
    if (x0 > W - 2) x0 = W - 2 > 0 ? W - 2 : 0;
    if (y0 > H - 2) y0 = H - 2 > 0 ? H - 2 : 0;
    const double fx = sx - (double)x0, fy = sy - (double)y0;
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const float* r0 = src + (size_t)y0 * W * C;
    const float* r1 = src + (size_t)y1 * W * C;
    const double gx = 1.0 - fx, gy = 1.0 - fy;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const double v00 = (double)r0[x0 * C + ch], v01 = (double)r0[x1 * C + ch];
        const double v10 = (double)r1[x0 * C + ch], v11 = (double)r1[x1 * C + ch];
        const double top = gx * v00 + fx * v01;
        const double bot = gx * v10 + fx * v11;
        o[ch] = (float)(gy * top + fy * bot);
    }
}

// PX = 4: W % 4 == 0 and out 16-byte aligned, so the 4 * C values of a lane are C whole 16-byte items
template <int C, int PX>
__global__ __launch_bounds__(AW_THREADS) void affine_warp_kernel(const float* __restrict__ in, int H, int W, const int32_t* __restrict__ rows,
                                                                 const double* __restrict__ coef, int tiles_x, int tiles, float* __restrict__ out) {
    const int bid = kpx_xcd_remap(blockIdx.x, gridDim.x);              // R * tiles <= 2^16 * 2^12
    const int r = bid / tiles, t = bid - r * tiles;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y = ty * AW_TILE + (threadIdx.x >> 4), x = (tx * AW_TILE + (threadIdx.x & 15)) * PX;
    if (y >= H || x >= W) return;
    double c[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = coef[(size_t)r * 6 + i];
    const float* src = in + (size_t)rows[r] * H * W * C;
    float* dst = out + (((size_t)r * H + y) * W + x) * C;
    if constexpr (PX == 4) {
        float v[4 * C];
#pragma unroll
        for (int p = 0; p < 4; ++p) aw_pixel<C>(src, H, W, c, x + p, y, v + p * C);
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const f32x4 item = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
            *reinterpret_cast<f32x4*>(dst + 4 * q) = item;
        }
    } else {
        float v[C];
        aw_pixel<C>(src, H, W, c, x, y, v);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) dst[ch] = v[ch];
    }
}

template <int C>
void aw_launch(const float* in, int H, int W, const int32_t* rows, const double* coef, int R, float* out, bool vec, hipStream_t s) {
    const int tiles_x = (W + AW_TILE * (vec ? 4 : 1) - 1) / (AW_TILE * (vec ? 4 : 1)), tiles = tiles_x * ((H + AW_TILE - 1) / AW_TILE);
    const dim3 grid((unsigned)(R * tiles)), block(AW_THREADS);
    if (vec)
        hipLaunchKernelGGL((affine_warp_kernel<C, 4>), grid, block, 0, s, in, H, W, rows, coef, tiles_x, tiles, out);
    else
        hipLaunchKernelGGL((affine_warp_kernel<C, 1>), grid, block, 0, s, in, H, W, rows, coef, tiles_x, tiles, out);
}

__device__ __forceinline__ bool eq_finite(double v) { return fabs(v) < __builtin_inf(); }   // false for NaN

__global__ __launch_bounds__(EQ_THREADS) void equivariance_scores_kernel(const float* __restrict__ pts, const float* __restrict__ pts_w,
                                                                         const int32_t* __restrict__ rows, const double* __restrict__ fwd, int R,
                                                                         int K, float* __restrict__ out, uint8_t* __restrict__ valid,
                                                                         float* __restrict__ frame_mean, int32_t* __restrict__ n_valid) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (KPX_WAVE - 1);
    const int r = blockIdx.x * EQ_ROWS + (threadIdx.x >> 6);           // one wavefront per row: it leaves or stays as a whole
    if (r >= R) return;
    const double* m = fwd + (size_t)r * 6;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const float* p = pts + (size_t)rows[r] * K * 2;
    const float* q = pts_w + (size_t)r * K * 2;
    double sum_err = 0.0, sum_moved = 0.0;
    int n = 0;
    for (int k0 = 0; k0 < K; k0 += KPX_WAVE) {
        const int k = k0 + lane;
        double e = 0.0, mv = 0.0;
        bool ok = false;
        if (k < K) {
            const double px = (double)p[2 * k], py = (double)p[2 * k + 1], qx = (double)q[2 * k], qy = (double)q[2 * k + 1];
            const double tx = (m0 * px + m1 * py) + m2, ty = (m3 * px + m4 * py) + m5;
            const double dx = qx - tx, dy = qy - ty, ux = tx - px, uy = ty - py;
            const double err = sqrt(dx * dx + dy * dy), moved = sqrt(ux * ux + uy * uy);
            ok = eq_finite(px) && eq_finite(py) && eq_finite(qx) && eq_finite(qy) && tx >= -1.0 && tx <= 1.0 && ty >= -1.0 && ty <= 1.0;
            const size_t i = (size_t)r * K + k;
            out[2 * i] = (float)err;
            out[2 * i + 1] = (float)moved;
            valid[i] = ok ? 1 : 0;
            if (ok) { e = err; mv = moved; }
        }
        for (int l = 0; l < KPX_WAVE; ++l) {                           // ascending k; an entry that is not valid adds +0 to a sum >= +0
            sum_err += __shfl(e, l, KPX_WAVE);
            sum_moved += __shfl(mv, l, KPX_WAVE);
        }
        n += __popcll(__ballot(ok));
    }
    if (lane == 0) {
        const double nan = __builtin_nan("");
        frame_mean[2 * (size_t)r] = (float)(n ? sum_err / (double)n : nan);
        frame_mean[2 * (size_t)r + 1] = (float)(n ? sum_moved / (double)n : nan);
        n_valid[r] = n;
    }
}

}  // namespace

extern "C" int kpx_affine_warp_f32(const float* in, int N, int H, int W, int C, const int32_t* rows, const double* coef, int R, float* out,
                                   void* stream) {
    if (!in || !rows || !coef || !out || N < 1 || H < 1 || H > 1024 || W < 1 || W > 1024 || !(C == 1 || C == 3) || R < 1 || R > KPX_WARP_MAX_ROWS)
        return KPX_EINVAL;
    if (((((uintptr_t)in) | ((uintptr_t)out) | ((uintptr_t)rows)) & 3) || (((uintptr_t)coef) & 7)) return KPX_EINVAL;
    const bool vec = W % 4 == 0 && (((uintptr_t)out) & 15) == 0;
    hipStream_t s = kpx_stream(stream);
    if (C == 1)
        aw_launch<1>(in, H, W, rows, coef, R, out, vec, s);
    else
        aw_launch<3>(in, H, W, rows, coef, R, out, vec, s);
    return kpx_launch_status();
}

extern "C" int kpx_equivariance_scores_f32(const float* pts, const float* pts_w, const int32_t* rows, const double* fwd, int R, int K, float* out,
                                           uint8_t* valid, float* frame_mean, int32_t* n_valid, void* stream) {
    if (!pts || !pts_w || !rows || !fwd || !out || !valid || !frame_mean || !n_valid || R < 1 || R > KPX_EQUIV_MAX_ROWS || K < 1 || K > 1024)
        return KPX_EINVAL;
    if (((((uintptr_t)pts) | ((uintptr_t)pts_w) | ((uintptr_t)rows) | ((uintptr_t)out) | ((uintptr_t)frame_mean) | ((uintptr_t)n_valid)) & 3) ||
        (((uintptr_t)fwd) & 7))
        return KPX_EINVAL;
    hipLaunchKernelGGL(equivariance_scores_kernel, dim3((unsigned)((R + EQ_ROWS - 1) / EQ_ROWS)), dim3(EQ_THREADS), 0, kpx_stream(stream), pts,
                       pts_w, rows, fwd, R, K, out, valid, frame_mean, n_valid);
    return kpx_launch_status();
}
