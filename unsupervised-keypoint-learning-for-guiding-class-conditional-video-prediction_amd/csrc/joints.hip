// Landmark regression from the detector's key points to annotated joints (make_pseudo_labels.py --joints, kpx_amd/joints.py; DESIGN.md
// section 2): a linear map from the K discovered points of a frame to its J annotated joints, fitted on the train split and scored on both.
// Throughout phi_f = (x_0, y_0, ..., x_{K-1}, y_{K-1}, 1) is the feature row of frame f (the fp32 key points widened to fp64, which is exact)
// and D = 2K + 1.  Everything is fp64; where a product and a sum are each rounded once the code carries `fp contract(off)`.
//
//   kpx_joint_targets_f32      annotations in the original frame's pixels -> the key points' normalised crop coordinates, the mask of the
//                              joints that can be scored and the frame's PCK normaliser.  One lane per (frame, joint); the lane of joint 0
//                              also writes the frame's normaliser.
//   kpx_joint_moments_add_f64  the masked normal equations per joint, in place: kpx_moments_add_f64's sibling (frechet.hip).  One workgroup
//                              per joint and 32 x 32 tile of G[j], 256 lanes as 16 x 16, lane (ty, tx) owns the elements (i0 + ty + 16 r,
//                              j0 + tx + 16 c): it reads their stored values, walks f in ascending order with one fma per frame that counts
//                              and writes them back.  The tiles of the first tile column also own Bm[j][i0 .. i0 + 32) (lanes tx < 2), the
//                              first tile owns n[j].  The two strips of phi a tile needs are staged in LDS 32 frames at a time, with the
//                              frames' targets and a flag "all 2K coordinates finite" that eight lanes per frame work out.  fma(a, b, acc)
//                              and fma(b, a, acc) are the same bits, so G stays bitwise symmetric; nothing but the stored value and the
//                              frames walked enters an element, so any split of the frames into consecutive calls gives the same bits.
//   kpx_joint_scores_f32       the regressor applied: one workgroup per joint, W[j] in LDS, a lane per frame of a run of 256.  The per-call
//                              sums are folded by the first wavefront lane by lane in ascending f (every lane holds the same chain), so
//                              their order does not depend on the launch.  The counts are ballots.
//
// No atomics, plain vector stores only.
#include "kpx_common.h"

namespace {

constexpr int JT_THREADS = 256;
constexpr int JM_THREADS = 256, JM_TILE = 32, JM_ROWS = 32, JM_E = JM_TILE / 16, JM_SCAN = JM_THREADS / JM_ROWS;
constexpr int JS_THREADS = 256, JS_MAX_D = 2 * KPX_JOINT_MAX_POINTS + 1;

__device__ __forceinline__ bool jt_finite(double v) { return fabs(v) < __builtin_inf(); }   // false for NaN

__global__ __launch_bounds__(JT_THREADS) void joint_targets_kernel(const float* __restrict__ xy, const uint8_t* __restrict__ vis,
                                                                   const float* __restrict__ bbox, const double* __restrict__ map, int F, int J,
                                                                   float* __restrict__ target, uint8_t* __restrict__ mask,
                                                                   float* __restrict__ norm) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * JT_THREADS + threadIdx.x;    // F * J <= 2^25
    if (i >= (size_t)F * J) return;
    const double ax = map[0], bx = map[1], ay = map[2], by = map[3];
    const double x = (double)xy[2 * i], y = (double)xy[2 * i + 1];
    const double tx = ax * x + bx, ty = ay * y + by;
    target[2 * i] = (float)tx;
    target[2 * i + 1] = (float)ty;
    mask[i] = vis[i] != 0 && jt_finite(x) && jt_finite(y) && tx >= -1.0 && tx <= 1.0 && ty >= -1.0 && ty <= 1.0 ? 1 : 0;
    const size_t f = i / J;
    if (i - f * J == 0) {
        const double x0 = (double)bbox[4 * f], y0 = (double)bbox[4 * f + 1], x1 = (double)bbox[4 * f + 2], y1 = (double)bbox[4 * f + 3];
        const bool ok = jt_finite(x0) && jt_finite(y0) && jt_finite(x1) && jt_finite(y1) && x1 > x0 && y1 > y0;
        const double w = fabs(ax) * (x1 - x0), h = fabs(ay) * (y1 - y0);
        norm[f] = ok ? (float)(w > h ? w : h) : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(JM_THREADS) void joint_moments_kernel(const float* __restrict__ pts, const float* __restrict__ target,
                                                                   const uint8_t* __restrict__ mask, int F, int K, int J,
                                                                   double* __restrict__ G, double* __restrict__ Bm, int64_t* __restrict__ n) {
    __shared__ double sa[JM_ROWS][JM_TILE], sb[JM_ROWS][JM_TILE], st[JM_ROWS][2];
    __shared__ uint8_t sfin[JM_ROWS][JM_SCAN];
    __shared__ int suse[JM_ROWS];
    const int D = 2 * K + 1, K2 = 2 * K;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int j = blockIdx.z, i0 = blockIdx.y * JM_TILE, j0 = blockIdx.x * JM_TILE;
    const bool bown = blockIdx.x == 0 && tx < 2;                       // this lane also owns Bm[j][i0 + ty + 16 r][tx]
    const bool nown = blockIdx.x == 0 && blockIdx.y == 0 && tid == 0;  // and this one n[j]
    double* Gj = G + (size_t)j * D * D;
    double* Bj = Bm + (size_t)j * D * 2;
    double acc[JM_E][JM_E], bacc[JM_E];
#pragma unroll
    for (int r = 0; r < JM_E; ++r) {
        const int i = i0 + ty + 16 * r;
#pragma unroll
        for (int c = 0; c < JM_E; ++c) {
            const int jj = j0 + tx + 16 * c;
            acc[r][c] = i < D && jj < D ? Gj[(size_t)i * D + jj] : 0.0;
        }
        bacc[r] = bown && i < D ? Bj[2 * i + tx] : 0.0;
    }
    int64_t cnt = nown ? n[j] : 0;

    for (int m0 = 0; m0 < F; m0 += JM_ROWS) {
        const int rows = min(JM_ROWS, F - m0);
        // the two strips of phi: column c < 2K is a coordinate, column 2K the constant 1; columns past D and frames past F stage 0 (those
        // columns' lanes write nothing, those frames are never walked)
#pragma unroll
        for (int k = 0; k < JM_ROWS * JM_TILE / JM_THREADS; ++k) {
            const int e = tid + k * JM_THREADS, mm = e / JM_TILE, col = e - mm * JM_TILE;
            const bool in = mm < rows;
            const float* row = pts + (size_t)(in ? m0 + mm : 0) * K2;
            const int ca = i0 + col, cb = j0 + col;
            sa[mm][col] = !in ? 0.0 : ca < K2 ? (double)row[ca] : ca == K2 ? 1.0 : 0.0;
            sb[mm][col] = !in ? 0.0 : cb < K2 ? (double)row[cb] : cb == K2 ? 1.0 : 0.0;
        }
        {                                                              // eight lanes per frame: are its 2K coordinates finite
            const int mm = tid / JM_SCAN, sub = tid - mm * JM_SCAN;
            bool ok = mm < rows;
            if (ok) {
                const float* row = pts + (size_t)(m0 + mm) * K2;
                for (int d = sub; d < K2; d += JM_SCAN) ok = ok && jt_finite((double)row[d]);
            }
            sfin[mm][sub] = ok ? 1 : 0;
        }
        if (tid < 2 * JM_ROWS) {
            const int mm = tid >> 1, c = tid & 1;
            st[mm][c] = mm < rows ? (double)target[((size_t)(m0 + mm) * J + j) * 2 + c] : 0.0;
        }
        __syncthreads();
        if (tid < JM_ROWS) {
            bool use = tid < rows && mask[(size_t)(m0 + tid) * J + j] != 0;
#pragma unroll
            for (int s = 0; s < JM_SCAN; ++s) use = use && sfin[tid][s] != 0;
            suse[tid] = use ? 1 : 0;
        }
        __syncthreads();
        for (int mm = 0; mm < rows; ++mm) {
            if (!suse[mm]) continue;                                   // the same for every lane of the workgroup
            double a[JM_E], b[JM_E];
#pragma unroll
            for (int r = 0; r < JM_E; ++r) a[r] = sa[mm][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < JM_E; ++c) b[c] = sb[mm][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < JM_E; ++r)
#pragma unroll
                for (int c = 0; c < JM_E; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
            if (bown) {
                const double t = st[mm][tx];
#pragma unroll
                for (int r = 0; r < JM_E; ++r) bacc[r] = fma(a[r], t, bacc[r]);
            }
            if (nown) ++cnt;
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < JM_E; ++r) {
        const int i = i0 + ty + 16 * r;
#pragma unroll
        for (int c = 0; c < JM_E; ++c) {
            const int jj = j0 + tx + 16 * c;
            if (i < D && jj < D) Gj[(size_t)i * D + jj] = acc[r][c];
        }
        if (bown && i < D) Bj[2 * i + tx] = bacc[r];
    }
    if (nown) n[j] = cnt;
}

__global__ __launch_bounds__(JS_THREADS) void joint_scores_kernel(const float* __restrict__ pts, const float* __restrict__ target,
                                                                  const uint8_t* __restrict__ mask, const float* __restrict__ norm,
                                                                  const double* __restrict__ W, const double* __restrict__ alpha, int F, int K,
                                                                  int J, int A, float* __restrict__ pred, float* __restrict__ err,
                                                                  uint8_t* __restrict__ hits, double* __restrict__ sum_err,
                                                                  int64_t* __restrict__ count, int64_t* __restrict__ pck_count,
                                                                  int64_t* __restrict__ hit_count) {
#pragma clang fp contract(off)
    __shared__ double sw[JS_MAX_D * 2], sal[KPX_JOINT_MAX_ALPHAS], serr[JS_THREADS];
    __shared__ unsigned sflag[JS_THREADS];
    const int D = 2 * K + 1, K2 = 2 * K, tid = threadIdx.x, lane = tid & (KPX_WAVE - 1), j = blockIdx.x;
    for (int i = tid; i < 2 * D; i += JS_THREADS) sw[i] = W[(size_t)j * D * 2 + i];
    if (tid < A) sal[tid] = alpha[tid];
    __syncthreads();
    double sum = 0.0;
    int64_t cnt = 0, pcnt = 0, hcnt[KPX_JOINT_MAX_ALPHAS];
#pragma unroll
    for (int a = 0; a < KPX_JOINT_MAX_ALPHAS; ++a) hcnt[a] = 0;
    for (int f0 = 0; f0 < F; f0 += JS_THREADS) {
        const int f = f0 + tid;
        double e = 0.0;
        unsigned flag = 0;                                             // bit 0 valid, bit 1 valid for PCK, bits 2 .. 9 the hits
        if (f < F) {
            const float* p = pts + (size_t)f * K2;
            double px = 0.0, py = 0.0;
            bool fin = true;
            for (int d = 0; d < K2; ++d) {                             // ascending d, every product and sum rounded once
                const double v = (double)p[d];
                fin = fin && jt_finite(v);
                px = px + v * sw[2 * d];
                py = py + v * sw[2 * d + 1];
            }
            px = px + sw[2 * K2];                                      // the constant feature: 1 * w is w
            py = py + sw[2 * K2 + 1];
            const size_t i = (size_t)f * J + j;
            const double dx = px - (double)target[2 * i], dy = py - (double)target[2 * i + 1];
            const double er = sqrt(dx * dx + dy * dy);
            pred[2 * i] = (float)px;
            pred[2 * i + 1] = (float)py;
            err[i] = (float)er;
            const bool valid = mask[i] != 0 && fin;
            const double nf = (double)norm[f];
            const bool pck = valid && jt_finite(nf);
            unsigned h = 0;
            if (pck)
                for (int a = 0; a < A; ++a)
                    if (er <= sal[a] * nf) h |= 1u << a;
            hits[i] = (uint8_t)h;
            if (valid) {
                e = er;
                flag = 1u | (pck ? 2u : 0u) | (h << 2);
            }
        }
        serr[tid] = e;
        sflag[tid] = flag;
        __syncthreads();
        if (tid < KPX_WAVE) {                                          // the first wavefront folds the run in ascending f
            for (int c = 0; c < JS_THREADS / KPX_WAVE && f0 + c * KPX_WAVE < F; ++c) {
                const double ev = serr[c * KPX_WAVE + lane];
                const unsigned fl = sflag[c * KPX_WAVE + lane];
                for (int l = 0; l < KPX_WAVE; ++l) sum += __shfl(ev, l, KPX_WAVE);   // an entry that is not valid adds +0 to a sum >= +0
                cnt += __popcll(__ballot(fl & 1u));
                pcnt += __popcll(__ballot(fl & 2u));
#pragma unroll
                for (int a = 0; a < KPX_JOINT_MAX_ALPHAS; ++a)         // bits past A are never set
                    hcnt[a] += __popcll(__ballot((fl >> (2 + a)) & 1u));
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        sum_err[j] = sum;
        count[j] = cnt;
        pck_count[j] = pcnt;
    }
    if (tid < A) {
        int64_t v = 0;
#pragma unroll
        for (int a = 0; a < KPX_JOINT_MAX_ALPHAS; ++a)
            if (a == tid) v = hcnt[a];
        hit_count[(size_t)j * A + tid] = v;
    }
}

bool jt_sizes_ok(int F, int K, int J) {
    return F >= 1 && F <= KPX_JOINT_MAX_FRAMES && K >= 1 && K <= KPX_JOINT_MAX_POINTS && J >= 1 && J <= KPX_JOINT_MAX_JOINTS;
}

}  // namespace

extern "C" int kpx_joint_targets_f32(const float* xy, const uint8_t* vis, const float* bbox, const double* map, int F, int J, float* target,
                                     uint8_t* mask, float* norm, void* stream) {
    if (!xy || !vis || !bbox || !map || !target || !mask || !norm || !jt_sizes_ok(F, 1, J)) return KPX_EINVAL;
    if (((((uintptr_t)xy) | ((uintptr_t)bbox) | ((uintptr_t)target) | ((uintptr_t)norm)) & 3) || (((uintptr_t)map) & 7)) return KPX_EINVAL;
    const size_t blocks = ((size_t)F * J + JT_THREADS - 1) / JT_THREADS;
    hipLaunchKernelGGL(joint_targets_kernel, dim3((unsigned)blocks), dim3(JT_THREADS), 0, kpx_stream(stream), xy, vis, bbox, map, F, J, target,
                       mask, norm);
    return kpx_launch_status();
}

extern "C" int kpx_joint_moments_add_f64(const float* pts, const float* target, const uint8_t* mask, int F, int K, int J, double* G, double* Bm,
                                         int64_t* n, void* stream) {
    if (!pts || !target || !mask || !G || !Bm || !n || !jt_sizes_ok(F, K, J)) return KPX_EINVAL;
    if (((((uintptr_t)pts) | ((uintptr_t)target)) & 3) || ((((uintptr_t)G) | ((uintptr_t)Bm) | ((uintptr_t)n)) & 7)) return KPX_EINVAL;
    const int t = (2 * K + 1 + JM_TILE - 1) / JM_TILE;
    hipLaunchKernelGGL(joint_moments_kernel, dim3(t, t, J), dim3(JM_THREADS), 0, kpx_stream(stream), pts, target, mask, F, K, J, G, Bm,
                       n);
    return kpx_launch_status();
}

extern "C" int kpx_joint_scores_f32(const float* pts, const float* target, const uint8_t* mask, const float* norm, const double* W,
                                    const double* alpha, int F, int K, int J, int A, float* pred, float* err, uint8_t* hits, double* sum_err,
                                    int64_t* count, int64_t* pck_count, int64_t* hit_count, void* stream) {
    if (!pts || !target || !mask || !norm || !W || !alpha || !pred || !err || !hits || !sum_err || !count || !pck_count || !hit_count ||
        !jt_sizes_ok(F, K, J) || A < 1 || A > KPX_JOINT_MAX_ALPHAS)
        return KPX_EINVAL;
    if (((((uintptr_t)pts) | ((uintptr_t)target) | ((uintptr_t)norm) | ((uintptr_t)pred) | ((uintptr_t)err)) & 3) ||
        ((((uintptr_t)W) | ((uintptr_t)alpha) | ((uintptr_t)sum_err) | ((uintptr_t)count) | ((uintptr_t)pck_count) | ((uintptr_t)hit_count)) & 7))
        return KPX_EINVAL;
    hipLaunchKernelGGL(joint_scores_kernel, dim3(J), dim3(JS_THREADS), 0, kpx_stream(stream), pts, target, mask, norm, W, alpha, F, K, J, A, pred,
                       err, hits, sum_err, count, pck_count, hit_count);
    return kpx_launch_status();
}
