// evaluate.py --novelty (kpx_amd/novelty.py, include/kpx.h ABI 25): the nearest training motion of every query sequence, per action class.
//
// A candidate is a window of the resident label store (csrc/augment_seq.hip reads the same buffer): 32 future frames of K points, read as the
// loader's un-augmented real_seq -- for gap >= 1 label row im_idx + gap * t, for gap == 0 the interpolated form with augment_seq's float32 add
// and halving -- and optionally its mirror image (x negated).  d2(q, w, m) = (sum over the 32 K points of ex^2 + ey^2) / (32 K) in fp64:
//
//   the sum   lane l of ONE wavefront takes the points j = l, l + 64, ... (j = (t - 1) K + k) in ascending order, s = fma(ex, ex, s) then
//             s = fma(ey, ey, s) from s = 0; the 64 lane sums meet in the xor butterfly 32, 16, ..., 1 (kpx_wave_sum_d); one division by 32 K.
//             Nothing in it depends on the window's place in the table, the query's place in the batch, Q or the grid.
//   the tile  a wavefront holds NN_WT windows x NN_QT queries in registers: per point NN_WT + NN_QT 8-byte loads feed NN_WT * NN_QT * 4 fp64
//             fmas (2 without the mirror), so the launch is bound by fp64 issue and the label rows come from L2.
//   the min   the table is read through `order`, which groups the windows by class in blocks of KPX_NEAREST_GROUP (-1 pads a class's last
//             block): a workgroup takes one block, so one class, and NN_QT queries.  It writes ONE partial (d2, code) per query into the
//             workspace; the second launch combines a class's blocks in ascending order.  A candidate is taken when its d2 is finite and
//             (d2, code) is lexicographically lower than the best so far, so ties go to the lowest code whatever the order of arrival.
//             No atomics anywhere.
#include "kpx_common.h"
#include <math.h>

enum { NW_VIDEO = 0, NW_IM_IDX, NW_GAP, NW_ACTION };
enum { NN_WT = 4, NN_QT = 8, NN_WAVES = 4, NN_TILES = 4, NN_THREADS = NN_WAVES * KPX_WAVE };
static_assert(NN_WT * NN_WAVES * NN_TILES == KPX_NEAREST_GROUP, "a workgroup takes one block of the class-grouped order");

__device__ __forceinline__ bool nn_better(double d, int c, double best_d, int best_c) { return d < best_d || (d == best_d && c < best_c); }

// frame t = 1..32 of a window, point k: real_seq[t - 1] of SequenceDataLoader.render without augmentation, as csrc/augment_seq.hip reads it.
// src, im_idx and gap are uniform over the wavefront (scalar registers); the offset inside one video's array fits 32 bits (the host's
// LabelIndex holds a video's rows * K * 2 below 2^31: a frame count is far below 2^22).
__device__ __forceinline__ float2 nn_frame(const float* __restrict__ src, int im_idx, int gap, int K, int t, int k) {
    if (gap >= 1) return *(const float2*)(src + (unsigned)((im_idx + gap * t) * K + k) * 2u);
    const unsigned o = (unsigned)((im_idx + (t >> 1)) * K + k) * 2u;
    float2 h = *(const float2*)(src + o);
    if (t & 1) {                                                 // (half[i] + half[i + 1]) / 2.0 in float32
        const float2 q = *(const float2*)(src + o + (unsigned)K * 2u);
        h.x = kpx_mul_rn(kpx_add_rn(h.x, q.x), 0.5f);
        h.y = kpx_mul_rn(kpx_add_rn(h.y, q.y), 0.5f);
    }
    return h;
}

template <bool MIRROR>
__global__ __launch_bounds__(NN_THREADS) void seq_nearest_partial_kernel(const float* __restrict__ labels, const int64_t* __restrict__ label_off,
                                                                         const int32_t* __restrict__ windows, const int32_t* __restrict__ order,
                                                                         const float* __restrict__ queries, const int32_t* __restrict__ exclude,
                                                                         int Q, int K, double* __restrict__ part_d, int32_t* __restrict__ part_c) {
    __shared__ double sh_d[NN_WAVES][NN_QT];
    __shared__ int sh_c[NN_WAVES][NN_QT];
    const int lane = threadIdx.x & (KPX_WAVE - 1), wave = threadIdx.x / KPX_WAVE;
    const int group = blockIdx.x, q0 = blockIdx.y * NN_QT;
    const int n = (KPX_SEQ_LEN - 1) * K;                         // points of a sequence, <= 8192
    const float2* qp[NN_QT];
    int excl[NN_QT], best_c[NN_QT];
    double best_d[NN_QT];
#pragma unroll
    for (int qi = 0; qi < NN_QT; ++qi) {
        const int q = min(q0 + qi, Q - 1);                       // a query past the batch repeats the last one; its result is dropped
        qp[qi] = (const float2*)queries + (size_t)q * n;
        excl[qi] = exclude ? exclude[q] : -1;
        best_d[qi] = INFINITY;
        best_c[qi] = -1;
    }
    for (int tile = 0; tile < NN_TILES; ++tile) {
        const int32_t* ord = order + (size_t)group * KPX_NEAREST_GROUP + (tile * NN_WAVES + wave) * NN_WT;
        if (ord[0] < 0) continue;                                // the pads close a block: nothing after the first one (uniform in the wave)
        const float* src[NN_WT];
        int wid[NN_WT], im_idx[NN_WT], gap[NN_WT], video[NN_WT];
#pragma unroll
        for (int wi = 0; wi < NN_WT; ++wi) {
            wid[wi] = __builtin_amdgcn_readfirstlane(ord[wi]);                                                   // the same in every lane: scalar registers
            const int32_t* row = windows + (size_t)(wid[wi] >= 0 ? wid[wi] : __builtin_amdgcn_readfirstlane(ord[0])) * KPX_NEAREST_ROW_INTS;     // a pad reads the tile's first window
            video[wi] = __builtin_amdgcn_readfirstlane(row[NW_VIDEO]);
            im_idx[wi] = __builtin_amdgcn_readfirstlane(row[NW_IM_IDX]);
            gap[wi] = __builtin_amdgcn_readfirstlane(row[NW_GAP]);
            const int64_t off = label_off[video[wi]];
            src[wi] = labels + (((int64_t)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)off));
        }
        double acc[NN_WT][NN_QT], accm[NN_WT][NN_QT];
#pragma unroll
        for (int wi = 0; wi < NN_WT; ++wi)
#pragma unroll
            for (int qi = 0; qi < NN_QT; ++qi) acc[wi][qi] = accm[wi][qi] = 0.0;
        for (int j = lane; j < n; j += KPX_WAVE) {
            const int t = j / K, k = j - t * K;
            double vx[NN_WT], vy[NN_WT];
#pragma unroll
            for (int wi = 0; wi < NN_WT; ++wi) {
                const float2 v = nn_frame(src[wi], im_idx[wi], gap[wi], K, t + 1, k);
                vx[wi] = (double)v.x;
                vy[wi] = (double)v.y;
            }
#pragma unroll
            for (int qi = 0; qi < NN_QT; ++qi) {
                const float2 qv = qp[qi][j];
                const double qx = (double)qv.x, qy = (double)qv.y;
#pragma unroll
                for (int wi = 0; wi < NN_WT; ++wi) {
                    const double ex = qx - vx[wi], ey = qy - vy[wi];
                    acc[wi][qi] = fma(ey, ey, fma(ex, ex, acc[wi][qi]));
                    if (MIRROR) {
                        const double em = qx + vx[wi];
                        accm[wi][qi] = fma(ey, ey, fma(em, em, accm[wi][qi]));
                    }
                }
            }
        }
#pragma unroll
        for (int wi = 0; wi < NN_WT; ++wi)
#pragma unroll
            for (int qi = 0; qi < NN_QT; ++qi) {
                const bool live = wid[wi] >= 0 && video[wi] != excl[qi];
                const double d = kpx_wave_sum_d(acc[wi][qi]) / (double)n;
                if (live && d < INFINITY && nn_better(d, 2 * wid[wi], best_d[qi], best_c[qi])) { best_d[qi] = d; best_c[qi] = 2 * wid[wi]; }
                if (MIRROR) {
                    const double dm = kpx_wave_sum_d(accm[wi][qi]) / (double)n;
                    if (live && dm < INFINITY && nn_better(dm, 2 * wid[wi] + 1, best_d[qi], best_c[qi])) { best_d[qi] = dm; best_c[qi] = 2 * wid[wi] + 1; }
                }
            }
    }
    if (lane == 0) {
#pragma unroll
        for (int qi = 0; qi < NN_QT; ++qi) { sh_d[wave][qi] = best_d[qi]; sh_c[wave][qi] = best_c[qi]; }
    }
    __syncthreads();
    if (threadIdx.x < NN_QT && q0 + (int)threadIdx.x < Q) {
        double d = sh_d[0][threadIdx.x];
        int c = sh_c[0][threadIdx.x];
        for (int w = 1; w < NN_WAVES; ++w)
            if (nn_better(sh_d[w][threadIdx.x], sh_c[w][threadIdx.x], d, c)) { d = sh_d[w][threadIdx.x]; c = sh_c[w][threadIdx.x]; }
        const size_t o = (size_t)group * Q + q0 + threadIdx.x;
        part_d[o] = d;
        part_c[o] = c;
    }
}

// one thread per (class, query): the class's blocks in ascending order
__global__ __launch_bounds__(256) void seq_nearest_combine_kernel(const double* __restrict__ part_d, const int32_t* __restrict__ part_c,
                                                                  const int32_t* __restrict__ group_first, int Q, int A,
                                                                  double* __restrict__ d2, int32_t* __restrict__ code) {
    const int id = blockIdx.x * 256 + threadIdx.x;               // Q * A <= 2^20
    if (id >= Q * A) return;
    const int a = id / Q, q = id - a * Q;
    double d = INFINITY;
    int c = -1;
    for (int g = group_first[a]; g < group_first[a + 1]; ++g) {
        const size_t o = (size_t)g * Q + q;
        if (nn_better(part_d[o], part_c[o], d, c)) { d = part_d[o]; c = part_c[o]; }
    }
    d2[(size_t)q * A + a] = d;
    code[(size_t)q * A + a] = c;
}

static bool nn_sizes_ok(int n_groups, int Q) { return n_groups >= 1 && n_groups <= (1 << 24) + KPX_SEQ_MAX_ACTIONS && Q >= 1 && Q <= KPX_NEAREST_MAX_QUERIES; }

extern "C" size_t kpx_seq_nearest_workspace_bytes(int n_groups, int Q) {
    if (!nn_sizes_ok(n_groups, Q)) return 0;
    return (size_t)n_groups * Q * (sizeof(double) + sizeof(int32_t));
}

extern "C" int kpx_seq_nearest_f32(const float* labels, const int64_t* label_off, const int32_t* windows, int W, const int32_t* order,
                                   const int32_t* group_first, int n_groups, const float* queries, const int32_t* exclude, int Q, int n_points,
                                   int n_action, int mirror, void* workspace, size_t workspace_bytes, double* d2, int32_t* code, void* stream) {
    if (!labels || !label_off || !windows || !order || !group_first || !queries || !workspace || !d2 || !code) return KPX_EINVAL;
    if (W < 1 || W > KPX_NEAREST_MAX_WINDOWS || !nn_sizes_ok(n_groups, Q) || n_points < 1 || n_points > KPX_SEQ_MAX_POINTS || n_action < 1 ||
        n_action > KPX_SEQ_MAX_ACTIONS || (mirror != 0 && mirror != 1))
        return KPX_EINVAL;
    if (n_groups > (W + KPX_NEAREST_GROUP - 1) / KPX_NEAREST_GROUP + n_action) return KPX_EINVAL;      // more blocks than any grouping of W windows has
    if (workspace_bytes < kpx_seq_nearest_workspace_bytes(n_groups, Q)) return KPX_EINVAL;
    if (((((uintptr_t)labels) | ((uintptr_t)label_off) | ((uintptr_t)queries) | ((uintptr_t)workspace) | ((uintptr_t)d2)) & 7) ||
        ((((uintptr_t)windows) | ((uintptr_t)order) | ((uintptr_t)group_first) | ((uintptr_t)exclude) | ((uintptr_t)code)) & 3))
        return KPX_EINVAL;
    double* part_d = (double*)workspace;
    int32_t* part_c = (int32_t*)(part_d + (size_t)n_groups * Q);
    hipStream_t s = kpx_stream(stream);
    const dim3 grid(n_groups, (Q + NN_QT - 1) / NN_QT);
    if (mirror)
        hipLaunchKernelGGL(seq_nearest_partial_kernel<true>, grid, dim3(NN_THREADS), 0, s, labels, label_off, windows, order, queries, exclude, Q,
                           n_points, part_d, part_c);
    else
        hipLaunchKernelGGL(seq_nearest_partial_kernel<false>, grid, dim3(NN_THREADS), 0, s, labels, label_off, windows, order, queries, exclude, Q,
                           n_points, part_d, part_c);
    int rc = kpx_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(seq_nearest_combine_kernel, dim3((Q * n_action + 255) / 256), dim3(256), 0, s, part_d, part_c, group_first, Q, n_action, d2,
                       code);
    return kpx_launch_status();
}
