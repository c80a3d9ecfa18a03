// Key-point action classifier: softmax cross-entropy (forward / backward) and the per-row scores evaluate.py --action-accuracy reads.
//   loss   : reduce_mean(tf.nn.softmax_cross_entropy_with_logits(labels, logits))
//   scores : arg max, rank of the target class, log-probability of the target class, confusion counts
// Rows are short (A = 9 classes in practice, <= 1024): one wavefront works on one row, lane l on the classes l, l + 64, ..., and the row's
// maximum / sums come from a 64-lane butterfly.  fp64 arithmetic in a fixed order, rounded to fp32 once; no float atomics.
#include "kpx_common.h"
#include <math.h>

namespace {

constexpr int CX_MAX_CLASSES = 1024;
constexpr int CX_MAX_ROWS = 1 << 20;
constexpr int CX_FWD_THREADS = 1024;                 // the forward's single workgroup: 16 wavefronts
constexpr int CX_FWD_CHUNK = 1024;                   // rows whose losses wait in LDS for the ordered sum
constexpr int CX_ROW_THREADS = 256;                  // scores: 4 wavefronts = 4 rows per workgroup and pass
constexpr int CX_MAX_BLOCKS = 2048;

__device__ __forceinline__ int cx_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// max_j + log(sum_j exp(x_j - max_j)) of one row, the same value in every lane of the wavefront
__device__ __forceinline__ double cx_row_lse(const float* __restrict__ x, int A, int lane) {
#pragma clang fp contract(off)
    float m = -INFINITY;
    for (int j = lane; j < A; j += KPX_WAVE) m = fmaxf(m, x[j]);
    m = kpx_wave_max(m);
    double s = 0.0;
    for (int j = lane; j < A; j += KPX_WAVE) s += exp((double)x[j] - (double)m);
    s = kpx_wave_sum_d(s);
    return (double)m + log(s);
}

// One workgroup: wavefront w takes the rows w, w + 16, ... of a chunk, the row losses wait in LDS and thread 0 adds them in ascending row
// order, so the mean does not depend on how the rows were spread over the wavefronts.
__global__ __launch_bounds__(CX_FWD_THREADS) void softmax_xent_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                                          int B, int A, float* __restrict__ loss_out,
                                                                          float* __restrict__ lse_out) {
#pragma clang fp contract(off)
    __shared__ double row_loss[CX_FWD_CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double total = 0.0;                                                   // thread 0 only
    for (int base = 0; base < B; base += CX_FWD_CHUNK) {
        const int rows = B - base < CX_FWD_CHUNK ? B - base : CX_FWD_CHUNK;
        for (int r = wave; r < rows; r += CX_FWD_THREADS / KPX_WAVE) {
            const float* x = logits + (size_t)(base + r) * A;
            const float* y = labels + (size_t)(base + r) * A;
            const double lse = cx_row_lse(x, A, lane);
            double l = 0.0;
            for (int j = lane; j < A; j += KPX_WAVE) l += (double)y[j] * ((double)x[j] - lse);
            l = kpx_wave_sum_d(l);
            if (lane == 0) {
                row_loss[r] = -l;
                lse_out[base + r] = (float)lse;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int r = 0; r < rows; ++r) total += row_loss[r];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_out = (float)(total / (double)B);
}

// dlogits = g / B * (exp(x - lse) - y): no reduction, one element per lane and pass
__global__ __launch_bounds__(256) void softmax_xent_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                               const float* __restrict__ lse, int B, int A, const float* gdev, float ghost,
                                                               float* __restrict__ dlogits) {
#pragma clang fp contract(off)
    const float g = ghost * (gdev ? *gdev : 1.0f);
    const double scale = (double)g / (double)B;
    const size_t n = (size_t)B * A;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t row = i / (size_t)A;
        const double p = exp((double)logits[i] - (double)lse[row]);
        dlogits[i] = (float)(scale * (p - (double)labels[i]));
    }
}

__global__ __launch_bounds__(CX_ROW_THREADS) void class_scores_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target,
                                                                      int M, int A, int32_t* __restrict__ pred, int32_t* __restrict__ rank,
                                                                      float* __restrict__ logp, int32_t* __restrict__ confusion) {
    const int lane = threadIdx.x & 63;
    const int waves = CX_ROW_THREADS / KPX_WAVE;
    for (int row = blockIdx.x * waves + (threadIdx.x >> 6); row < M; row += gridDim.x * waves) {   // wavefront-uniform
        const float* x = logits + (size_t)row * A;
        const int t = target[row];
        const bool t_ok = t >= 0 && t < A;                                // the wrapper refuses such a target; never read outside the row
        int bad = 0, best_j = CX_MAX_CLASSES;
        float best = -INFINITY;
        for (int j = lane; j < A; j += KPX_WAVE) {
            const float v = x[j];
            bad |= !isfinite(v);
            if (v > best || best_j == CX_MAX_CLASSES) { best = v; best_j = j; }    // ascending j: the first of equal values stays
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oj = __shfl_xor(best_j, o, 64);
            if (oj != CX_MAX_CLASSES && (best_j == CX_MAX_CLASSES || ov > best || (ov == best && oj < best_j))) { best = ov; best_j = oj; }
        }
        bad = cx_wave_sum_i(bad);
        if (bad || !t_ok) {
            if (lane == 0) {
                pred[row] = bad ? -1 : best_j;
                rank[row] = A;
                logp[row] = NAN;
            }
            continue;
        }
        const float xt = x[t];
        int above = 0;
        for (int j = lane; j < A; j += KPX_WAVE) above += (j != t && x[j] >= xt) ? 1 : 0;
        above = cx_wave_sum_i(above);
        const double lse = cx_row_lse(x, A, lane);
        if (lane == 0) {
            pred[row] = best_j;
            rank[row] = 1 + above;
            logp[row] = (float)((double)xt - lse);
            if (confusion) atomicAdd(&confusion[(size_t)t * A + best_j], 1);       // integer: exact whatever the order
        }
    }
}

inline bool cx_misaligned(const void* p) { return (((uintptr_t)p) & 3) != 0; }

}  // namespace

extern "C" int kpx_softmax_xent_fwd_f32(const float* logits, const float* labels, int B, int A, float* loss_out, float* lse_out, void* stream) {
    if (!logits || !labels || !loss_out || !lse_out || B < 1 || B > CX_MAX_ROWS || A < 1 || A > CX_MAX_CLASSES || cx_misaligned(logits) ||
        cx_misaligned(labels) || cx_misaligned(loss_out) || cx_misaligned(lse_out))
        return KPX_EINVAL;
    hipLaunchKernelGGL(softmax_xent_fwd_kernel, dim3(1), dim3(CX_FWD_THREADS), 0, kpx_stream(stream), logits, labels, B, A, loss_out, lse_out);
    return kpx_launch_status();
}

extern "C" int kpx_softmax_xent_bwd_f32(const float* logits, const float* labels, const float* lse, int B, int A, const float* gscale_dev,
                                        float gscale_host, float* dlogits, void* stream) {
    if (!logits || !labels || !lse || !dlogits || B < 1 || B > CX_MAX_ROWS || A < 1 || A > CX_MAX_CLASSES || cx_misaligned(logits) ||
        cx_misaligned(labels) || cx_misaligned(lse) || cx_misaligned(gscale_dev) || cx_misaligned(dlogits))
        return KPX_EINVAL;
    size_t nb = ((size_t)B * A + 255) / 256;
    if (nb > CX_MAX_BLOCKS) nb = CX_MAX_BLOCKS;
    hipLaunchKernelGGL(softmax_xent_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, kpx_stream(stream), logits, labels, lse, B, A, gscale_dev,
                       gscale_host, dlogits);
    return kpx_launch_status();
}

extern "C" int kpx_class_scores_f32(const float* logits, const int32_t* target, int M, int A, int32_t* pred, int32_t* rank, float* logp,
                                    int32_t* confusion, void* stream) {
    if (!logits || !target || !pred || !rank || !logp || M < 1 || M > CX_MAX_ROWS || A < 1 || A > CX_MAX_CLASSES || cx_misaligned(logits) ||
        cx_misaligned(target) || cx_misaligned(pred) || cx_misaligned(rank) || cx_misaligned(logp) || cx_misaligned(confusion))
        return KPX_EINVAL;
    const int waves = CX_ROW_THREADS / KPX_WAVE;
    int nb = (M + waves - 1) / waves;
    if (nb > CX_MAX_BLOCKS) nb = CX_MAX_BLOCKS;
    hipLaunchKernelGGL(class_scores_kernel, dim3(nb), dim3(CX_ROW_THREADS), 0, kpx_stream(stream), logits, target, M, A, pred, rank, logp,
                       confusion);
    return kpx_launch_status();
}
