// Fréchet distance in VGG19 feature space (evaluate.py --frechet, DESIGN.md sections 2 and 4.4): the two device passes.
//
// kpx_feature_pool_f64: the mean over the H * W positions of one layer's features (fp32 NHWC) per frame and channel, in fp64.  A frame is cut
// into S slabs of positions, S a function of (H, W, C) alone.  One workgroup per (slab, frame): R = 256 / (C / 4) rows of lanes, lane (r, j)
// owns the four channels 4j .. 4j + 3 and walks the positions p0 + r, p0 + r + R, ... of the slab with 16-byte loads (the R * C / 4 active
// lanes read one contiguous run per pass); every value is converted to fp64 before its first addition.  The R partials of a channel are
// folded through LDS in ascending r and written to `work`; a second launch folds a frame's slabs in ascending order and divides by H * W.
// No atomics: frame n's row depends on frame n alone, whatever N, its position in the batch or the run.
//
// kpx_moments_add_f64: sum += column sums and outer += X^T X of fp64 rows X [M, D], in place.  One workgroup per T x T tile of `outer`
// (T = 32 up to D = 128, else 64), 256 lanes as 16 x 16, lane (ty, tx) owns the elements (i0 + ty + 16 r, j0 + tx + 16 c): it reads their old
// values, walks m in ascending order with one fma per row and writes them back.  The two column strips of X that a tile needs are staged in
// LDS 32 rows at a time, the next 32 fetched into registers meanwhile.  fma(a, b, acc) and fma(b, a, acc) are the same bits, so accumulators
// that start symmetric stay bitwise symmetric.
// The tiles of the first tile row also own sum[j0 .. j0 + T).
#include "kpx_common.h"

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_SLAB_BYTES = 65536;                                   // per workgroup: what feature_pair_kernel reads of its two sides
constexpr int PL_MAX_SLABS = 128;

int pl_slabs(int H, int W, int C) {
    const long long bytes = (long long)H * W * C * 4;
    const long long s = (bytes + PL_SLAB_BYTES - 1) / PL_SLAB_BYTES;
    return (int)(s > PL_MAX_SLABS ? PL_MAX_SLABS : s);                // >= 1; never more slabs than positions (C * 4 <= 2048 < a slab)
}

__global__ __launch_bounds__(PL_THREADS) void feature_pool_kernel(const float* __restrict__ f, int N, int P, int C4, int S,
                                                                   double* __restrict__ work) {
    __shared__ double red[PL_THREADS][4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int R = PL_THREADS / C4;                                     // C4 <= 128: at least two rows of lanes
    const int r = tid / C4, j = tid - r * C4;
    const bool active = r < R;
    const int p0 = (int)((long long)P * s / S), p1 = (int)((long long)P * (s + 1) / S);
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const f32x4* fn = reinterpret_cast<const f32x4*>(f) + (size_t)n * P * C4;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (active) {
#pragma unroll 8
            for (int p = p0 + r; p < p1; p += R) {
                const f32x4 v = fn[(size_t)p * C4 + j];
                a0 += (double)v[0];
                a1 += (double)v[1];
                a2 += (double)v[2];
                a3 += (double)v[3];
            }
        }
        red[tid][0] = a0; red[tid][1] = a1; red[tid][2] = a2; red[tid][3] = a3;
        __syncthreads();
        if (tid < C4) {                                                // row 0 folds the rows of its column in ascending r
            for (int i = 1; i < R; ++i) {
                const double* o = red[i * C4 + tid];
                a0 += o[0]; a1 += o[1]; a2 += o[2]; a3 += o[3];
            }
            double* w = work + ((size_t)n * S + s) * (size_t)(4 * C4) + 4 * tid;
            w[0] = a0; w[1] = a1; w[2] = a2; w[3] = a3;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PL_THREADS) void feature_pool_finalize_kernel(const double* __restrict__ work, size_t NC, int C, int S, double npos,
                                                                            double* __restrict__ pooled) {
    const size_t idx = (size_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (idx >= NC) return;
    const size_t n = idx / C, c = idx - n * C;
    const double* w = work + n * S * C + c;
    double a = 0.0;
    int i = 0;
    for (; i + 8 <= S; i += 8) {                                       // eight loads in flight, added in ascending order
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w[(size_t)(i + k) * C];
#pragma unroll
        for (int k = 0; k < 8; ++k) a += v[k];
    }
    for (; i < S; ++i) a += w[(size_t)i * C];
    pooled[idx] = a / npos;
}

constexpr int MA_THREADS = 256;
constexpr int MA_ROWS = 32;                                            // rows of X staged per pass

template <int T>
__global__ __launch_bounds__(MA_THREADS) void moments_add_kernel(const double* __restrict__ x, int M, int D, double* __restrict__ sum,
                                                                  double* __restrict__ outer) {
    constexpr int E = T / 16;                                          // elements per lane and direction
    __shared__ double sa[MA_ROWS][T], sb[MA_ROWS][T];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
    const bool sums = blockIdx.y == 0 && ty == 0;                      // this lane also owns sum[j0 + tx + 16 c]
    double acc[E][E], sacc[E];
#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
        for (int c = 0; c < E; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            acc[r][c] = i < D && j < D ? outer[(size_t)i * D + j] : 0.0;
        }
#pragma unroll
    for (int c = 0; c < E; ++c) sacc[c] = sums && j0 + tx + 16 * c < D ? sum[j0 + tx + 16 * c] : 0.0;

    // The staged rows of the next pass are fetched into registers before the current pass is computed, so the loads' latency hides behind
    // the fmas; columns past D and rows past M stage 0 (those columns' lanes write nothing, those rows are never walked).
    constexpr int NS = MA_ROWS * T / MA_THREADS;                       // staged elements per lane and strip
    double pa[NS], pb[NS];
    auto fetch = [&](int m0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int e = tid + k * MA_THREADS, mm = e / T, col = e - mm * T;
            const bool in = m0 + mm < M;
            const double* row = x + (size_t)(in ? m0 + mm : 0) * D;
            pa[k] = in && i0 + col < D ? row[i0 + col] : 0.0;
            pb[k] = in && j0 + col < D ? row[j0 + col] : 0.0;
        }
    };
    fetch(0);
    for (int m0 = 0; m0 < M; m0 += MA_ROWS) {
        const int rows = min(MA_ROWS, M - m0);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int e = tid + k * MA_THREADS, mm = e / T, col = e - mm * T;
            sa[mm][col] = pa[k];
            sb[mm][col] = pb[k];
        }
        __syncthreads();
        if (m0 + MA_ROWS < M) fetch(m0 + MA_ROWS);
        for (int mm = 0; mm < rows; ++mm) {
            double a[E], b[E];
#pragma unroll
            for (int r = 0; r < E; ++r) a[r] = sa[mm][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < E; ++c) b[c] = sb[mm][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < E; ++r)
#pragma unroll
                for (int c = 0; c < E; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
            if (sums) {
#pragma unroll
                for (int c = 0; c < E; ++c) sacc[c] += b[c];
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < E; ++r)
#pragma unroll
        for (int c = 0; c < E; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < D && j < D) outer[(size_t)i * D + j] = acc[r][c];
        }
    if (sums) {
#pragma unroll
        for (int c = 0; c < E; ++c)
            if (j0 + tx + 16 * c < D) sum[j0 + tx + 16 * c] = sacc[c];
    }
}

bool pl_shape_ok(int N, int H, int W, int C) { return N >= 1 && H >= 1 && H <= 1024 && W >= 1 && W <= 1024 && C >= 4 && C <= 512 && C % 4 == 0; }

}  // namespace

extern "C" size_t kpx_feature_pool_workspace_bytes(int N, int H, int W, int C) {
    if (!pl_shape_ok(N, H, W, C)) return 0;
    return (size_t)N * pl_slabs(H, W, C) * C * sizeof(double);
}

extern "C" int kpx_feature_pool_f64(const float* f, int N, int H, int W, int C, double* work, double* pooled, void* stream) {
    if (!f || !work || !pooled || !pl_shape_ok(N, H, W, C) || (((uintptr_t)f) & 15) || ((((uintptr_t)work) | ((uintptr_t)pooled)) & 7))
        return KPX_EINVAL;
    const int P = H * W, C4 = C / 4, S = pl_slabs(H, W, C);
    const size_t NC = (size_t)N * C, blocks = (NC + PL_THREADS - 1) / PL_THREADS;
    if (blocks > 0x7fffffffULL) return KPX_EINVAL;
    hipStream_t s = kpx_stream(stream);
    hipLaunchKernelGGL(feature_pool_kernel, dim3(S, N > 65535 ? 65535 : N), dim3(PL_THREADS), 0, s, f, N, P, C4, S, work);
    int rc = kpx_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(feature_pool_finalize_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, s, (const double*)work, NC, C, S, (double)P,
                       pooled);
    return kpx_launch_status();
}

extern "C" int kpx_moments_add_f64(const double* x, int M, int D, double* sum, double* outer, void* stream) {
    if (!x || !sum || !outer || M < 1 || M > (1 << 20) || D < 1 || D > 1024 || ((((uintptr_t)x) | ((uintptr_t)sum) | ((uintptr_t)outer)) & 7))
        return KPX_EINVAL;
    hipStream_t s = kpx_stream(stream);
    if (D <= 128) {
        const int t = (D + 31) / 32;
        hipLaunchKernelGGL(moments_add_kernel<32>, dim3(t, t), dim3(MA_THREADS), 0, s, x, M, D, sum, outer);
    } else {
        const int t = (D + 63) / 64;
        hipLaunchKernelGGL(moments_add_kernel<64>, dim3(t, t), dim3(MA_THREADS), 0, s, x, M, D, sum, outer);
    }
    return kpx_launch_status();
}
