// evaluate.py --prdc (kpx_amd/prdc.py, include/kpx.h): the k nearest rows of a reference set for every query row, exact in fp64 -- the
// general form of csrc/novelty.hip's search: rows of any width, the k smallest instead of the minimum, one skipped reference per query,
// per-row groups and the count of references whose ball holds the query.  d2(j, i) = sum_d (q[j,d] - r[i,d])^2 in fp64:
//
//   the sum   lane l of ONE wavefront takes d = l, l + 64, ... in ascending order, e = q - r (one rounding), s = fma(e, e, s) from s = 0; the
//             64 lane sums meet in the xor butterfly 32, 16, ..., 1 (kpx_wave_sum_d).  No division.  Nothing in it depends on the rows'
//             places, M, N or the grid: the order is a function of D alone.
//   the tile  a wavefront holds SN_RT refs x SN_QT queries in registers: per d SN_RT + SN_QT 8-byte loads feed SN_RT * SN_QT subtractions and
//             fmas.  A workgroup takes one block of KPX_SET_BLOCK refs (SN_TILES tiles of each of its SN_WAVES wavefronts) x SN_QT queries.
//   the list  after the butterfly every lane holds every d2 of the tile.  Lane 8 g + s of a wavefront keeps place s of query g's sorted list
//             of the KPX_SET_MAX_K lowest (d2, i): a candidate enters all eight lists with ONE shuffle from the lane below (the entry that
//             moves down) and two comparisons.  A pair is taken when d2 is finite, i is not the query's skipped index and the groups agree;
//             (d2, i) orders lexicographically, so ties go to the lowest index whatever the order of arrival.
//   the merge the four wavefronts' lists meet in LDS, one thread per query writes the block's k lowest and its count into the workspace;
//             the second launch, one thread per query, takes the blocks in ascending order.  Counts are integer sums.  No atomics anywhere.
#include "kpx_common.h"
#include <math.h>

enum { SN_RT = 4, SN_QT = 8, SN_WAVES = 4, SN_TILES = 4, SN_THREADS = SN_WAVES * KPX_WAVE, SN_K = KPX_SET_MAX_K };
static_assert(SN_RT * SN_WAVES * SN_TILES == KPX_SET_BLOCK, "a workgroup takes one block of refs");
static_assert(SN_QT * SN_K == KPX_WAVE, "one lane per (query of the tile, place of its list)");

__device__ __forceinline__ bool sn_better(double d, int c, double best_d, int best_c) { return d < best_d || (d == best_d && c < best_c); }

// (d, c) into the ascending list (bd, bc) of SN_K places; what falls off the end is dropped.  Static indices only: the list stays in registers.
__device__ __forceinline__ void sn_insert(double d, int c, double (&bd)[SN_K], int (&bc)[SN_K]) {
#pragma unroll
    for (int s = 0; s < SN_K; ++s)
        if (sn_better(d, c, bd[s], bc[s])) {
            const double td = bd[s];
            const int tc = bc[s];
            bd[s] = d; bc[s] = c;
            d = td; c = tc;
        }
}

__global__ __launch_bounds__(SN_THREADS) void set_neighbours_partial_kernel(const double* __restrict__ q, int M, const double* __restrict__ r, int N,
                                                                            int D, const int32_t* __restrict__ q_group,
                                                                            const int32_t* __restrict__ r_group, const int32_t* __restrict__ q_skip,
                                                                            const double* __restrict__ r_radius2, int k, double* __restrict__ part_d,
                                                                            int32_t* __restrict__ part_c, int32_t* __restrict__ part_n) {
    __shared__ double sh_d[SN_WAVES][KPX_WAVE];
    __shared__ int sh_c[SN_WAVES][KPX_WAVE];
    __shared__ int sh_n[SN_WAVES][SN_QT];
    const int lane = threadIdx.x & (KPX_WAVE - 1), wave = threadIdx.x / KPX_WAVE;
    const int block = blockIdx.x, q0 = blockIdx.y * SN_QT;
    const double* qp[SN_QT];
#pragma unroll
    for (int qi = 0; qi < SN_QT; ++qi) qp[qi] = q + (size_t)min(q0 + qi, M - 1) * D;     // a query past the set repeats the last one; its result is dropped
    // this lane's place in the lists: query g of the tile, place s
    const int g = lane >> 3, s = lane & 7;
    const int my_q = min(q0 + g, M - 1);
    const int my_skip = q_skip ? q_skip[my_q] : -1;
    const int my_group = q_group ? q_group[my_q] : 0;
    double list_d = INFINITY;
    int list_c = -1, count = 0;
    for (int tile = 0; tile < SN_TILES; ++tile) {
        const int i0 = block * KPX_SET_BLOCK + (tile * SN_WAVES + wave) * SN_RT;          // uniform in the wavefront
        if (i0 >= N) break;
        const double* rp[SN_RT];
#pragma unroll
        for (int ri = 0; ri < SN_RT; ++ri) rp[ri] = r + (size_t)min(i0 + ri, N - 1) * D;  // a ref past the set repeats the last one and is never eligible
        double acc[SN_RT][SN_QT];
#pragma unroll
        for (int ri = 0; ri < SN_RT; ++ri)
#pragma unroll
            for (int qi = 0; qi < SN_QT; ++qi) acc[ri][qi] = 0.0;
        for (int d = lane; d < D; d += KPX_WAVE) {
            double rv[SN_RT];
#pragma unroll
            for (int ri = 0; ri < SN_RT; ++ri) rv[ri] = rp[ri][d];
#pragma unroll
            for (int qi = 0; qi < SN_QT; ++qi) {
                const double qv = qp[qi][d];
#pragma unroll
                for (int ri = 0; ri < SN_RT; ++ri) {
                    const double e = qv - rv[ri];
                    acc[ri][qi] = fma(e, e, acc[ri][qi]);
                }
            }
        }
#pragma unroll
        for (int ri = 0; ri < SN_RT; ++ri) {
            double mine = 0.0;                                   // d2(query g, ref i0 + ri): every lane holds all eight, this one keeps its query's
#pragma unroll
            for (int qi = 0; qi < SN_QT; ++qi) {
                const double v = kpx_wave_sum_d(acc[ri][qi]);
                if (qi == g) mine = v;
            }
            const int i = i0 + ri;
            const int ic = min(i, N - 1);
            bool ok = i < N && mine < INFINITY && i != my_skip;  // a NaN compares false: never eligible
            if (r_group) ok = ok && r_group[ic] == my_group;
            if (r_radius2) {
                const double rad = r_radius2[ic];
                count += (ok && rad < INFINITY && mine <= rad) ? 1 : 0;
            }
            // sorted insertion, all eight lists at once: place s takes the entry of place s - 1 when the candidate goes in above it
            const double up_d = __shfl_up(list_d, 1, SN_K);
            const int up_c = __shfl_up(list_c, 1, SN_K);
            if (ok) {
                if (s > 0 && sn_better(mine, i, up_d, up_c)) { list_d = up_d; list_c = up_c; }
                else if (sn_better(mine, i, list_d, list_c)) { list_d = mine; list_c = i; }
            }
        }
    }
    sh_d[wave][lane] = list_d;
    sh_c[wave][lane] = list_c;
    if (s == 0) sh_n[wave][g] = count;
    __syncthreads();
    if (threadIdx.x < SN_QT && q0 + (int)threadIdx.x < M) {
        const int qi = threadIdx.x;
        double bd[SN_K];
        int bc[SN_K], n = 0;
#pragma unroll
        for (int t = 0; t < SN_K; ++t) { bd[t] = INFINITY; bc[t] = -1; }
        for (int w = 0; w < SN_WAVES; ++w) {
            n += sh_n[w][qi];
            for (int t = 0; t < SN_K; ++t) sn_insert(sh_d[w][qi * SN_K + t], sh_c[w][qi * SN_K + t], bd, bc);
        }
        const size_t o = (size_t)block * k * M + q0 + qi;        // [block][place][query]: the second launch reads along the queries
#pragma unroll
        for (int t = 0; t < SN_K; ++t)
            if (t < k) { part_d[o + (size_t)t * M] = bd[t]; part_c[o + (size_t)t * M] = bc[t]; }
        part_n[(size_t)block * M + q0 + qi] = n;
    }
}

// one thread per query: the blocks in ascending order
__global__ __launch_bounds__(256) void set_neighbours_combine_kernel(const double* __restrict__ part_d, const int32_t* __restrict__ part_c,
                                                                     const int32_t* __restrict__ part_n, int M, int n_blocks, int k,
                                                                     double* __restrict__ nn_d2, int32_t* __restrict__ nn_idx,
                                                                     int32_t* __restrict__ inside) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double bd[SN_K];
    int bc[SN_K], n = 0;
#pragma unroll
    for (int t = 0; t < SN_K; ++t) { bd[t] = INFINITY; bc[t] = -1; }
    for (int b = 0; b < n_blocks; ++b) {
        const size_t o = (size_t)b * k * M + j;
        for (int t = 0; t < k; ++t) {
            const int c = part_c[o + (size_t)t * M];
            if (c < 0) break;                                    // a block's list is ascending and its empty places come last
            sn_insert(part_d[o + (size_t)t * M], c, bd, bc);
        }
        n += part_n[(size_t)b * M + j];
    }
#pragma unroll
    for (int t = 0; t < SN_K; ++t)
        if (t < k) { nn_d2[(size_t)j * k + t] = bd[t]; nn_idx[(size_t)j * k + t] = bc[t]; }
    if (inside) inside[j] = n;
}

static bool sn_sizes_ok(int M, int N, int k) {
    return M >= 1 && M <= KPX_SET_MAX_QUERIES && N >= 1 && N <= KPX_SET_MAX_REFS && k >= 1 && k <= KPX_SET_MAX_K;
}

static size_t sn_blocks(int N) { return ((size_t)N + KPX_SET_BLOCK - 1) / KPX_SET_BLOCK; }

extern "C" size_t kpx_set_neighbours_workspace_bytes(int M, int N, int k) {
    if (!sn_sizes_ok(M, N, k)) return 0;
    return sn_blocks(N) * (size_t)M * ((size_t)k * (sizeof(double) + sizeof(int32_t)) + sizeof(int32_t));
}

extern "C" int kpx_set_neighbours_f64(const double* q, int M, const double* r, int N, int D, const int32_t* q_group, const int32_t* r_group,
                                      const int32_t* q_skip, const double* r_radius2, int k, void* workspace, size_t workspace_bytes,
                                      double* nn_d2, int32_t* nn_idx, int32_t* inside, void* stream) {
    if (!q || !r || !workspace || !nn_d2 || !nn_idx) return KPX_EINVAL;
    if (!sn_sizes_ok(M, N, k) || D < 1 || D > KPX_SET_MAX_DIM) return KPX_EINVAL;
    if ((q_group == nullptr) != (r_group == nullptr)) return KPX_EINVAL;                   // both or neither
    if ((r_radius2 == nullptr) != (inside == nullptr)) return KPX_EINVAL;                 // the count needs the radii, the radii the count
    if (workspace_bytes < kpx_set_neighbours_workspace_bytes(M, N, k)) return KPX_EINVAL;
    if (((((uintptr_t)q) | ((uintptr_t)r) | ((uintptr_t)r_radius2) | ((uintptr_t)workspace) | ((uintptr_t)nn_d2)) & 7) ||
        ((((uintptr_t)q_group) | ((uintptr_t)r_group) | ((uintptr_t)q_skip) | ((uintptr_t)nn_idx) | ((uintptr_t)inside)) & 3))
        return KPX_EINVAL;
    const int n_blocks = (int)sn_blocks(N);
    double* part_d = (double*)workspace;
    int32_t* part_c = (int32_t*)(part_d + (size_t)n_blocks * k * M);
    int32_t* part_n = part_c + (size_t)n_blocks * k * M;
    hipStream_t st = kpx_stream(stream);
    hipLaunchKernelGGL(set_neighbours_partial_kernel, dim3(n_blocks, (M + SN_QT - 1) / SN_QT), dim3(SN_THREADS), 0, st, q, M, r, N, D, q_group,
                       r_group, q_skip, r_radius2, k, part_d, part_c, part_n);
    int rc = kpx_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(set_neighbours_combine_kernel, dim3((M + 255) / 256), dim3(256), 0, st, part_d, part_c, part_n, M, n_blocks, k, nn_d2, nn_idx,
                       inside);
    return kpx_launch_status();
}
