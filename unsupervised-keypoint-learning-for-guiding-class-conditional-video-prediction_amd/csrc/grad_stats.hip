// Per-variable statistics of a flat bucket (train.py --grad-stats): for every variable, the sum of squares of its gradient and of its
// parameters (fp64), the largest finite |g| and the count of NaN / +-Inf gradient values.  One segmented reduction in two launches:
//   partial : one chunk (<= KPX_SEG_CHUNK elements of ONE variable, counted from the variable's own start) per workgroup -> one partial
//   fold    : one wavefront per variable adds the variable's partials in ascending order, then a butterfly
// The chunk table is the caller's (ops.grad_segment_table), in device memory.  No atomics; every result is bitwise reproducible and does
// not depend on where a variable starts in the bucket.  The padding floats between variables belong to no chunk and are never read.
#include "kpx_common.h"
#include "kpx_health.h"

static_assert(sizeof(KpxSegChunk) == 16 && sizeof(KpxSegRange) == 8 && sizeof(KpxSegStats) == 32, "segment table records");

#define SEG_LANES 256
#define SEG_ITERS (KPX_SEG_CHUNK / (SEG_LANES * 4))
static_assert(SEG_ITERS * SEG_LANES * 4 == KPX_SEG_CHUNK, "a chunk is a whole number of passes");

// Lane t owns the elements k*1024 + 4*t + j of the chunk (k < SEG_ITERS, j < 4), counted from the chunk's start, and adds them in ascending
// (k, j).  Whether the four arrive as one 16-byte load or four 4-byte loads changes no operand and no order.  Nothing at or beyond len is read.
template <bool VEC>
__device__ __forceinline__ void seg_chunk(const float* __restrict__ x, unsigned len, HealthAcc& a) {
    for (int k = 0; k < SEG_ITERS; ++k) {
        const unsigned i = (unsigned)k * (SEG_LANES * 4) + 4u * threadIdx.x;
        if (i >= len) break;
        if (VEC && i + 4 <= len) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(x + i);
            health_add(a, q[0]); health_add(a, q[1]); health_add(a, q[2]); health_add(a, q[3]);
        } else {
            for (unsigned j = 0; j < 4; ++j)
                if (i + j < len) health_add(a, x[i + j]);
        }
    }
}

// work = [C] fp64 sums of g^2, [C] fp64 sums of p^2, [C] fp32 maxima, [C] uint32 counts, C = number of chunks
__global__ __launch_bounds__(SEG_LANES) void seg_partial_kernel(const float* __restrict__ g, const float* __restrict__ p, size_t n,
                                                                const KpxSegChunk* __restrict__ chunks, unsigned n_chunks,
                                                                double* __restrict__ wsg, double* __restrict__ wsp,
                                                                float* __restrict__ wmax, unsigned* __restrict__ wbad) {
    __shared__ double sm_g[4], sm_p[4];
    __shared__ float sm_m[4];
    __shared__ unsigned sm_b[4];
    for (unsigned c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        size_t start = (size_t)chunks[c].start;                   // uniform over the workgroup
        unsigned len = chunks[c].len;
        if (len > KPX_SEG_CHUNK) len = KPX_SEG_CHUNK;             // a wrong table reads wrong elements of g[0:n], never others
        if (start >= n) { start = 0; len = 0; }
        else if ((size_t)len > n - start) len = (unsigned)(n - start);
        HealthAcc ag = {0.0, 0.0f, 0u}, ap = {0.0, 0.0f, 0u};
        if (((uintptr_t)(g + start) & 15) == 0) seg_chunk<true>(g + start, len, ag);
        else seg_chunk<false>(g + start, len, ag);
        if (p) {
            if (((uintptr_t)(p + start) & 15) == 0) seg_chunk<true>(p + start, len, ap);
            else seg_chunk<false>(p + start, len, ap);
        }
        const double sg = kpx_wave_sum_d(ag.s), sp = kpx_wave_sum_d(ap.s);
        const float mx = kpx_wave_max(ag.mx);
        unsigned bad = ag.bad;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += (unsigned)__shfl_xor((int)bad, o, 64);
        if ((threadIdx.x & 63) == 0) { sm_g[threadIdx.x >> 6] = sg; sm_p[threadIdx.x >> 6] = sp; sm_m[threadIdx.x >> 6] = mx; sm_b[threadIdx.x >> 6] = bad; }
        __syncthreads();
        if (threadIdx.x == 0) {
            wsg[c] = (sm_g[0] + sm_g[1]) + (sm_g[2] + sm_g[3]);
            wsp[c] = (sm_p[0] + sm_p[1]) + (sm_p[2] + sm_p[3]);
            wmax[c] = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
            wbad[c] = sm_b[0] + sm_b[1] + sm_b[2] + sm_b[3];
        }
        __syncthreads();                                          // the next chunk's waves overwrite sm_*
    }
}

// One wavefront per variable: lane t adds the variable's partials t, t+64, ... in ascending order, then the butterfly over the wavefront.
// The order depends on the variable's chunk count alone.  The count is carried in fp64 (exact to 2^53) and saturates at 2^32-1.
__global__ __launch_bounds__(64) void seg_fold_kernel(const double* __restrict__ wsg, const double* __restrict__ wsp,
                                                      const float* __restrict__ wmax, const unsigned* __restrict__ wbad, unsigned n_chunks,
                                                      const KpxSegRange* __restrict__ ranges, unsigned n_segs, KpxSegStats* __restrict__ out) {
    for (unsigned s = blockIdx.x; s < n_segs; s += gridDim.x) {
        unsigned first = ranges[s].first, count = ranges[s].count;
        if (first >= n_chunks) { first = 0; count = 0; }
        else if (count > n_chunks - first) count = n_chunks - first;
        double sg = 0.0, sp = 0.0, bad = 0.0;
        float mx = 0.0f;
        for (unsigned i = threadIdx.x; i < count; i += 64) {
            sg += wsg[first + i];
            sp += wsp[first + i];
            mx = fmaxf(mx, wmax[first + i]);
            bad += (double)wbad[first + i];
        }
        sg = kpx_wave_sum_d(sg); sp = kpx_wave_sum_d(sp); bad = kpx_wave_sum_d(bad); mx = kpx_wave_max(mx);
        if (threadIdx.x == 0) {
            KpxSegStats r;
            r.sumsq_g = sg;
            r.sumsq_p = sp;
            r.maxabs_g = mx;
            r.nonfinite_g = bad >= 4294967295.0 ? 0xffffffffu : (unsigned)bad;
            r.pad_[0] = r.pad_[1] = 0u;
            out[s] = r;
        }
    }
}

extern "C" size_t kpx_grad_segment_stats_workspace_bytes(size_t n_chunks) { return n_chunks * 24; }

extern "C" int kpx_grad_segment_stats_f32(const float* g, const float* p, size_t n, const KpxSegChunk* chunks, size_t n_chunks,
                                          const KpxSegRange* ranges, size_t n_segs, void* work, KpxSegStats* out, void* stream) {
    if (!g || !chunks || !ranges || !work || !out || n == 0 || n_chunks == 0 || n_segs == 0 || n_chunks >= ((size_t)1 << 31) ||
        n_segs >= ((size_t)1 << 31))
        return KPX_EINVAL;
    if (((((uintptr_t)g) | ((uintptr_t)p) | ((uintptr_t)ranges)) & 3) || ((((uintptr_t)chunks) | ((uintptr_t)work) | ((uintptr_t)out)) & 7))
        return KPX_EINVAL;
    double* wsg = (double*)work;
    double* wsp = wsg + n_chunks;
    float* wmax = (float*)(wsp + n_chunks);
    unsigned* wbad = (unsigned*)(wmax + n_chunks);
    hipStream_t s = kpx_stream(stream);
    hipLaunchKernelGGL(seg_partial_kernel, dim3((unsigned)(n_chunks < 2048 ? n_chunks : 2048)), dim3(SEG_LANES), 0, s, g, p, n, chunks,
                       (unsigned)n_chunks, wsg, wsp, wmax, wbad);
    int rc = kpx_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(seg_fold_kernel, dim3((unsigned)(n_segs < 2048 ? n_segs : 2048)), dim3(64), 0, s, (const double*)wsg, (const double*)wsp,
                       (const float*)wmax, (const unsigned*)wbad, (unsigned)n_chunks, ranges, (unsigned)n_segs, out);
    return kpx_launch_status();
}
