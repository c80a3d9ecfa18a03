// Animated grids (animate.py): one cell of a time-major canvas [B, T+1, rows*H, cols*W, 3] composed in one launch -- frame 0 from `first`
// [B,H,W,C], frames 1..T from `seq` [B,T,H,W,C], quantised to the bytes evaluate.py writes (kpx_png8_unit / kpx_png8_raw) as
// kpx_sheet_paste_u8_f32 does, with key-point markers (a filled disc and a one-pixel black outline) drawn over them.  DESIGN.md section 4.4.
//
// The stream is sheet.hip's: a lane takes G consecutive source values of one frame row (G = 16, 4 or 1 under the same width and alignment
// rules) and writes the 3 G / C bytes they become.  blockIdx.y walks the B (T+1) frames, blockIdx.x the items of a frame in row order, so a
// workgroup holds whole rows of ONE frame at a time; it stages that frame's K marker centres (1/16 pixel, integers) and the K colours in LDS
// once, and every lane then tests its pixels against them in integers: the same bytes on every path.  A wave spans two or three rows, so
// the row test `|16 y - cy| <= 16 r` is close to uniform and most centres cost one LDS broadcast and a compare.
#include "kpx_common.h"

namespace {

typedef uint32_t cf_u32x4 __attribute__((ext_vector_type(4)));
constexpr int CF_THREADS = 256;
constexpr int CF_MAX_BLOCKS = 2048;                                    // 8 workgroups per CU: grid-stride beyond that
constexpr int CF_MAX_POINTS = 64;
constexpr uint32_t CF_NONE = 0xffffffffu;                              // "no marker here" (a colour has 24 bits)
constexpr int CF_NOWHERE = 1 << 28;                                    // cy of a key point that draws nothing: no row is within 16 r of it

struct CfGeom {
    int frames, T, K;                 // B (T+1) frames of the canvas; frames per sample of seq; key points per frame
    int frame_floats, row_floats;     // H W C, W C
    int items;                        // per frame: H W C / G
    size_t image_bytes, line_bytes;   // of the canvas: rows H cols W 3, cols W 3
    size_t cell0;                     // byte offset of cell (row, col) in its image
    int r16, r16sq, rin16sq;          // 16 r, (16 r)^2, (16 (r - 1))^2
    float sx, sy;                     // (float)(16 (W - 1)), (float)(16 (H - 1))
};

template <int PREMAP>
__device__ __forceinline__ uint32_t cf_q(float x) {
    return (uint32_t)(PREMAP == KPX_SHEET_RAW ? kpx_png8_raw(x) : kpx_png8_unit(x));
}

// centre of a marker in 1/16 pixel: (int) rint(fl(fl(fl(v + 1) * 0.5) * scale)), every step rounded to fp32
__device__ __forceinline__ int cf_centre(float v, float scale) {
    return (int)rintf(kpx_mul_rn(kpx_mul_rn(kpx_add_rn(v, 1.0f), 0.5f), scale));
}

// markers of the NPIX pixels (y, p0 ..) of one row: CF_NONE, 0 (outline) or the packed colour of the lowest covering key point
template <int NPIX>
__device__ __forceinline__ bool cf_marks(const int2* ctr, const uint32_t* col, const CfGeom& g, int y, int p0, uint32_t (&mk)[NPIX]) {
#pragma unroll
    for (int j = 0; j < NPIX; ++j) mk[j] = CF_NONE;
    bool hit = false;
    const int y16 = 16 * y, x16 = 16 * p0;
    for (int k = g.K - 1; k >= 0; --k) {                               // descending: the lowest k is written last
        const int2 c = ctr[k];
        const int dy = y16 - c.y;
        if (abs(dy) > g.r16) continue;
        const int dy2 = dy * dy, dx0 = x16 - c.x;
        const uint32_t fill = col[k];
#pragma unroll
        for (int j = 0; j < NPIX; ++j) {
            const int dx = dx0 + 16 * j;
            if (abs(dx) <= g.r16) {                                    // |dx|, |dy| <= 256: the squares fit
                const int d2 = dx * dx + dy2;
                if (d2 <= g.r16sq) {
                    mk[j] = d2 <= g.rin16sq ? fill : 0u;
                    hit = true;
                }
            }
        }
    }
    return hit;
}

// output byte n of the item is channel (PHASE + n) % 3 of pixel slot (PHASE + n) / 3
template <int PHASE, int NB, int NPIX>
__device__ __forceinline__ void cf_overlay(uint32_t (&ob)[NB], const uint32_t (&mk)[NPIX]) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int s = (PHASE + n) / 3, ch = (PHASE + n) % 3;
        if (s < NPIX && mk[s] != CF_NONE) ob[n] = (mk[s] >> (8 * ch)) & 255u;
    }
}

template <int C, int G, int PREMAP, bool MARK>
__global__ __launch_bounds__(CF_THREADS) void cell_frames_kernel(const float* __restrict__ first, const float* __restrict__ seq,
                                                                 const float* __restrict__ pts_first, const float* __restrict__ pts_seq,
                                                                 const uint8_t* __restrict__ colors, CfGeom g, uint8_t* __restrict__ canvas) {
    constexpr int REP = 3 / C;                                         // output bytes per source value
    constexpr int NB = G * REP;                                        // output bytes per item
    constexpr int NPIX = (NB + 1) / 3 + 1;                             // pixels an item can touch (C = 3: it may start inside a pixel)
    __shared__ int2 ctr[CF_MAX_POINTS];
    __shared__ uint32_t col[CF_MAX_POINTS];
    if constexpr (MARK) {
        if ((int)threadIdx.x < g.K) {
            const uint8_t* c = colors + 3 * threadIdx.x;
            col[threadIdx.x] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
        }
    }
    const int t1 = g.T + 1;
    for (int f = blockIdx.y; f < g.frames; f += gridDim.y) {
        const int b = f / t1, t = f - b * t1;
        const float* s = t == 0 ? first + (size_t)b * g.frame_floats : seq + ((size_t)b * g.T + (t - 1)) * g.frame_floats;
        uint8_t* d = canvas + (size_t)f * g.image_bytes + g.cell0;
        if constexpr (MARK) {
            __syncthreads();                                           // the previous frame's centres are no longer read
            if ((int)threadIdx.x < g.K) {
                const float* p = (t == 0 ? pts_first + (size_t)b * g.K * 2 : pts_seq + ((size_t)b * g.T + (t - 1)) * g.K * 2) + 2 * threadIdx.x;
                const float x = p[0], y = p[1];
                int2 c;
                if (fabsf(x) <= 4.0f && fabsf(y) <= 4.0f) {            // (false for NaN and inf)
                    c.x = cf_centre(x, g.sx);
                    c.y = cf_centre(y, g.sy);
                } else {
                    c.x = 0;
                    c.y = CF_NOWHERE;
                }
                ctr[threadIdx.x] = c;
            }
            __syncthreads();
        }
        for (int it = blockIdx.x * CF_THREADS + threadIdx.x; it < g.items; it += gridDim.x * CF_THREADS) {
            const int fo = it * G;                                     // first value of the item in its frame (G divides W C: one row)
            const int y = fo / g.row_floats, xo = fo - y * g.row_floats;
            const int byte0 = xo * REP;                                // of the cell row
            uint8_t* o = d + (size_t)y * g.line_bytes + (size_t)byte0;
            uint32_t q[G];
            if constexpr (G == 1) {
                q[0] = cf_q<PREMAP>(s[fo]);
            } else {
#pragma unroll
                for (int k = 0; k < G / 4; ++k) {
                    const f32x4 v = reinterpret_cast<const f32x4*>(s + fo)[k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) q[4 * k + e] = cf_q<PREMAP>(v[e]);
                }
            }
            uint32_t ob[NB];                                           // output byte n = q[n / REP]
#pragma unroll
            for (int n = 0; n < NB; ++n) ob[n] = q[n / REP];
            if constexpr (MARK) {
                const int p0 = byte0 / 3, phase = byte0 - 3 * p0;
                uint32_t mk[NPIX];
                if (cf_marks<NPIX>(ctr, col, g, y, p0, mk)) {
                    if (C == 1 || phase == 0) cf_overlay<0, NB, NPIX>(ob, mk);
                    else if (phase == 1) cf_overlay<1, NB, NPIX>(ob, mk);
                    else cf_overlay<2, NB, NPIX>(ob, mk);
                }
            }
            if constexpr (G == 1) {
#pragma unroll
                for (int n = 0; n < NB; ++n) o[n] = (uint8_t)ob[n];
            } else {
                uint32_t w[NB / 4];
#pragma unroll
                for (int m = 0; m < NB / 4; ++m) w[m] = ob[4 * m] | (ob[4 * m + 1] << 8) | (ob[4 * m + 2] << 16) | (ob[4 * m + 3] << 24);
                if constexpr (G == 16) {
#pragma unroll
                    for (int m = 0; m < NB / 16; ++m) {
                        cf_u32x4 v;
                        v[0] = w[4 * m]; v[1] = w[4 * m + 1]; v[2] = w[4 * m + 2]; v[3] = w[4 * m + 3];
                        reinterpret_cast<cf_u32x4*>(o)[m] = v;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < NB / 4; ++m) reinterpret_cast<uint32_t*>(o)[m] = w[m];
                }
            }
        }
    }
}

struct CfArgs {
    const float *first, *seq, *pts_first, *pts_seq;
    const uint8_t* colors;
    uint8_t* canvas;
};

template <int C, int G, int PREMAP>
void cf_launch2(const CfArgs& a, const CfGeom& g, bool mark, dim3 grid, hipStream_t s) {
    const dim3 block(CF_THREADS);
    if (mark)
        hipLaunchKernelGGL((cell_frames_kernel<C, G, PREMAP, true>), grid, block, 0, s, a.first, a.seq, a.pts_first, a.pts_seq, a.colors, g,
                           a.canvas);
    else
        hipLaunchKernelGGL((cell_frames_kernel<C, G, PREMAP, false>), grid, block, 0, s, a.first, a.seq, a.pts_first, a.pts_seq, a.colors, g,
                           a.canvas);
}

template <int C, int G>
void cf_launch(const CfArgs& a, const CfGeom& g, bool mark, int premap, hipStream_t s) {
    const int bx_all = (g.items + CF_THREADS - 1) / CF_THREADS;
    const int bx = bx_all > CF_MAX_BLOCKS ? CF_MAX_BLOCKS : bx_all;
    const int by_cap = CF_MAX_BLOCKS / bx;                             // >= 1
    const dim3 grid(bx, g.frames > by_cap ? by_cap : g.frames);
    if (premap == KPX_SHEET_RAW) cf_launch2<C, G, KPX_SHEET_RAW>(a, g, mark, grid, s);
    else cf_launch2<C, G, KPX_SHEET_UNIT>(a, g, mark, grid, s);
}

}  // namespace

extern "C" int kpx_cell_frames_u8_f32(const float* first, const float* seq, int B, int T, int H, int W, int C, const float* pts_first,
                                      const float* pts_seq, int K, const uint8_t* colors, int radius, uint8_t* canvas, int rows, int cols,
                                      int row, int col, int premap, void* stream) {
    if (!first || !seq || !canvas || (((uintptr_t)first) & 3) || (((uintptr_t)seq) & 3) || B < 1 || T < 1 || H < 1 || H > 1024 || W < 1 ||
        W > 1024 || !(C == 1 || C == 3) || rows < 1 || rows > 64 || cols < 1 || cols > 64 || row < 0 || row >= rows || col < 0 || col >= cols ||
        radius < 0 || radius > 16 || !(premap == KPX_SHEET_UNIT || premap == KPX_SHEET_RAW))
        return KPX_EINVAL;
    const bool mark = radius >= 1;
    if (mark && (!pts_first || !pts_seq || !colors || (((uintptr_t)pts_first) & 3) || (((uintptr_t)pts_seq) & 3) || K < 1 || K > CF_MAX_POINTS))
        return KPX_EINVAL;
    if ((long long)B * (T + 1LL) > 0x7fffffffLL) return KPX_EINVAL;
    CfGeom g;
    g.frames = B * (T + 1);
    g.T = T;
    g.K = mark ? K : 0;
    g.frame_floats = H * W * C;                                        // <= 3 * 2^20
    g.row_floats = W * C;
    g.line_bytes = (size_t)cols * W * 3;
    g.image_bytes = (size_t)rows * H * g.line_bytes;
    g.cell0 = (size_t)row * H * g.line_bytes + (size_t)col * W * 3;
    g.r16 = 16 * radius;
    g.r16sq = g.r16 * g.r16;
    g.rin16sq = mark ? 256 * (radius - 1) * (radius - 1) : 0;
    g.sx = (float)(16 * (W - 1));
    g.sy = (float)(16 * (H - 1));
    const bool src16 = ((((uintptr_t)first) | ((uintptr_t)seq)) & 15) == 0;
    const int G = W % 16 == 0 && src16 && (((uintptr_t)canvas) & 15) == 0 ? 16 : W % 4 == 0 && src16 && (((uintptr_t)canvas) & 3) == 0 ? 4 : 1;
    g.items = g.frame_floats / G;
    const CfArgs a = {first, seq, pts_first, pts_seq, colors, canvas};
    hipStream_t s = kpx_stream(stream);
    if (C == 3) {
        if (G == 16) cf_launch<3, 16>(a, g, mark, premap, s);
        else if (G == 4) cf_launch<3, 4>(a, g, mark, premap, s);
        else cf_launch<3, 1>(a, g, mark, premap, s);
    } else {
        if (G == 16) cf_launch<1, 16>(a, g, mark, premap, s);
        else if (G == 4) cf_launch<1, 4>(a, g, mark, premap, s);
        else cf_launch<1, 1>(a, g, mark, premap, s);
    }
    return kpx_launch_status();
}
