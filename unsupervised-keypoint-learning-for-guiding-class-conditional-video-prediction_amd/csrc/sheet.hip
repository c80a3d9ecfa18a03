// Contact sheets (evaluate.py --actions): J frames of a rollout src [B,F,H,W,C] quantised to the bytes evaluate.py writes (kpx_png8_unit /
// kpx_png8_raw) and pasted side by side into one row of cells of an 8-bit RGB canvas [B, rows*H, cols*W, 3].  DESIGN.md section 4.4.
//
// A pure stream: 4 C bytes in, 3 bytes out per pixel.  A frame is contiguous in src and a cell row is contiguous in the canvas, and for
// C = 3 output byte n of a cell row is the quantised source value n of the frame row, so a lane takes G consecutive source values of one
// frame row and writes the 3 G / C bytes they become:
//   G = 16  four 16-byte loads -> one (C = 3) or three (C = 1) 16-byte stores; needs W % 16 == 0 and 16-byte aligned src and canvas
//           (every cell row then starts on a multiple of 48 bytes);
//   G = 4   one 16-byte load -> one or three 4-byte stores; needs W % 4 == 0, src 16-byte and canvas 4-byte aligned;
//   G = 1   one value -> one or three byte stores: odd widths and misaligned bases.
// blockIdx.y walks the (sample, pasted frame) cells, blockIdx.x the items of a cell, both grid-strided under a cap of SP_MAX_BLOCKS
// workgroups.  The frame indices are launch arguments (a cell is uniform over its workgroup: one scalar load), so the call needs no device
// index buffer and replays from a captured graph.
#include "kpx_common.h"

namespace {

typedef uint32_t sp_u32x4 __attribute__((ext_vector_type(4)));
constexpr int SP_THREADS = 256;
constexpr int SP_MAX_BLOCKS = 2048;                                   // 8 workgroups per CU: grid-stride beyond that

struct SpFrames { int f[KPX_SHEET_MAX_FRAMES]; };

struct SpGeom {
    int cells, J, F;                  // B * J cells; frames per sample of src
    int frame_floats, row_floats;     // H W C, W C
    int items;                        // per cell: H W C / G
    size_t image_bytes, line_bytes;   // of the canvas: rows H cols W 3, cols W 3
    size_t cell0;                     // byte offset of cell (row, col) in its image
    int cell_bytes;                   // W 3
};

template <int PREMAP>
__device__ __forceinline__ uint32_t sp_q(float x) {
    return (uint32_t)(PREMAP == KPX_SHEET_RAW ? kpx_png8_raw(x) : kpx_png8_unit(x));
}

template <int C, int G, int PREMAP>
__global__ __launch_bounds__(SP_THREADS) void sheet_paste_kernel(const float* __restrict__ src, SpGeom g, SpFrames fr,
                                                                 uint8_t* __restrict__ canvas) {
    constexpr int REP = 3 / C;                                         // output bytes per source value
    constexpr int NB = G * REP;                                        // output bytes per item
    for (int cell = blockIdx.y; cell < g.cells; cell += gridDim.y) {
        const int b = cell / g.J, j = cell - b * g.J;
        const float* s = src + ((size_t)b * g.F + fr.f[j]) * g.frame_floats;
        uint8_t* d = canvas + (size_t)b * g.image_bytes + g.cell0 + (size_t)j * g.cell_bytes;
        for (int it = blockIdx.x * SP_THREADS + threadIdx.x; it < g.items; it += gridDim.x * SP_THREADS) {
            const int fo = it * G;                                     // first value of the item in its frame (G divides W C: one row)
            const int y = fo / g.row_floats, xo = fo - y * g.row_floats;
            uint8_t* o = d + (size_t)y * g.line_bytes + (size_t)xo * REP;
            uint32_t q[G];
            if constexpr (G == 1) {
                q[0] = sp_q<PREMAP>(s[fo]);
#pragma unroll
                for (int n = 0; n < NB; ++n) o[n] = (uint8_t)q[0];
            } else {
#pragma unroll
                for (int k = 0; k < G / 4; ++k) {
                    const f32x4 v = reinterpret_cast<const f32x4*>(s + fo)[k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) q[4 * k + e] = sp_q<PREMAP>(v[e]);
                }
                uint32_t w[NB / 4];                                    // output byte n = q[n / REP]
#pragma unroll
                for (int m = 0; m < NB / 4; ++m)
                    w[m] = q[(4 * m) / REP] | (q[(4 * m + 1) / REP] << 8) | (q[(4 * m + 2) / REP] << 16) | (q[(4 * m + 3) / REP] << 24);
                if constexpr (G == 16) {
#pragma unroll
                    for (int m = 0; m < NB / 16; ++m) {
                        sp_u32x4 t;
                        t[0] = w[4 * m]; t[1] = w[4 * m + 1]; t[2] = w[4 * m + 2]; t[3] = w[4 * m + 3];
                        reinterpret_cast<sp_u32x4*>(o)[m] = t;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < NB / 4; ++m) reinterpret_cast<uint32_t*>(o)[m] = w[m];
                }
            }
        }
    }
}

template <int C, int G>
void sp_launch(const float* src, const SpGeom& g, const SpFrames& fr, uint8_t* canvas, int premap, hipStream_t s) {
    const int bx_all = (g.items + SP_THREADS - 1) / SP_THREADS;
    const int bx = bx_all > SP_MAX_BLOCKS ? SP_MAX_BLOCKS : bx_all;
    const int by_cap = SP_MAX_BLOCKS / bx;                             // >= 1
    const dim3 grid(bx, g.cells > by_cap ? by_cap : g.cells), block(SP_THREADS);
    if (premap == KPX_SHEET_RAW)
        hipLaunchKernelGGL((sheet_paste_kernel<C, G, KPX_SHEET_RAW>), grid, block, 0, s, src, g, fr, canvas);
    else
        hipLaunchKernelGGL((sheet_paste_kernel<C, G, KPX_SHEET_UNIT>), grid, block, 0, s, src, g, fr, canvas);
}

}  // namespace

extern "C" int kpx_sheet_paste_u8_f32(const float* src, int B, int F, int H, int W, int C, const int* frames, int J, uint8_t* canvas, int rows,
                                      int cols, int row, int col, int premap, void* stream) {
    if (!src || !frames || !canvas || (((uintptr_t)src) & 3) || B < 1 || F < 1 || H < 1 || H > 1024 || W < 1 || W > 1024 || !(C == 1 || C == 3) ||
        J < 1 || J > KPX_SHEET_MAX_FRAMES || rows < 1 || rows > 64 || cols < 1 || cols > 64 || row < 0 || row >= rows || col < 0 ||
        col > cols - J || !(premap == KPX_SHEET_UNIT || premap == KPX_SHEET_RAW))
        return KPX_EINVAL;
    SpFrames fr;
    for (int j = 0; j < KPX_SHEET_MAX_FRAMES; ++j) {
        fr.f[j] = j < J ? frames[j] : 0;
        if (fr.f[j] < 0 || fr.f[j] >= F) return KPX_EINVAL;
    }
    if ((long long)B * J > 0x7fffffffLL) return KPX_EINVAL;
    SpGeom g;
    g.cells = B * J;
    g.J = J;
    g.F = F;
    g.frame_floats = H * W * C;                                        // <= 3 * 2^20
    g.row_floats = W * C;
    g.cell_bytes = W * 3;
    g.line_bytes = (size_t)cols * W * 3;
    g.image_bytes = (size_t)rows * H * g.line_bytes;
    g.cell0 = (size_t)row * H * g.line_bytes + (size_t)col * W * 3;
    const bool src16 = (((uintptr_t)src) & 15) == 0;
    const int G = W % 16 == 0 && src16 && (((uintptr_t)canvas) & 15) == 0 ? 16 : W % 4 == 0 && src16 && (((uintptr_t)canvas) & 3) == 0 ? 4 : 1;
    g.items = g.frame_floats / G;
    hipStream_t s = kpx_stream(stream);
    if (C == 3) {
        if (G == 16) sp_launch<3, 16>(src, g, fr, canvas, premap, s);
        else if (G == 4) sp_launch<3, 4>(src, g, fr, canvas, premap, s);
        else sp_launch<3, 1>(src, g, fr, canvas, premap, s);
    } else {
        if (G == 16) sp_launch<1, 16>(src, g, fr, canvas, premap, s);
        else if (G == 4) sp_launch<1, 4>(src, g, fr, canvas, premap, s);
        else sp_launch<1, 1>(src, g, fr, canvas, premap, s);
    }
    return kpx_launch_status();
}
