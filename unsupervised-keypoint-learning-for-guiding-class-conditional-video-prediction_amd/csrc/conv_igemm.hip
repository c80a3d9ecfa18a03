// fp32 implicit-GEMM convolution for gfx950 (MI355X): forward and dgrad on
// v_mfma_f32_32x32x2_f32 (exact f32 fma chain, 157 TF peak); the weight gradients are in conv_wgrad.hip.
//
// Replaces tf.layers.conv2d / tf.nn.conv2d of the reference (models/networks/layers.py:6-9,
// models/networks/vgg.py:51) and their TF-generated data gradients.
//
// One "gather conv" kernel serves forward and dgrad:
//   out[n, a*osy+oy0, b*osx+ox0, j] = act( bias[j] + sum_{tr,tq,c} in[n, a*isy+tr*ity+iy0, b*isx+tq*itx+ix0, c] * B[tap(tr,tq)][c][j] )
// forward : in = x, B = HWIO weights as stored ([c][j] row-major),   a,b = output pixel, input step = stride
// dgrad   : in = dy, B = the same HWIO weights read transposed ([j][c]), one launch per stride-parity class of
//           dx pixels so that no MFMA is spent on the zeros of a dilated gradient.
// GEMM view: M = N*Ha*Wa pixels, N = output channels, K = taps*Cin; the A tile (pixels x 16 channels) is gathered
// straight from NHWC (channels contiguous -> 16-B loads), staged in LDS [m][16+4] and read back as ds_read_b128;
// the B tile is staged [k][n] and read as ds_read_b32.  Within a 16-wide K chunk lane-half h consumes channels
// {8u+4h+j}: a K permutation shared by A and B, so the product is unchanged.
#include "kpx_internal.h"
#include "kpx_bf16.h"

// Tile geometry: BM x BN outputs per workgroup, WM x WN wavefronts each owning (BM/WM) x (BN/WN) as 32x32 MFMA
// accumulators, K chunks of 32 channels.  LDS (double buffered): A [BM][32] with the 16-B slot index XOR-swizzled by
// ((row>>1)&7) -- conflict-free for both the 8-lane ds_write_b128 groups (one row = 128 contiguous bytes = one full cache
// line of the pixel's channels) and the 16-lane ds_read_b128 groups; B [32][BN], for dgrad (weights read transposed) the
// column index is XORed with ((k>>2)&7)<<2 so the scalar transposing writes spread over all banks.
// 16 zero bytes in the code object: invalid (out-of-image / out-of-range) 16-B units are loaded from here, so the
// TAIL=false kernels need no per-element select between the load and the LDS write.
__device__ __attribute__((aligned(16))) float kpx_zero16[4] = {0.f, 0.f, 0.f, 0.f};          // (each translation unit that needs it has its own)

template <int BM, int BN, int WM, int WN, bool BT, bool VEC, bool MERGE, bool TAIL>
__global__ __launch_bounds__(WM * WN * 64) void conv_igemm_kernel(const ConvGeom g) {
    constexpr int NT = WM * WN * 64;
    constexpr int BK = 32;
    constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
    constexpr int RA = (BM * 8) / NT;              // A float4 units per thread (BM rows x 8 slots)
    constexpr int RB = (BN * 8 + NT - 1) / NT;     // B float4 units per thread (32 x BN/4, or BN rows x 8 slots when BT)
    constexpr int BU = BN * 8;
    constexpr int ASZ = BM * BK, BSZ = BK * BN;    // floats per LDS stage
    static_assert(TM >= 1 && TN >= 1 && RA >= 1 && (BM * 8) % NT == 0, "tile/wave shape");
    __shared__ __attribute__((aligned(16))) float As[2 * ASZ];
    __shared__ __attribute__((aligned(16))) float Bs[2 * BSZ];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const ConvClass k = g.cls[blockIdx.y];
    const int L = kpx_xcd_remap(blockIdx.x, gridDim.x);
    if (L >= k.mt * g.nt) return;                  // this class has fewer tiles than the widest one
    const int m0 = (L / g.nt) * BM, n0 = (L % g.nt) * BN;
    const int HW = k.Ha * k.Wa;
    const int wrow = wm * TM * 32, wcol = wn * TN * 32;

    // ---- everything that does not change over the K loop is computed once per thread: pointers of the A / B units at
    // tap (0,0) / channel 0, their validity as bit masks over the taps, and all LDS addresses.  Per chunk only wave-uniform
    // (scalar) offsets are added, so the loop carries ~2 VALU per MFMA instead of ~6.
    const int kq = t & 7;
    const float* a_ptr[RA];
    unsigned a_vr[RA], a_vq[RA];
    int a_iw0[RA], a_st[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int row = (t >> 3) + (NT / 8) * i;
        const int m = m0 + row;
        const bool ok = m < k.M;
        const int mm = ok ? m : 0;
        const int n = mm / HW, rem = mm - n * HW, a = rem / k.Wa, b = rem - a * k.Wa;
        const int ih0 = a * g.isy + k.iy0, iw0 = b * g.isx + k.ix0;
        a_ptr[i] = g.x + (ptrdiff_t)(n * g.Hi * g.Wi + ih0 * g.Wi + iw0) * g.ldx + kq * 4;
        unsigned vr = 0, vq = 0;
        for (int r = 0; r < k.Tr; ++r) if (ok && (unsigned)(ih0 + r * g.ity) < (unsigned)g.Hi) vr |= 1u << r;
        for (int q = 0; q < k.Tq; ++q) if (MERGE || (unsigned)(iw0 + q * g.itx) < (unsigned)g.Wi) vq |= 1u << q;
        a_vr[i] = vr; a_vq[i] = vq; a_iw0[i] = iw0;
        a_st[i] = row * BK + ((kq ^ ((row >> 1) & 7)) << 2);
    }
    const float* b_ptr[RB];
    bool b_ok[RB];
    int b_k[RB], b_n[RB], b_st[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int u = t + NT * i;
        if (!BT) {
            const int kr = u / (BN / 4), n4 = u % (BN / 4), n = n0 + n4 * 4;
            b_k[i] = kr; b_n[i] = n; b_ok[i] = u < BU && n < g.Cout;
            b_ptr[i] = g.w + (size_t)kr * g.ldw + n;
            b_st[i] = kr * BN + n4 * 4;
        } else {
            const int nn = u >> 3, ks = u & 7, n = n0 + nn;
            b_k[i] = ks * 4; b_n[i] = n; b_ok[i] = u < BU && n < g.Cout;
            b_ptr[i] = g.w + (size_t)n * g.ldw + ks * 4;
            b_st[i] = (ks * 4) * BN + (nn ^ (ks << 2));
        }
    }
    int a_rd[TM][4], b_rd[TN][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int ks = 2 * u + lh;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = wrow + i * 32 + li;
            a_rd[i][u] = row * BK + ((ks ^ ((row >> 1) & 7)) << 2);
        }
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            const int col = wcol + n * 32 + li;
            b_rd[n][u] = (ks * 4) * BN + (BT ? (col ^ (ks << 2)) : col);
        }
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nck = (g.Cin + BK - 1) / BK;
    int nchunks = k.Tr * k.Tq * nck;
    int tr = 0, tq = 0, c0 = 0;
    if (g.ksplit > 1) {                                 // this workgroup's slice of the K loop
        const int cps = (nchunks + g.ksplit - 1) / g.ksplit;
        const int cb = blockIdx.z * cps, ce = min(nchunks, cb + cps);
        const int tap0 = cb / nck;
        c0 = (cb - tap0 * nck) * BK; tr = tap0 / k.Tq; tq = tap0 - tr * k.Tq;
        nchunks = ce > cb ? ce - cb : 0;
    }
    f32x4 ra[RA], rb[RB];
    unsigned am[RA], bm[RB];

    auto tail4 = [](int c, int lim) -> unsigned {      // bit j set iff c + j < lim
        const int r = lim - c;
        return r >= 4 ? 15u : (r <= 0 ? 0u : (15u >> (4 - r)));
    };
    auto load4 = [&](const float* p, unsigned mask, const float* safe) -> f32x4 {
        f32x4 v;
        if (VEC) {
            v = *reinterpret_cast<const f32x4*>(mask ? p : safe);
        } else {
            v[0] = *((mask & 1u) ? p : safe);
            v[1] = *((mask & 2u) ? p + 1 : safe);
            v[2] = *((mask & 4u) ? p + 2 : safe);
            v[3] = *((mask & 8u) ? p + 3 : safe);
        }
        return v;
    };
    // Loads go out unconditionally: an invalid unit reads the 16 zero bytes of kpx_zero16 (or, with TAIL, a clamped
    // address that is masked when the registers are written to LDS), so nothing in the MFMA phase depends on them.
    auto load_chunk = [&]() {
        const int a_off = ((tr * g.ity) * g.Wi + tq * g.itx) * g.ldx + c0;          // wave-uniform
        const int tap = (k.wr0 + tr * g.wrs) * g.KW + (k.wq0 + tq * g.wqs);
        const size_t b_off = (size_t)tap * g.wts + (BT ? (size_t)c0 : (size_t)c0 * g.ldw);
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int c = c0 + kq * 4;
            const bool v = (((a_vr[i] >> tr) & (a_vq[i] >> tq)) & 1u) != 0 && c < g.Cin;
            const float* p = a_ptr[i] + a_off;
            unsigned mask = v ? 15u : 0u;
            if (TAIL) {
                if (MERGE) {
                    mask = 0;
                    if (v) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (c + j < g.Cin && (unsigned)(a_iw0[i] + (c + j) / g.merge) < (unsigned)g.Wi) mask |= 1u << j;
                    }
                } else if (v) {
                    mask = tail4(c, g.Cin);
                }
            }
            am[i] = mask;
            ra[i] = load4(p, mask, TAIL ? g.x : kpx_zero16);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const bool v = b_ok[i] && c0 + b_k[i] < g.Cin;
            unsigned mask = v ? 15u : 0u;
            if (TAIL && v) mask = BT ? tail4(c0 + b_k[i], g.Cin) : tail4(b_n[i], g.Cout);
            bm[i] = mask;
            rb[i] = load4(b_ptr[i] + b_off, mask, TAIL ? g.w : kpx_zero16);
        }
        c0 += BK;
        if (c0 >= g.Cin) {
            c0 = 0;
            if (++tq == k.Tq) { tq = 0; ++tr; }
        }
    };
    auto masked = [](f32x4 v, unsigned m) -> f32x4 {
        if (!TAIL) return v;
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (m >> j) & 1u ? v[j] : 0.f;
        return r;
    };
    auto store_chunk = [&](int buf) {                  // buf is a compile-time constant at every call site
#pragma unroll
        for (int i = 0; i < RA; ++i)
            *reinterpret_cast<f32x4*>(&As[buf * ASZ + a_st[i]]) = masked(ra[i], am[i]);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (t + NT * i < BU) {
                const f32x4 v = masked(rb[i], bm[i]);
                if (!BT) {
                    *reinterpret_cast<f32x4*>(&Bs[buf * BSZ + b_st[i]]) = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) Bs[buf * BSZ + b_st[i] + j * BN] = v[j];
                }
            }
        }
    };
    // one group = 8 k-steps: lane-half lh consumes channels 4*(2u+lh) .. +3 of the chunk (a K permutation shared by A and B).
    // The fragments of group u+1 are read from LDS before the MFMAs of group u are issued (register double buffering), so
    // only the first group of a chunk exposes the LDS latency.
    struct Frag { f32x4 a[TM]; float b[4][TN]; };
    auto read_frag = [&](int buf, int u, Frag& f) {
#pragma unroll
        for (int i = 0; i < TM; ++i) f.a[i] = *reinterpret_cast<const f32x4*>(&As[buf * ASZ + a_rd[i][u]]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int n = 0; n < TN; ++n) f.b[j][n] = Bs[buf * BSZ + b_rd[n][u] + j * BN];
    };
    auto mfma_frag = [&](const Frag& f) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int n = 0; n < TN; ++n)
                    acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[i][j], f.b[j][n], acc[i][n], 0, 0, 0);
    };
    // The next chunk's global loads are issued after the first group and written to the other LDS buffer after the third,
    // so their address arithmetic, the wait and the ds_writes sit between MFMAs instead of in the gap around the barrier.
    auto chunk = [&](auto bufc, bool more) {
        constexpr int buf = decltype(bufc)::value;
        Frag f0, f1;
        read_frag(buf, 0, f0);
        read_frag(buf, 1, f1);
        mfma_frag(f0);
        if (more) load_chunk();
        read_frag(buf, 2, f0);
        mfma_frag(f1);
        read_frag(buf, 3, f1);
        mfma_frag(f0);
        if (more) store_chunk(buf ^ 1);
        mfma_frag(f1);
        __syncthreads();
    };

    if (nchunks > 0) {
        load_chunk();
        store_chunk(0);
    }
    __syncthreads();
    int ch = 0;
    for (; ch + 1 < nchunks; ch += 2) {                // unrolled by two: the LDS buffer index is an immediate
        chunk(kpx_ic<0>{}, true);
        chunk(kpx_ic<1>{}, ch + 2 < nchunks);
    }
    if (ch < nchunks) chunk(kpx_ic<0>{}, false);

    // epilogue: the output pixel of every tile row goes through LDS (the A buffers are free now)
    int* rowpix = reinterpret_cast<int*>(&As[0]);
    if (t < BM) {
        const int m = m0 + t;
        int pix = -1;
        if (m < k.M) {
            const int n = m / HW, rem = m - n * HW, a = rem / k.Wa, b = rem - a * k.Wa;
            pix = (n * g.Ho + a * g.osy + k.oy0) * g.Wo + b * g.osx + k.ox0;
        }
        rowpix[t] = pix;
    }
    __syncthreads();
    if (g.ksplit > 1) {                                 // raw partial sums; bias / activation happen in splitk_reduce_kernel
        float* wsl = g.ws + (size_t)blockIdx.z * g.ws_slab;
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            const int col = n0 + wcol + n * 32 + li;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pix = rowpix[wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
                    if (col < g.Cout && pix >= 0) wsl[(size_t)pix * g.Cout + col] = acc[i][n][r];
                }
        }
        return;
    }
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        const int col = n0 + wcol + n * 32 + li;
        const bool cok = col < g.Cout;
        const float bv = (cok && g.bias) ? g.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int pix = rowpix[row];
                if (cok && pix >= 0) {
                    float v = acc[i][n][r] + bv;
                    if (g.act == KPX_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (g.act == KPX_ACT_LRELU) v = v > 0.f ? v : 0.01f * v;
                    else if (g.act == KPX_ACT_TANH) v = tanhf(v);
                    if (g.mul_y) v *= kpx_act_grad_from_y(g.mul_y[(size_t)pix * g.ld_mul + col], g.mul_act);
                    g.y[(size_t)pix * g.ldy + col] = v;
                }
            }
        }
    }
}

// y[pix][c] = act( bias[c] + sum_s ws[s][pix][c] ), fixed summation order
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, size_t slab, int S, size_t npix, int C,
                                                            const float* __restrict__ bias, int act, float* __restrict__ y, int ldy,
                                                            const float* __restrict__ mul_y, int ld_mul, int mul_act, int io16 = 0) {
    const int C4 = C >> 2;                              // C % 4 == 0 is a precondition of the split-K path
    const size_t total = npix * (size_t)C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / C4;
        const int c = (int)(i - pix * C4) * 4;
        f32x4 a = *reinterpret_cast<const f32x4*>(ws + pix * C + c);
        for (int s2 = 1; s2 < S; ++s2) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(ws + (size_t)s2 * slab + pix * C + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += b[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = a[j] + (bias ? bias[c + j] : 0.f);
            if (act == KPX_ACT_RELU) v = fmaxf(v, 0.f);
            else if (act == KPX_ACT_LRELU) v = v > 0.f ? v : 0.01f * v;
            else if (act == KPX_ACT_TANH) v = tanhf(v);
            a[j] = v;
        }
        if (mul_y) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float my = (io16 & 4) ? __builtin_bit_cast(float, (unsigned)reinterpret_cast<const unsigned short*>(mul_y)[pix * ld_mul + c + j] << 16) : mul_y[pix * ld_mul + c + j];
                a[j] *= kpx_act_grad_from_y(my, mul_act);
            }
        }
        if (io16 & 2) {                                  // bf16 output (the bf16 configuration): four channels = 8 bytes
            typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
            const bf16x4 o = {(__bf16)a[0], (__bf16)a[1], (__bf16)a[2], (__bf16)a[3]};
            *reinterpret_cast<bf16x4*>(reinterpret_cast<unsigned short*>(y) + pix * ldy + c) = o;
        } else *reinterpret_cast<f32x4*>(y + pix * ldy + c) = a;
    }
}

// Split-K plan (shape only): used when the 128x128 tiling would leave most CUs idle (small M, long K).
static int conv_splitk_plan(long M, int Cout, long nchunks_total) {
    if (Cout % 4 != 0 || Cout < 64) return 1;
    const long tiles = ((M + 127) / 128) * ((Cout + 127) / 128);
    const long max_tiles = 256;                          // a full round of 128x128 tiles: splitting only adds the reduce pass
    if (tiles >= max_tiles) return 1;
    long S = 512 / tiles;
    if (S > 8) S = 8;
    while (S > 1 && nchunks_total / S < 6) --S;         // keep >= 6 chunks (192 channels-taps) per split
    if ((double)S * (double)M * Cout * 4.0 > (double)((size_t)256 << 20)) return 1;
    return (int)(S < 1 ? 1 : S);
}

// The second launch of a split-K convolution: the g.ksplit partial slabs in g.ws -> y, with the bias / activation / multiplier epilogue
// (g.io16 is 0 wherever the fp32 kernels of this file made the slabs: bf16 tensors only reach conv_gemm3.hip)
static int launch_splitk_reduce(const ConvGeom& g, hipStream_t s) {
    const size_t npix = (size_t)g.N * g.Ho * g.Wo;
    size_t nb = (npix * (g.Cout / 4) + 255) / 256; if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const float*)g.ws, g.ws_slab, g.ksplit, npix, g.Cout,
                       g.bias, g.act, g.y, g.ldy, g.mul_y, g.ld_mul, g.mul_act, g.io16);
    return kpx_launch_status();
}

template <bool BT, bool VEC, bool MERGE, bool TAIL>
static int launch_gather_conv_v(ConvGeom g, hipStream_t s) {
    if (g.ncls <= 0) { g.ncls = 1; g.cls[0] = ConvClass{g.Ha, g.Wa, g.oy0, g.ox0, g.Tr, g.Tq, g.iy0, g.ix0, g.wr0, g.wq0, 0, 0}; }
    g.M = 0;
    for (int i = 0; i < g.ncls; ++i) { g.cls[i].M = g.N * g.cls[i].Ha * g.cls[i].Wa; if (g.cls[i].M > g.M) g.M = g.cls[i].M; }
    if (g.M <= 0 || g.Cout <= 0) return 0;
    if (g.ksplit > 1) {                                 // decided by the entry point (needs the caller's workspace)
        const int BMs = 128, BNs = g.Cout > 64 ? 128 : 64;
        g.nt = (g.Cout + BNs - 1) / BNs;
        int mtmax = 0;
        for (int i = 0; i < g.ncls; ++i) { g.cls[i].mt = (g.cls[i].M + BMs - 1) / BMs; if (g.cls[i].mt > mtmax) mtmax = g.cls[i].mt; }
        g.mt = mtmax;
        const dim3 nblk((unsigned)(g.mt * g.nt), (unsigned)g.ncls, (unsigned)g.ksplit);
        if (BNs == 128) hipLaunchKernelGGL((conv_igemm_kernel<128, 128, 2, 4, BT, VEC, MERGE, TAIL>), nblk, dim3(512), 0, s, g);
        else hipLaunchKernelGGL((conv_igemm_kernel<128, 64, 4, 2, BT, VEC, MERGE, TAIL>), nblk, dim3(512), 0, s, g);
        const int rc = kpx_launch_status();
        return rc ? rc : launch_splitk_reduce(g, s);
    }
    // N tile: smallest padded width, ties -> wider tile
    int BN = 128;
    {
        auto pad = [&](int b) { return (g.Cout + b - 1) / b * b; };
        if (pad(64) < pad(BN)) BN = 64;
        if (pad(32) < pad(BN)) BN = 32;
    }
    auto blocks = [&](int bm, int bn) {
        long b = 0;
        for (int i = 0; i < g.ncls; ++i) b += (long)((g.cls[i].M + bm - 1) / bm) * ((g.Cout + bn - 1) / bn);
        return b;
    };
    // pick the tile by how well its workgroup count fills 256 CUs x resident workgroups per CU (LDS-limited)
    int BM = 128;
    if (BN != 32) {
        struct Cand { int bm, bn, occ; double eff; };
        const Cand c128[] = {{128, 128, 2, 1.0}, {64, 128, 3, 0.92}, {128, 64, 3, 0.92}, {64, 64, 5, 0.85}};
        const Cand c64[] = {{128, 64, 3, 1.0}, {64, 64, 5, 0.92}};
        const Cand* cs = BN == 128 ? c128 : c64;
        const int nc = BN == 128 ? 4 : 2;
        double best = -1;
        for (int i = 0; i < nc; ++i) {
            const long nb = blocks(cs[i].bm, cs[i].bn), slots = 256L * cs[i].occ;
            const long rounds = (nb + slots - 1) / slots;
            const double score = cs[i].eff * (double)nb / (double)(rounds * slots);
            if (score > best) { best = score; BM = cs[i].bm; BN = cs[i].bn; }
        }
    }
    g.nt = (g.Cout + BN - 1) / BN;
    int mtmax = 0;
    for (int i = 0; i < g.ncls; ++i) { g.cls[i].mt = (g.cls[i].M + BM - 1) / BM; if (g.cls[i].mt > mtmax) mtmax = g.cls[i].mt; }
    g.mt = mtmax;
    const dim3 nblk((unsigned)(g.mt * g.nt), (unsigned)g.ncls);
#define KPX_LAUNCH(bm, bn, wm, wn) \
    hipLaunchKernelGGL((conv_igemm_kernel<bm, bn, wm, wn, BT, VEC, MERGE, TAIL>), nblk, dim3((wm) * (wn) * 64), 0, s, g)
    if (BM == 128 && BN == 128) KPX_LAUNCH(128, 128, 2, 4);        // 8 waves of 64x32
    else if (BM == 64 && BN == 128) KPX_LAUNCH(64, 128, 2, 4);     // 8 waves of 32x32 (small M, wide N)
    else if (BM == 128 && BN == 64) KPX_LAUNCH(128, 64, 4, 2);     // 8 waves of 32x32
    else if (BM == 64 && BN == 64) KPX_LAUNCH(64, 64, 2, 2);       // 4 waves of 32x32
    else KPX_LAUNCH(128, 32, 4, 1);                                // 4 waves of 32x32
#undef KPX_LAUNCH
    return kpx_launch_status();
}

// conv_gemm3.hip first: the same gather convolution on the bf16 matrix pipe with fp32 operands split into three bf16 terms (fp32-equivalent)
template <bool BT>
static int launch_gather_conv(const ConvGeom& g, hipStream_t s) {
    if (kpx_gemm3_eligible(&g)) {
        int rc = kpx_gemm3_launch(g, BT ? 1 : 0, g.terms == 1 ? 1 : 3, s);
        return rc || g.ksplit <= 1 ? rc : launch_splitk_reduce(g, s);
    }
    if (g.io16) return KPX_EINVAL;                       // bf16 tensors: only the kernel above reads them
    if (g.merge) return launch_gather_conv_v<false, false, true, true>(g, s);
    if (g.vecA && g.vecB) {
        if (g.Cin % 4 == 0 && g.Cout % 4 == 0) return launch_gather_conv_v<BT, true, false, false>(g, s);
        return launch_gather_conv_v<BT, true, false, true>(g, s);
    }
    return launch_gather_conv_v<BT, false, false, true>(g, s);
}

// Tiny-Cout / long-K forward (img_discr D_logit: 3x3x2048 -> 1, reference networks/__init__.py:150): one wavefront
// per output pixel, lanes stride over the contiguous channel axis, shuffle-tree reduction.  An MFMA tile would idle
// 31/32 of its columns and serialise 18432-deep K loops on a handful of workgroups.
__global__ __launch_bounds__(256) void conv_small_cout_kernel(const ConvGeom g) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= g.M) return;
    const int HW = g.Ha * g.Wa;
    const int n = m / HW, rem = m - n * HW, a = rem / g.Wa, b = rem - a * g.Wa;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int tr = 0; tr < g.Tr; ++tr) {
        const int ih = a * g.isy + g.iy0 + tr * g.ity;
        if ((unsigned)ih >= (unsigned)g.Hi) continue;
        for (int tq = 0; tq < g.Tq; ++tq) {
            const int iw = b * g.isx + g.ix0 + tq * g.itx;
            if ((unsigned)iw >= (unsigned)g.Wi) continue;
            const float* xp = g.x + ((size_t)(n * g.Hi + ih) * g.Wi + iw) * g.ldx;
            const float* wp = g.w + (size_t)((g.wr0 + tr * g.wrs) * g.KW + g.wq0 + tq * g.wqs) * g.wts;
            for (int c = lane * 4; c < g.Cin; c += 256) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + c);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    for (int o = 0; o < g.Cout; ++o) acc[o] = fmaf(xv[j], wp[(size_t)(c + j) * g.ldw + o], acc[o]);
            }
        }
    }
    const int pix = (n * g.Ho + a * g.osy + g.oy0) * g.Wo + b * g.osx + g.ox0;
    for (int o = 0; o < g.Cout; ++o) {
        float v = kpx_wave_sum(acc[o]);
        if (lane == 0) {
            v += g.bias ? g.bias[o] : 0.f;
            if (g.act == KPX_ACT_RELU) v = fmaxf(v, 0.f);
            else if (g.act == KPX_ACT_LRELU) v = v > 0.f ? v : 0.01f * v;
            else if (g.act == KPX_ACT_TANH) v = tanhf(v);
            g.y[(size_t)pix * g.ldy + o] = v;
        }
    }
}
static int launch_small_cout(ConvGeom g, hipStream_t s) {
    g.M = g.N * g.Ha * g.Wa;
    hipLaunchKernelGGL(conv_small_cout_kernel, dim3((unsigned)((g.M + 3) / 4)), dim3(256), 0, s, g);
    return kpx_launch_status();
}

static int dgrad_splitk_plan(int N, int Hi, int Wi, int Cin, int Cout, int KH, int KW, int stride) {
    const long Mcls = (long)N * ((Hi + stride - 1) / stride) * ((Wi + stride - 1) / stride);      // largest parity class
    const long chunks = (long)(KH / stride > 0 ? KH / stride : 1) * (KW / stride > 0 ? KW / stride : 1) * ((Cout + 31) / 32);   // smallest class
    if (Cin % 4 != 0) return 1;
    int S = conv_splitk_plan(Mcls * stride * stride, Cin, chunks);   // tiles are counted over all classes of the launch
    return S;
}

static inline size_t wino_ws_bytes(int Cin, int Cout) {          // U[16][K padded to 8][Nn padded to 32] for either direction
    const size_t a = (size_t)((Cin + 7) & ~7) * ((Cout + 31) & ~31), b = (size_t)((Cout + 7) & ~7) * ((Cin + 31) & ~31);
    return 16 * 4 * (a > b ? a : b);
}

extern "C" size_t kpx_conv2d_fwd_workspace_bytes(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW) {
    if (Cin % 4 != 0) return 0;
    const int S = conv_splitk_plan((long)N * Ho * Wo, Cout, (long)KH * KW * ((Cin + 31) / 32));
    size_t b = S > 1 ? (size_t)S * N * Ho * Wo * Cout * 4 : 0;
    if (KH == 3 && KW == 3 && b < wino_ws_bytes(Cin, Cout)) b = wino_ws_bytes(Cin, Cout);     // stride unknown here: upper bound
    return b;
}

extern "C" size_t kpx_conv2d_dgrad_workspace_bytes(int N, int Hi, int Wi, int Cin, int Cout, int KH, int KW, int stride) {
    const int S = dgrad_splitk_plan(N, Hi, Wi, Cin, Cout, KH, KW, stride);
    size_t b = S > 1 ? (size_t)S * N * Hi * Wi * Cin * 4 : 0;
    if (KH == 3 && KW == 3 && stride == 1 && b < wino_ws_bytes(Cin, Cout)) b = wino_ws_bytes(Cin, Cout);
    return b;
}

static int fwd_impl(const float* x, int N, int Hi, int Wi, int Cin, int ldx, const float* w, int KH, int KW, const float* bias,
                    float* y, int Ho, int Wo, int Cout, int ldy, int stride, int pad_t, int pad_l, int act, int arith, int io16,
                    void* workspace, size_t workspace_bytes, void* stream);
extern "C" int kpx_conv2d_fwd_f32(const float* x, int N, int Hi, int Wi, int Cin, int ldx,
                                  const float* w, int KH, int KW, const float* bias,
                                  float* y, int Ho, int Wo, int Cout, int ldy,
                                  int stride, int pad_t, int pad_l, int act, int arith, void* workspace, size_t workspace_bytes, void* stream) {
    return fwd_impl(x, N, Hi, Wi, Cin, ldx, w, KH, KW, bias, y, Ho, Wo, Cout, ldy, stride, pad_t, pad_l, act, arith, 0, workspace, workspace_bytes, stream);
}
// bf16 configuration: x bf16 (pixel stride ldx elements, a multiple of 8), y bf16 (y_f32 = 0) or fp32; only shapes the bf16-pipe gather kernel
// takes (KPX_EINVAL otherwise: the caller converts and uses the fp32 entry)
extern "C" int kpx_conv2d_fwd_bf16(const void* x, int N, int Hi, int Wi, int Cin, int ldx, const float* w, int KH, int KW, const float* bias,
                                   void* y, int y_f32, int Ho, int Wo, int Cout, int ldy, int stride, int pad_t, int pad_l, int act,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (ldx % 8 || !kpx_aligned16(x) || !kpx_aligned16(y) || (!y_f32 && ldy % 4)) return KPX_EINVAL;
    return fwd_impl((const float*)x, N, Hi, Wi, Cin, ldx, w, KH, KW, bias, (float*)y, Ho, Wo, Cout, ldy, stride, pad_t, pad_l, act, KPX_ARITH_BF16, 1 | (y_f32 ? 0 : 2),
                    workspace, workspace_bytes, stream);
}
static int fwd_impl(const float* x, int N, int Hi, int Wi, int Cin, int ldx, const float* w, int KH, int KW, const float* bias,
                    float* y, int Ho, int Wo, int Cout, int ldy, int stride, int pad_t, int pad_l, int act, int arith, int io16,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !y || N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 ||
        KH <= 0 || KW <= 0 || stride <= 0 || ldx < Cin || ldy < Cout || act < 0 || act > 3 || arith < 0 || arith > 1)
        return KPX_EINVAL;
    if (io16) goto gather;                               // bf16 tensors: the specialised fp32 kernels below do not read them
    if (KH == 3 && KW == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && Ho == Hi && Wo == Wi && act != KPX_ACT_TANH &&
        kpx_conv3x3_c16_eligible(N, Hi, Wi, Cin, Cout, ldx, ldy, x))                 // exactly 16 produced channels: 16x16x4 MFMA blocks (conv_c16.hip)
        return kpx_conv3x3_c16_f32(x, N, Hi, Wi, Cin, ldx, w, 0, bias, y, ldy, act, nullptr, stream);
    if (Cout <= 4 && Cin <= 128 && (size_t)N * Ho * Wo >= 65536) {            // few produced channels over a large image: VALU kernel (conv_rgb.hip)
        const int rc = kpx_conv_few_fwd(x, N, Hi, Wi, Cin, ldx, w, KH, KW, bias, y, Ho, Wo, Cout, ldy, stride, pad_t, pad_l, act, kpx_stream(stream));
        if (rc != -2) return rc;
    }
    if (KH == 3 && KW == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && Ho == Hi && Wo == Wi && act != KPX_ACT_TANH && kpx_aligned16(w) &&
        workspace && workspace_bytes >= wino_ws_bytes(Cin, Cout) && kpx_wino_eligible(N, Hi, Wi, Cin, Cout, ldx, x))
        return kpx_wino_conv3x3(x, N, Hi, Wi, Cin, ldx, w, Cin, Cout, 0, bias, act, y, Cout, ldy, (float*)workspace, kpx_stream(stream));
    if (Cin <= 4 && ldx == Cin && stride <= 2 && Cout <= 64 && Ho * Wo >= 256) {       // image-input layers (stride 2: img_discr conv_0): patch + filter resident in LDS
        const int rc = kpx_conv_rgb_fwd(x, N, Hi, Wi, Cin, w, KH, KW, bias, y, Ho, Wo, Cout, ldy, stride, pad_t, pad_l, act, kpx_stream(stream));
        if (rc != -2) return rc;
    }
gather:
    ConvGeom g{};
    g.x = x; g.y = y; g.w = w; g.bias = bias; g.io16 = io16;
    g.N = N; g.Hi = Hi; g.Wi = Wi; g.Cin = Cin; g.ldx = ldx;
    g.Ho = Ho; g.Wo = Wo; g.Cout = Cout; g.ldy = ldy;
    g.Ha = Ho; g.Wa = Wo; g.osy = 1; g.oy0 = 0; g.osx = 1; g.ox0 = 0;
    g.isy = stride; g.iy0 = -pad_t; g.isx = stride; g.ix0 = -pad_l;
    g.Tr = KH; g.Tq = KW; g.ity = 1; g.itx = 1;
    g.wr0 = 0; g.wrs = 1; g.wq0 = 0; g.wqs = 1; g.KW = KW;
    g.wts = Cin * Cout; g.ldw = Cout; g.act = act; g.terms = arith == KPX_ARITH_BF16 ? 1 : 3;
    g.vecA = (ldx % 4 == 0) && kpx_aligned16(x);
    g.vecB = (Cout % 4 == 0) && kpx_aligned16(w);
    if (Cin % 4 != 0 && ldx == Cin && KW > 1 && KW * Cin <= 64) {      // image inputs (Cin = 3): merge each filter row
        g.merge = Cin; g.Tq = 1; g.KW = 1; g.Cin = KW * Cin; g.wts = KW * Cin * Cout; g.vecA = 0;
    }
    if (io16 && !kpx_gemm3_eligible(&g)) return KPX_EINVAL;
    if (!io16 && Cout <= 4 && Cin % 4 == 0 && Cin >= 256 && g.vecA && g.vecB == (Cout == 4))
        return launch_small_cout(g, kpx_stream(stream));
    if (g.vecA && g.vecB && !g.merge && Cin % 4 == 0) {        // small-M / long-K layers (the discriminator's 10x10 .. 4x4 maps): split K over workgroups
        const int S = conv_splitk_plan((long)N * Ho * Wo, Cout, (long)KH * KW * ((Cin + 31) / 32));
        g.ws_slab = (size_t)N * Ho * Wo * Cout;
        if (S > 1 && workspace && workspace_bytes >= (size_t)S * g.ws_slab * 4) { g.ksplit = S; g.ws = (float*)workspace; }
    }
    return launch_gather_conv<false>(g, kpx_stream(stream));
}

// dx = dgrad(dy) [* act_in'(y_in)]: the optional factor is the activation backward of the tensor dx is the gradient of (y_in = its ACTIVATED
// value, same shape as dx).  Fused into the epilogue where the layer runs on the gather kernels; a second pass over dx otherwise.
static int dgrad_impl(const float* dy, int N, int Ho, int Wo, int Cout, int lddy, const float* w, int KH, int KW,
                      float* dx, int Hi, int Wi, int Cin, int lddx, int stride, int pad_t, int pad_l, int arith,
                      const float* y_in, int ld_y_in, int act_in, void* workspace, size_t workspace_bytes, void* stream, int io16 = 0);

extern "C" int kpx_conv2d_dgrad_f32(const float* dy, int N, int Ho, int Wo, int Cout, int lddy,
                                    const float* w, int KH, int KW,
                                    float* dx, int Hi, int Wi, int Cin, int lddx,
                                    int stride, int pad_t, int pad_l, int arith, void* workspace, size_t workspace_bytes, void* stream) {
    return dgrad_impl(dy, N, Ho, Wo, Cout, lddy, w, KH, KW, dx, Hi, Wi, Cin, lddx, stride, pad_t, pad_l, arith, nullptr, 0, KPX_ACT_NONE,
                      workspace, workspace_bytes, stream);
}

extern "C" int kpx_conv2d_dgrad_act_f32(const float* dy, int N, int Ho, int Wo, int Cout, int lddy,
                                        const float* w, int KH, int KW,
                                        float* dx, int Hi, int Wi, int Cin, int lddx,
                                        int stride, int pad_t, int pad_l, int arith,
                                        const float* y_in, int ld_y_in, int act_in, void* workspace, size_t workspace_bytes, void* stream) {
    if (!y_in || ld_y_in < Cin || (act_in != KPX_ACT_RELU && act_in != KPX_ACT_LRELU)) return KPX_EINVAL;
    return dgrad_impl(dy, N, Ho, Wo, Cout, lddy, w, KH, KW, dx, Hi, Wi, Cin, lddx, stride, pad_t, pad_l, arith, y_in, ld_y_in, act_in,
                      workspace, workspace_bytes, stream);
}

// bf16 configuration, image-input layers (the images stay fp32; what the layer produces / receives is bf16).  KPX_EINVAL for shapes the
// LDS-resident image kernels (conv_rgb.hip) do not take: the caller then converts and uses the fp32 entries.  (Their weight gradient,
// kpx_conv_image_wgrad_bf16, is in conv_wgrad.hip.)
//   forward:  x fp32 [N, Hi, Wi, Cin <= 4] contiguous -> y bf16 (pixel stride ldy elements)
extern "C" int kpx_conv_image_fwd_bf16(const float* x, int N, int Hi, int Wi, int Cin, const float* w, int KH, int KW, const float* bias,
                                       void* y, int Ho, int Wo, int Cout, int ldy, int stride, int pad_t, int pad_l, int act, void* stream) {
    if (!x || !w || !y || N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cin > 4 || Cout <= 0 || Cout > 64 || Ho * Wo < 256 || stride < 1 || stride > 2 ||
        ldy < Cout || act < 0 || act > 3)
        return KPX_EINVAL;
    const int rc = kpx_conv_rgb_fwd(x, N, Hi, Wi, Cin, w, KH, KW, bias, (float*)y, Ho, Wo, Cout, ldy, stride, pad_t, pad_l, act, kpx_stream(stream), 1);
    return rc == -2 ? KPX_EINVAL : rc;
}
//   data gradient:  dy bf16 (pixel stride lddy elements, a multiple of 8) -> dx fp32 [N, Hi, Wi, Cin] (pixel stride lddx)
extern "C" int kpx_conv_image_dgrad_bf16(const void* dy, int N, int Ho, int Wo, int Cout, int lddy, const float* w, int KH, int KW,
                                         float* dx, int Hi, int Wi, int Cin, int lddx, int stride, int pad_t, int pad_l, void* stream) {
    if (!dy || !w || !dx || N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cin > 4 || Cout <= 0 || Ho <= 0 || Wo <= 0 || lddy < Cout || lddx < Cin)
        return KPX_EINVAL;
    const int rc = kpx_conv_rgb_dgrad((const float*)dy, N, Ho, Wo, Cout, lddy, w, KH, KW, dx, Hi, Wi, Cin, lddx, stride, pad_t, pad_l, kpx_stream(stream), 1);
    return rc == -2 ? KPX_EINVAL : rc;
}

// bf16 configuration: dy bf16, dx bf16 (dx_f32 = 0) or fp32 (the gradient towards an fp32 tensor); y_in (optional, with act_in): the bf16
// ACTIVATED tensor dx is the gradient of -- its activation backward is applied in the epilogue.  KPX_EINVAL for shapes the bf16-pipe gather
// kernel does not take.
extern "C" int kpx_conv2d_dgrad_bf16(const void* dy, int N, int Ho, int Wo, int Cout, int lddy, const float* w, int KH, int KW,
                                     void* dx, int dx_f32, int Hi, int Wi, int Cin, int lddx, int stride, int pad_t, int pad_l,
                                     const void* y_in, int ld_y_in, int act_in, void* workspace, size_t workspace_bytes, void* stream) {
    if (lddy % 8 || !kpx_aligned16(dy) || !kpx_aligned16(dx) || (!dx_f32 && lddx % 4)) return KPX_EINVAL;
    if (y_in && (ld_y_in < Cin || (act_in != KPX_ACT_RELU && act_in != KPX_ACT_LRELU))) return KPX_EINVAL;
    return dgrad_impl((const float*)dy, N, Ho, Wo, Cout, lddy, w, KH, KW, (float*)dx, Hi, Wi, Cin, lddx, stride, pad_t, pad_l, KPX_ARITH_BF16,
                      (const float*)y_in, ld_y_in, y_in ? act_in : KPX_ACT_NONE, workspace, workspace_bytes, stream, 1 | (dx_f32 ? 0 : 2) | (y_in ? 4 : 0));
}

// the specialised data-gradient kernels have no factor in their epilogues: one pass over dx afterwards (contiguous tensors only)
static int dgrad_act_pass(int rc, float* dx, int N, int Hi, int Wi, int Cin, int lddx, const float* y_in, int ld_y_in, int act_in, void* stream) {
    if (rc || !y_in) return rc;
    if (lddx != Cin || ld_y_in != Cin) return KPX_EINVAL;
    return kpx_act_bwd_f32(dx, y_in, dx, (size_t)N * Hi * Wi * Cin, act_in, stream);
}

static int dgrad_impl(const float* dy, int N, int Ho, int Wo, int Cout, int lddy, const float* w, int KH, int KW,
                      float* dx, int Hi, int Wi, int Cin, int lddx, int stride, int pad_t, int pad_l, int arith,
                      const float* y_in, int ld_y_in, int act_in, void* workspace, size_t workspace_bytes, void* stream, int io16) {
    if (!dy || !w || !dx || N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 ||
        KH <= 0 || KW <= 0 || stride <= 0 || lddy < Cout || lddx < Cin || arith < 0 || arith > 1)
        return KPX_EINVAL;
    if (stride > 2) return KPX_EINVAL;             // at most 4 parity classes per launch (the path has strides 1 and 2)
    if (io16) goto gather;                         // bf16 tensors: only the bf16-pipe gather kernel reads them
    if (KH == 3 && KW == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && Ho == Hi && Wo == Wi &&
        kpx_conv3x3_c16_eligible(N, Hi, Wi, Cout, Cin, lddy, lddx, dy))
        return dgrad_act_pass(kpx_conv3x3_c16_f32(dy, N, Hi, Wi, Cout, lddy, w, 1, nullptr, dx, lddx, KPX_ACT_NONE, nullptr, stream),
                              dx, N, Hi, Wi, Cin, lddx, y_in, ld_y_in, act_in, stream);
    if (Cin <= 4) {                                // gradient towards an image: VALU kernel (conv_rgb.hip)
        const int rc = kpx_conv_rgb_dgrad(dy, N, Ho, Wo, Cout, lddy, w, KH, KW, dx, Hi, Wi, Cin, lddx, stride, pad_t, pad_l, kpx_stream(stream));
        if (rc != -2) return dgrad_act_pass(rc, dx, N, Hi, Wi, Cin, lddx, y_in, ld_y_in, act_in, stream);
    }
    if (KH == 3 && KW == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && Ho == Hi && Wo == Wi &&
        workspace && workspace_bytes >= wino_ws_bytes(Cin, Cout) && kpx_wino_eligible(N, Hi, Wi, Cout, Cin, lddy, dy))
        return dgrad_act_pass(kpx_wino_conv3x3(dy, N, Hi, Wi, Cout, lddy, w, Cin, Cout, 1, nullptr, KPX_ACT_NONE, dx, Cin, lddx, (float*)workspace, kpx_stream(stream)),
                              dx, N, Hi, Wi, Cin, lddx, y_in, ld_y_in, act_in, stream);
gather:
    ConvGeom g{};
    g.x = dy; g.y = dx; g.w = w; g.bias = nullptr; g.io16 = io16;
    g.mul_y = y_in; g.ld_mul = ld_y_in; g.mul_act = act_in;
    g.N = N; g.Hi = Ho; g.Wi = Wo; g.Cin = Cout; g.ldx = lddy;       // "input" of the gather = dy
    g.Ho = Hi; g.Wo = Wi; g.Cout = Cin; g.ldy = lddx;                // "output" = dx
    g.osy = stride; g.osx = stride;
    g.isy = 1; g.ity = -1; g.isx = 1; g.itx = -1;
    g.wrs = stride; g.wqs = stride; g.KW = KW;
    g.wts = Cin * Cout; g.ldw = Cout; g.act = KPX_ACT_NONE; g.terms = arith == KPX_ARITH_BF16 ? 1 : 3;
    g.vecA = (lddy % 4 == 0) && kpx_aligned16(dy);
    g.vecB = (Cout % 4 == 0) && kpx_aligned16(w);
    g.ncls = 0;
    for (int ph = 0; ph < stride; ++ph) {
        for (int pw = 0; pw < stride; ++pw) {
            if (ph >= Hi || pw >= Wi) continue;
            ConvClass c{};
            c.Ha = (Hi - ph + stride - 1) / stride; c.Wa = (Wi - pw + stride - 1) / stride;
            c.oy0 = ph; c.ox0 = pw;
            const int r0 = (ph + pad_t) % stride, q0 = (pw + pad_l) % stride;
            c.Tr = r0 < KH ? (KH - r0 + stride - 1) / stride : 0;
            c.Tq = q0 < KW ? (KW - q0 + stride - 1) / stride : 0;
            if (c.Tr == 0 || c.Tq == 0) { c.Tr = 0; c.Tq = 0; }
            c.iy0 = (ph + pad_t - r0) / stride;
            c.ix0 = (pw + pad_l - q0) / stride;
            c.wr0 = r0; c.wq0 = q0;
            g.cls[g.ncls++] = c;
        }
    }
    if (io16 && !kpx_gemm3_eligible(&g)) return KPX_EINVAL;
    if (g.vecA && g.vecB && Cout % 4 == 0) {
        const int S = dgrad_splitk_plan(N, Hi, Wi, Cin, Cout, KH, KW, stride);
        g.ws_slab = (size_t)N * Hi * Wi * Cin;
        if (S > 1 && workspace && workspace_bytes >= (size_t)S * g.ws_slab * 4) { g.ksplit = S; g.ws = (float*)workspace; }
    }
    return launch_gather_conv<true>(g, kpx_stream(stream));
}
