// Option rules of the two F(4x4,3x3) entries, kpx_conv3x3_wino43_f32 (conv_wino43.hip) and kpx_conv3x3_wino43b_f32 (conv_wino43b.hip):
// the same arguments, the same rules, different kernels.  Shape eligibility is each kernel's own (kpx_conv3x3_wino43(b)_eligible).
//   tile_stats alone: batch-norm sums of the output per 4 x 16-pixel strip (none for packed 16 x 16 images);
//   tile_stats + bn_y + bn_beta: data gradient towards bn_y = relu(batch norm)'s output, masked, with that batch norm's backward sums
//     (no bias / act);
//   mask_y / pool_y: VGG19's fused ReLU backward / 2x2 max-pool (no tile_stats).
// The bn and mask / pool forms need Nn % 64 == 0 and 16-B aligned rows everywhere.
#pragma once
#include "kpx_bf16.h"

static inline bool wino43_options_valid(const float* in, int H, int W, int K, int ldin, const void* U, const float* bias,
                                        const float* out, int Nn, int ldout, int act, const float* mask_y, int ld_mask,
                                        const float* pool_y, int ld_pool, const float* tile_stats, const float* bn_y, int ld_bn_y,
                                        const float* bn_beta) {
    if (!in || !U || !out || ldin < K || ldout < Nn || act < 0 || act > 2) return false;
    if (tile_stats && W == 16) return false;             // packed 16 x 16 images: kpx_conv3x3_wino43_stats_tiles is 0 for them
    const bool out_rows = Nn % 64 == 0 && ldout % 4 == 0 && kpx_aligned16(out);
    if (bn_y || bn_beta)
        return tile_stats && bn_y && bn_beta && !mask_y && !pool_y && !bias && act == KPX_ACT_NONE && out_rows &&
               ld_bn_y % 4 == 0 && ld_bn_y >= Nn && kpx_aligned16(bn_y) && kpx_aligned16(bn_beta);
    if (mask_y || pool_y)
        return !tile_stats && out_rows && (!mask_y || (ld_mask % 4 == 0 && ld_mask >= Nn && kpx_aligned16(mask_y))) &&
               (!pool_y || (ld_pool % 4 == 0 && ld_pool >= Nn && kpx_aligned16(pool_y) && H % 2 == 0 && W % 2 == 0));
    return true;
}
