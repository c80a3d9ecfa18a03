"""CPU: the C-ABI library loads and exports every symbol include/kpx.h declares, with matching arity in the ctypes table."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _header_functions():
    src = open(os.path.join(REPO, 'include', 'kpx.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(int|size_t)\s+(kpx_\w+)\s*\(([^;]*?)\)\s*;', src, flags=re.S):
        args = m.group(3).strip()
        out[m.group(2)] = 0 if args in ('', 'void') else args.count(',') + 1
    return out


def test_library_exports_every_declared_symbol():
    import kpx_amd  # noqa: F401  (fails loudly if the .so is missing)
    from kpx_amd import _lib
    decl = _header_functions()
    assert len(decl) >= 30
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in decl.items():
        assert hasattr(lib, name), 'missing export %s' % name
        assert name in _lib.SIGNATURES, 'no ctypes signature for %s' % name
        assert len(_lib.SIGNATURES[name][1]) == nargs, (name, len(_lib.SIGNATURES[name][1]), nargs)
    assert set(_lib.SIGNATURES) == set(decl)
    header_version = int(re.search(r'#define\s+KPX_ABI_VERSION\s+(\d+)', open(os.path.join(REPO, 'include', 'kpx.h')).read()).group(1))
    assert lib.kpx_abi_version() == header_version == _lib.ABI_VERSION          # header, library and ctypes table agree


def test_bad_arguments_are_rejected_without_a_gpu():
    from kpx_amd._lib import lib
    assert lib.kpx_conv2d_fwd_f32(None, 1, 8, 8, 4, 4, None, 3, 3, None, None, 8, 8, 4, 4, 1, 1, 1, 0, 0, None, 0, None) == -1
    # the batch-norm train entries (groups = 1: the single call) refuse a null x / dy before any device call
    a = 1 << 20                                                 # an aligned fake address
    assert lib.kpx_bn_train_fwd_f32(None, 64, 1, 8, 8, None, 0, 1e-5, a, a, a, a, None, None, 0.999, a, 8, 1, a, None) == -1
    assert lib.kpx_bn_train_fwd_bf16(None, 64, 1, 8, 8, None, 0, 1e-5, a, a, a, a, None, None, 0.999, a, 8, 0, 1, a, None) == -1
    assert lib.kpx_bn_train_bwd_f32(None, 8, a, 8, 64, 1, 8, a, a, a, a, 1, a, 8, a, a, 0, None, 0, a, None) == -1
    assert lib.kpx_bn_train_bwd_bf16(None, 8, 0, a, 8, 64, 1, 8, a, a, a, a, 1, a, 8, a, a, 0, None, 0, a, None) == -1
    assert lib.kpx_conv2d_wgrad_workspace_bytes(32, 128, 128, 64, 64, 3, 3) > 0
    assert lib.kpx_conv2d_wgrad_workspace_bytes(1, 4, 4, 1024, 2048, 4, 4) == 0
    # per-call arithmetic selector and the activation-backward factor: range-checked before anything touches a device
    assert lib.kpx_conv2d_fwd_f32(1, 1, 8, 8, 4, 4, 1, 3, 3, None, 1, 8, 8, 4, 4, 1, 1, 1, 0, 2, None, 0, None) == -1           # arith = 2
    assert lib.kpx_conv2d_dgrad_act_f32(1, 1, 8, 8, 4, 4, 1, 3, 3, 1, 8, 8, 4, 4, 1, 1, 1, 0, None, 4, 2, None, 0, None) == -1   # y_in = NULL
    assert lib.kpx_conv2d_dgrad_act_f32(1, 1, 8, 8, 4, 4, 1, 3, 3, 1, 8, 8, 4, 4, 1, 1, 1, 0, 1, 4, 3, None, 0, None) == -1      # tanh: not an epilogue factor
    # the two F(4x4,3x3) entries share their arguments and option rules: both refuse the same mixes before any device call
    for entry in (lib.kpx_conv3x3_wino43_f32, lib.kpx_conv3x3_wino43b_f32):
        def f43(n=2, h=32, w=32, nn=64, bias=None, act=0, mask=None, pool=None, stats=None, bn_y=None, bn_beta=None):
            return entry(a, n, h, w, 64, 64, a, bias, a, nn, nn, act, mask, nn, pool, nn, stats, bn_y, nn, bn_beta, None)
        assert f43(bn_y=a, bn_beta=a) == -1                     # bn_y without tile_stats
        assert f43(stats=a, bn_y=a) == -1                       # bn_y without bn_beta
        assert f43(stats=a, bn_y=a, bn_beta=a, bias=a) == -1    # the bn form takes no bias ...
        assert f43(stats=a, bn_y=a, bn_beta=a, act=1) == -1     # ... and no activation
        assert f43(mask=a, stats=a) == -1                       # mask_y with tile_stats
        assert f43(h=33, pool=a) == -1                          # pool_y with odd H
        assert f43(nn=96, pool=a) == -1                         # mask / pool need Nn % 64 == 0
        assert f43(h=16, w=16, stats=a) == -1                   # packed 16 x 16 images: no statistics strips
    # F(2x2,3x3): statistics need whole 16 x 16 tiles (8 x 8 images are packed four to a workgroup); the bn form needs tile_stats
    assert lib.kpx_conv3x3_wino_f32(a, 4, 8, 8, 16, 16, a, None, a, 32, 32, 0, a, None, 0, None, None) == -1
    assert lib.kpx_conv3x3_wino_f32(a, 2, 32, 32, 16, 16, a, None, a, 32, 32, 0, None, a, 32, a, None) == -1


def test_keypoint_head_fold_eligibility_is_a_host_question():
    """networks.pose_encoder asks kpx_keypoint_head_proj_eligible before choosing the folded 1x1 + key-point head operator; a shape outside
    the operator's limits (channels, key-points, profile rows within 64 KB of LDS) takes the conv + head pair instead of failing in the launch."""
    from kpx_amd._lib import lib
    assert lib.kpx_keypoint_head_proj_eligible(64, 128, 128, 16, 15) == 1 and lib.kpx_keypoint_head_proj_eligible(32, 256, 256, 16, 40) == 1
    assert lib.kpx_keypoint_head_proj_eligible(2, 128, 128, 18, 15) == 0        # C % 4
    assert lib.kpx_keypoint_head_proj_eligible(2, 128, 128, 512, 15) == 0       # C > 256
    assert lib.kpx_keypoint_head_proj_eligible(2, 1024, 1024, 16, 15) == 0      # image side > 512
    assert lib.kpx_keypoint_head_proj_eligible(2, 128, 128, 16, 100) == 0       # K > 64


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    with pytest.raises(KpxError):
        ops.conv2d(torch.zeros(1, 4, 4, 4), torch.zeros(3, 3, 4, 4))
