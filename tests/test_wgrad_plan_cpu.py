"""CPU: the plan of the fp32 weight gradient (csrc/conv_wgrad.hip: wgrad_plan) seen through its two host queries,
kpx_conv2d_wgrad_plan and kpx_conv2d_wgrad_workspace_bytes.  No device call anywhere: pointers are fake addresses, as in test_abi.py."""
import itertools
import json
import os
import re

import pytest

from kpx_amd import _lib
from kpx_amd._lib import lib
from kpx_amd.ops import same_pad

HERE = os.path.dirname(os.path.abspath(__file__))
A = 1 << 20                                                     # an aligned fake address
# enum KpxWgradFamily, read from include/kpx.h so that no second copy of its order can drift
HEADER = open(os.path.join(HERE, '..', 'include', 'kpx.h')).read()
FAMILIES = tuple(re.findall(r'KPX_WGRAD_(\w+)', HEADER[HEADER.index('enum KpxWgradFamily {'):].split('}')[0]))

GRID_N, GRID_HW = (1, 2, 16, 64), (4, 8, 16, 32, 64, 128)
GRID_CIN, GRID_COUT, GRID_K = (3, 16, 24, 32, 64, 130, 158, 256, 512), (1, 4, 15, 16, 32, 64, 160, 512), (1, 3, 4, 7)


def conv_cases():
    from test_ops_gpu import CONV_CASES                   # plain data; importing a gpu-marked module is harmless here
    return CONV_CASES


def case_geometry(n, h, w, cin, cout, k, s, pad):
    """The weight-gradient call ops.conv2d makes for a CONV_CASES row: (N, Hi, Wi, Cin, Ho, Wo, Cout, K, stride, pad_t, pad_l)."""
    pt, _, ho = same_pad(h + 2 * pad, k, s)
    pl, _, wo = same_pad(w + 2 * pad, k, s)
    return n, h, w, cin, ho, wo, cout, k, s, pad + pt, pad + pl


def query_points():
    """(N, Ho, Wo, Cin, Cout, K) of the workspace query: every CONV_CASES row, then the grid."""
    pts = []
    for row in conv_cases():
        n, _, _, cin, ho, wo, cout, k, _, _, _ = case_geometry(*row[:8])
        pts.append((n, ho, wo, cin, cout, k))
    pts += [(n, hw, hw, cin, cout, k) for n, hw, cin, cout, k in itertools.product(GRID_N, GRID_HW, GRID_CIN, GRID_COUT, GRID_K)]
    return pts


def query(n, ho, wo, cin, cout, k):
    return lib.kpx_conv2d_wgrad_workspace_bytes(n, ho, wo, cin, cout, k, k)


def plan(n, hi, wi, cin, ldx, ho, wo, cout, lddy, k, stride, pad_t, pad_l, arith=0, x=A, dy=A):
    """(family name, splits, workspace bytes) of the fp32 entry's plan."""
    import ctypes
    fam, s, nbytes = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_size_t(0)
    rc = lib.kpx_conv2d_wgrad_plan(x, n, hi, wi, cin, ldx, dy, ho, wo, cout, lddy, k, k, stride, pad_t, pad_l, arith,
                                   ctypes.byref(fam), ctypes.byref(s), ctypes.byref(nbytes))
    assert rc == 0, rc
    return FAMILIES[fam.value], s.value, nbytes.value


def case_plan(row, arith=0):
    n, hi, wi, cin, ho, wo, cout, k, s, pad_t, pad_l = case_geometry(*row[:8])
    return plan(n, hi, wi, cin, cin, ho, wo, cout, cout, k, s, pad_t, pad_l, arith)


def test_workspace_query_is_the_one_recorded_before_the_plan():
    """kpx_conv2d_wgrad_workspace_bytes on the fixed grid against golden/wgrad_workspace_parent.json, recorded from the library as it was
    when the query re-derived every family's split plan by hand."""
    doc = json.load(open(os.path.join(HERE, 'golden', 'wgrad_workspace_parent.json')))
    g = doc['grid']
    assert (tuple(g['N']), tuple(g['HW']), tuple(g['Cin']), tuple(g['Cout']), tuple(g['K'])) == (GRID_N, GRID_HW, GRID_CIN, GRID_COUT, GRID_K)
    pts = [tuple(c[:6]) for c in doc['cases']]
    pts += [(n, hw, hw, cin, cout, k) for n, hw, cin, cout, k in itertools.product(GRID_N, GRID_HW, GRID_CIN, GRID_COUT, GRID_K)]
    want = [c[6] for c in doc['cases']] + g['bytes']
    assert len(pts) == len(want) == len(doc['cases']) + len(GRID_N) * len(GRID_HW) * len(GRID_CIN) * len(GRID_COUT) * len(GRID_K)
    diff = [(p, query(*p), w) for p, w in zip(pts, want) if query(*p) != w]
    assert not diff, '%d of %d points differ, first (point, now, recorded): %s' % (len(diff), len(pts), diff[:8])


def test_workspace_query_covers_every_plan():
    """Whatever the stride, padding, pixel strides, alignment and arithmetic of a call, its plan needs no more than the query answers
    for the shape: a caller that sizes its workspace with the query (ops.conv_wgrad_raw) is never refused."""
    r8 = lambda c: (c + 7) & ~7
    worst = []
    for n, hw, cin, cout, k in itertools.product(GRID_N, GRID_HW, GRID_CIN, GRID_COUT, (3, 4, 7)):
        have = query(n, hw, hw, cin, cout, k)
        for stride, pad, ldx, lddy, off, arith in itertools.product((1, 2), (0, 1), (cin, r8(cin), cin + 16), (cout, r8(cout), cout + 16), (0, 4), (0, 1)):
            fam, s, need = plan(n, hw * stride, hw * stride, cin, ldx, hw, hw, cout, lddy, k, stride, pad, pad, arith, A + off, A + off)
            if need > have:
                worst.append(((n, hw, cin, cout, k, stride, pad, ldx, lddy, off, arith), fam, s, need, have))
    # the CONV_CASES rows as ops.conv2d calls them: their Hi is not always Ho * stride (Ho = 65 from Hi = 128), which the tiny-filter plan sees
    for row, arith in itertools.product(conv_cases(), (0, 1)):
        n, _, _, cin, ho, wo, cout, k, _, _, _ = case_geometry(*row[:8])
        fam, s, need = case_plan(row, arith)
        if need > query(n, ho, wo, cin, cout, k):
            worst.append((row, arith, fam, s, need, query(n, ho, wo, cin, cout, k)))
    assert not worst, '%d plans above the query, first: %s' % (len(worst), worst[:5])


# CONV_CASES rows whose comment names the weight-gradient kernel they are there for
LABELLED = {
    (8, 32, 64, 64, 128, 3, 1, 0, 0): 'WINO', (16, 32, 32, 128, 16, 3, 1, 0, 0): 'WINO', (16, 32, 32, 32, 160, 3, 1, 0, 1): 'WINO',
    (2, 64, 64, 256, 128, 3, 1, 0, 0): 'WINO',
    (4, 128, 128, 16, 16, 3, 1, 0, 0): 'WSMALL',                # pose conv_7_1: the 16 -> 16 variant, not the rows kernel
    (4, 128, 128, 3, 32, 7, 1, 0, 0): 'WSMALL',                 # encoder conv_1: the 7x7 image-input variant, not the rows-merged kernel
    (8, 64, 64, 64, 4, 3, 1, 0, 0): 'WSMALL',
    # the tiny-filter block
    (2, 128, 128, 16, 16, 3, 1, 0, 1): 'WSMALL', (3, 100, 120, 16, 12, 3, 1, 0, 0): 'WSMALL', (3, 104, 120, 3, 24, 7, 1, 0, 0): 'WSMALL',
    (8, 128, 128, 3, 64, 4, 2, 1, 2): 'WSMALL', (5, 96, 72, 64, 4, 3, 1, 0, 0): 'WSMALL', (2, 128, 128, 32, 32, 3, 1, 0, 1): 'WSMALL',
    (5, 100, 72, 32, 24, 3, 1, 0, 0): 'WSMALL',
    # the two row kernels
    (4, 128, 128, 3, 16, 3, 1, 0, 0): 'ROWS_MERGED', (4, 128, 128, 16, 32, 3, 1, 0, 0): 'ROWS',
    (1, 32, 32, 128, 128, 3, 1, 0, 0): 'TAP_ROWS',              # Cin, Cout = 128: the 128x128 tile instantiation
}


def test_every_family_has_a_conv_case_and_the_labels_are_true():
    from test_ops_gpu import WGRAD_FAMILY_ROWS
    cases = conv_cases()
    assert {case_plan(row)[0] for row in cases} == set(FAMILIES)
    for row, fam in LABELLED.items():
        assert row in cases and case_plan(row)[0] == fam, (row, case_plan(row), fam)
    assert {name.split('-')[0] for name in WGRAD_FAMILY_ROWS} == set(FAMILIES)
    for name, row in WGRAD_FAMILY_ROWS.items():
        assert row in cases and case_plan(row)[0] == name.split('-')[0], (name, row, case_plan(row))
    # the entry's argument checks are the plan's
    assert lib.kpx_conv2d_wgrad_plan(A, 2, 8, 8, 16, 8, A, 8, 8, 16, 16, 3, 3, 1, 1, 1, 0, A, A, A) == -1          # ldx < Cin
    assert lib.kpx_conv2d_wgrad_plan(A, 2, 8, 8, 16, 16, A, 8, 8, 16, 16, 3, 3, 1, 1, 1, 2, A, A, A) == -1         # arith = 2
    assert lib.kpx_conv2d_wgrad_plan(None, 2, 8, 8, 16, 16, A, 8, 8, 16, 16, 3, 3, 1, 1, 1, 0, A, A, A) == -1      # x = NULL


def test_a_workspace_below_the_plan_is_refused_before_any_device_call():
    """One rule for every family: the fp32 entry answers KPX_EINVAL when workspace_bytes is below its plan's need (or the workspace is
    missing) -- no family steps aside for the next one."""
    from test_ops_gpu import WGRAD_FAMILY_ROWS
    seen = set()
    for name, row in WGRAD_FAMILY_ROWS.items():
        n, hi, wi, cin, ho, wo, cout, k, s, pad_t, pad_l = case_geometry(*row[:8])
        fam, splits, need = case_plan(row)
        if splits == 1:
            assert need == 0
            continue
        assert need == splits * k * k * cin * cout * 4
        seen.add(fam)
        args = (A, n, hi, wi, cin, cin, A, ho, wo, cout, cout, A, k, k, s, pad_t, pad_l, 0)
        assert lib.kpx_conv2d_wgrad_f32(*args, A, need - 1, None) == -1
        assert lib.kpx_conv2d_wgrad_f32(*args, None, need, None) == -1
    assert seen == set(FAMILIES)
