"""The losses of the training graph's forward and CenterCrop without a GPU: the float64 restatement of tests/loss_cases.py against the
reference's recorded results (tests/golden/loss_golden.npz), the bite of the fixture -- each wrong port moves a recorded case far beyond
the bar, and by how much is printed --, the new symbols in header / ctypes table / library, and the refusals that touch no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import loss_cases as lc
from conftest import ROOT

NEW_SYMBOLS = ('syn_wing_loss', 'syn_param_loss', 'syn_synergy_losses', 'syn_center_crop_u8')


@pytest.fixture(scope='module')
def lgold():
    return dict(np.load(lc.GOLDEN, allow_pickle=False))


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def test_fixture_is_data_and_its_inputs_come_back_from_the_integers(lgold):
    assert all(v.dtype.kind in 'iufU' for v in lgold.values())
    assert os.path.getsize(lc.GOLDEN) < 400 << 10
    for name in lc.wing_case_names():
        B, n, v = lc.parse_wing_case(name)
        assert np.array_equal(lc.checksum(*lc.wing_inputs(B, n, v)), lgold[name + '_sum']), name
    for B in lc.PARAM_B:
        for same in (False, True):
            assert np.array_equal(lc.checksum(*lc.param_inputs(B, same)), lgold[f'param_B{B}_normal' + ('_same' if same else '') + '_sum'])
    assert np.array_equal(lc.checksum(lc.ramp()[0]), lgold['crop_sum'])


@pytest.mark.parametrize('name', lc.wing_case_names())
def test_wing_restatement_matches_the_recording(lgold, name):
    B, n, v = lc.parse_wing_case(name)
    pred, target = lc.wing_inputs(B, n, v)
    d = np.abs(target.astype(np.float64) - pred.astype(np.float64))
    below = float(np.nextafter(np.float32(lc.OMEGA), np.float32(0)))
    if v != 'allnan':                                             # exactly omega, and its fp32 neighbour below
        assert d.ravel()[1] == below and d.ravel()[0] == (below if v == 'small' else lc.OMEGA)
    if v in ('plain', 'nan', 'inf') and d.size >= 200:
        assert (d < lc.OMEGA).any() and (d >= lc.OMEGA).any() and np.nanmax(d[np.isfinite(d)]) > 25       # both branches, spread to 30
    if v == 'small':
        assert (d < lc.OMEGA).all()                                                                        # empty linear branch
    got, want = lc.wing(pred, target), lgold[name]
    assert lc.same_class(got, want), (name, got, want)
    if np.isfinite(want):
        print(name, 'rel', _rel(got, want))
        assert _rel(got, want) <= lc.CPU_BAR


@pytest.mark.parametrize('B', lc.PARAM_B)
@pytest.mark.parametrize('mode', ['normal', 'only_3dmm'])
def test_param_restatement_matches_the_recording(lgold, B, mode):
    for same in (False, True):
        a, b = lc.param_inputs(B, same)
        want = lgold[f'param_B{B}_{mode}' + ('_same' if same else '')]
        got = lc.param_loss(a, b, mode)
        assert got.shape == want.shape == (B,)
        assert _rel(got, want) <= lc.CPU_BAR
        if same and mode == 'normal':
            assert (want == 0).all() and (got == 0).all()              # input == target: exactly 0
        else:
            assert (want > 0.5).all()                                  # only_3dmm of a tensor with itself is NOT 0: the slices are shifted


def test_graph_restatement_matches_the_recording(lgold):
    g = lambda k: lgold['graph_' + k]
    d = np.abs(g('lmk').astype(np.float64) - g('lmk_gt'))
    assert d.mean() > 2 and (d < lc.OMEGA).any() and (d >= lc.OMEGA).any()
    assert np.array_equal(g('lmk_refined') >= g('lmk'), np.ones_like(g('lmk'), dtype=bool)) and (g('lmk_refined') != g('lmk')).any()
    got = lc.graph_losses(g('param'), g('target'), g('lmk'), g('lmk_gt'), g('lmk_refined'), g('param_rev'))
    for name, v in zip(lc.LOSS_NAMES, got):
        want = g(name)
        assert np.shape(v) == want.shape == (() if 'LMK' in name else (5,))
        print(name, 'rel', _rel(v, want))
        assert _rel(v, want) <= lc.CPU_BAR


@pytest.mark.parametrize('m', lc.CROP_MARGINS)
def test_center_crop_restatement_matches_the_recording(lgold, m):
    img = lc.ramp()[0]
    assert img.min() >= 1
    want = lgold[f'crop_m{m}']
    assert np.array_equal(lc.center_crop(img, m), want)
    assert int(want.any(2).sum()) == max(120 - 2 * m, 0) ** 2


# ---- the fixture bites ----
def _moved(name, wrong, want, factor=100):
    r = _rel(wrong, want)
    print(f'{name}: the wrong variant is off by {r:.3g} (bar {lc.CPU_BAR:g})')
    assert r > factor * lc.CPU_BAR, (name, r)


def test_bite_counting_the_nan_element(lgold):
    pred, target = lc.wing_inputs(3, 68, 'nan')
    _moved('NaN counted', lc.wing(pred, target, count_nan=True), lgold['wing_B3_n68_nan'])


def test_bite_boundary_element_in_the_log_branch_with_another_constant(lgold):
    """The two branches meet at omega (omega log(1 + omega / eps) = omega - C), so moving the boundary element alone cannot show in the
    value: the first line prints that.  It shows as soon as C is not the reference's -- here the constant of a port that forms the
    log term as log(1 + eps / omega)."""
    pred, target = lc.wing_inputs(1, 1, 'plain')                 # 3 elements, one of them exactly omega
    want = lgold['wing_B1_n1_plain']
    print('boundary element moved alone: off by', _rel(lc.wing(pred, target, boundary_to_log=True), want))
    assert _rel(lc.wing(pred, target, boundary_to_log=True), want) <= lc.CPU_BAR
    C = lc.OMEGA - lc.OMEGA * np.log(1.0 + lc.EPSILON / lc.OMEGA)
    for name in ('wing_B3_n68_plain', 'wing_B1025_n68_plain'):
        B, n, v = lc.parse_wing_case(name)
        _moved(name + ' wrong C', lc.wing(*lc.wing_inputs(B, n, v), boundary_to_log=True, C=C), lgold[name])


def test_bite_aligned_only_3dmm_slices(lgold):
    a, b = lc.param_inputs(3)
    _moved('only_3dmm aligned', lc.param_loss(a, b, 'only_3dmm', aligned=True), lgold['param_B3_only_3dmm'])
    g = lambda k: lgold['graph_' + k]
    wrong = lc.graph_losses(g('param'), g('target'), g('lmk'), g('lmk_gt'), g('lmk_refined'), g('param_rev'), aligned=True)
    _moved('graph loss_Param_S2 aligned', wrong[3], g('loss_Param_S2'))
    _moved('graph loss_Param_S1S2 aligned', wrong[4], g('loss_Param_S1S2'))


@pytest.mark.parametrize('m', [4, 6])
def test_bite_border_of_another_width(lgold, m):
    wrong, want = lc.center_crop(lc.ramp()[0], m), lgold['crop_m5']
    n = int((wrong != want).any(2).sum())
    print(f'margin {m} instead of 5: {n} pixels differ')
    assert n == abs((120 - 2 * m) ** 2 - 110 ** 2)


# ---- ABI ----
def test_new_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import build_library
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    for s in NEW_SYMBOLS:
        assert s in abi.EXPORTED_SYMBOLS and hasattr(l, s), s
        decl = re.search(r'\bint ' + s + r'\(([^;]*)\);', hdr)
        assert decl, s
        args = re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S)
        assert len(args.split(',')) == len(abi._SIGS[s][1]), s
    l.syn_abi_version.restype = ctypes.c_int
    assert l.syn_abi_version() == 1


def test_null_handle_is_refused_without_a_device():
    from synergynet_amd import abi
    lib = abi.lib()
    buf = np.full(8, 7.0, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for name, call in (('syn_wing_loss', lambda: lib.syn_wing_loss(None, p, p, 1, 1, 10.0, 2.0, p, None)),
                       ('syn_param_loss', lambda: lib.syn_param_loss(None, p, p, 1, 0, p, None)),
                       ('syn_synergy_losses', lambda: lib.syn_synergy_losses(None, p, p, p, 1, p, p, None, None)),
                       ('syn_center_crop_u8', lambda: lib.syn_center_crop_u8(None, p, 1, 1, 1, 1, 0, p, None))):
        assert call() == abi.SYN_ERR_INVALID, name
        assert name.encode() in lib.syn_last_error() and b'NULL' in lib.syn_last_error()
    assert (buf == 7.0).all()


def test_python_surface_names():
    from synergynet_amd import evaluate
    from synergynet_amd.synergy3DMM import LOSS_NAMES, SynergyNet
    assert LOSS_NAMES == lc.LOSS_NAMES
    for m in ('forward', 'get_losses', 'losses_crops_u8', 'wing_loss', 'param_loss', 'validate'):
        assert callable(getattr(SynergyNet, m)), m
    for f in ('center_crop', 'extract_param', 'benchmark'):
        assert callable(getattr(evaluate, f)), f
