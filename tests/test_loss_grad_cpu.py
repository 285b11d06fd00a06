"""Gradients of the loss head without a GPU: the float64 torch restatement of tests/loss_grad_cases.py against torch autograd through the
reference as recorded in tests/golden/loss_grad_golden.npz (bar 1e-5 x max |g| per tensor), the bite of the fixture -- each wrong port
moves a recorded tensor by more than ten times the bar, and by how much is printed --, the new symbols in header / ctypes table /
library, and the refusals that touch no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import loss_cases as lc
import loss_grad_cases as lg
from conftest import ROOT

NEW_SYMBOLS = ('syn_synergy_losses_backward', 'syn_wing_loss_backward', 'syn_param_loss_backward')


@pytest.fixture(scope='module')
def ggold():
    return dict(np.load(lg.GOLDEN, allow_pickle=False))


@pytest.fixture(scope='module')
def head(ggold):
    from synergynet_amd import synth
    g = dict(np.load(os.path.join(lg.HERE, 'golden', 'reference_outputs.npz'), allow_pickle=False))
    return lg.Head(synth.make_3dmm(int(g['seeds'][1])), synth.make_synergy_state(int(ggold['graph_seed'])))


@pytest.fixture(scope='module')
def head_grads(head):
    return head.grads(*lg.graph_inputs())                     # computed once, shared, never modified


def _close(name, got, want):
    assert lg.same_classes(got, want), name
    r = lg.rel_to_max(got, want)
    print(f'{name}: off by {r:.3g} x max |g| (bar {lg.CPU_BAR:g})')
    assert r <= lg.CPU_BAR, (name, r)


def _moved(name, wrong, want):
    r = lg.rel_to_max(wrong, want)
    print(f'{name}: the wrong variant is off by {r:.3g} x max |g| (bar {lg.CPU_BAR:g})')
    assert r > 10 * lg.CPU_BAR, (name, r)


def test_fixture_is_data_and_small(ggold):
    assert all(v.dtype.kind in 'iufU' for v in ggold.values())
    assert os.path.getsize(lg.GOLDEN) < 400 << 10


@pytest.mark.parametrize('name', lc.wing_case_names())
def test_wing_gradient_restatement_matches_the_recording(ggold, name):
    B, n, v = lc.parse_wing_case(name)
    pred, target = lc.wing_inputs(B, n, v)
    want = ggold['g_' + name]
    got = lg.wing_grad(pred, target)
    _close(name, lg.recorded_part(got, B), want)
    d = np.abs(target.astype(np.float64) - pred.astype(np.float64)).ravel()
    if v == 'nan':
        assert got.ravel()[np.isnan(d)].tolist() == [0.0] and np.isfinite(want).all()       # not counted, gradient 0, no NaN anywhere
    if v == 'inf':
        n_counted = d.size
        assert abs(abs(got.ravel()[np.isinf(d)][0]) - 1.0 / n_counted) < 1e-12              # linear branch: +-1 / n
    if v == 'allnan':
        assert (want == 0).all() and (got == 0).all()


@pytest.mark.parametrize('key', lg.param_grad_keys())
def test_param_gradient_restatement_matches_the_recording(ggold, key):
    B, mode, same = int(key.split('_')[1][1:]), ('only_3dmm' if 'only_3dmm' in key else 'normal'), key.endswith('_same')
    a, b = lc.param_inputs(B, same)
    got = lg.param_grad(a, b, mode, lg.param_grad_upstream(B))
    for side, x in zip(('in', 'tg'), got):
        want = ggold[f'g_{key}_{side}']
        _close(f'{key}_{side}', lg.recorded_part(x, B), want)
        assert np.isnan(want).all() == (same and mode == 'normal')                           # sqrt'(0) x 0: the whole tensor is NaN
    if mode == 'only_3dmm':
        assert (got[0][:, 50:] == 0).all() and (got[1][:, :12] == 0).all()                   # outside the misaligned slices


def test_identical_face_is_a_nan_row_that_stays_in_its_row(ggold):
    a, b = lg.identical_face()
    got = lg.param_grad(a, b, 'normal', lg.param_grad_upstream(3))
    for side, x in zip(('in', 'tg'), got):
        want = ggold[f'g_identical_{side}']
        assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()
        _close('identical_' + side, x, want)


def test_tie_goes_to_the_first_maximum(ggold):
    import torch
    assert ggold['tie_grad'].tolist() == [0.0, 1.0, 0.0, 0.0]
    x = torch.tensor(lg.TIE_ROW, dtype=torch.float64).reshape(1, 1, 4).requires_grad_(True)
    lg.Head._max(x).sum().backward()
    assert x.grad.reshape(4).tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize('name', lc.LOSS_NAMES + ('total',))
def test_graph_gradient_restatement_matches_the_recording(ggold, head_grads, name):
    for what, got in zip(('param', 'pool'), head_grads[name]):
        want = ggold[f'graph_d_{what}_{name}']
        assert got.shape == want.shape
        _close(f'graph_d_{what}_{name}', got, want)
    if name in ('loss_LMK_f0', 'loss_Param_In'):
        assert (ggold[f'graph_d_pool_{name}'] == 0).all()                                   # these two never see the pooled feature
    else:
        assert (ggold[f'graph_d_pool_{name}'] != 0).all()
    assert (ggold[f'graph_d_param_{name}'] != 0).all()


# ---- the fixture bites ----
def test_bite_dropping_the_param_term_of_param_s1s2(ggold, head):
    wrong = head.grads(*lg.graph_inputs(), drop_s1s2_param=True)
    _moved('Param_S1S2 without d param[12:62]', wrong['loss_Param_S1S2'][0], ggold['graph_d_param_loss_Param_S1S2'])
    # the loss's weight is 0.001: in the TOTAL the missing term is below the GPU bar (printed, not asserted), so a GPU test has to
    # hold loss_Param_S1S2's own gradient to the recording, not only the total's
    print('total without it: off by %.3g x max |g|' % lg.rel_to_max(wrong['total'][0], ggold['graph_d_param_total']))


def test_bite_aligned_only_3dmm_slices(ggold, head):
    wrong = head.grads(*lg.graph_inputs(), aligned=True)
    for name in ('loss_Param_S2', 'loss_Param_S1S2'):
        _moved(name + ' aligned, d param', wrong[name][0], ggold[f'graph_d_param_{name}'])
        _moved(name + ' aligned, d pool', wrong[name][1], ggold[f'graph_d_pool_{name}'])
    a, b = lc.param_inputs(3)
    _moved('module only_3dmm aligned', lg.param_grad(a, b, 'only_3dmm', lg.param_grad_upstream(3), aligned=True)[0], ggold['g_param_B3_only_3dmm_in'])


def test_bite_ties_routed_to_the_last_maximum(ggold):
    import torch
    x = torch.tensor(lg.TIE_ROW, dtype=torch.float64).reshape(1, 1, 4).requires_grad_(True)
    lg.Head._max(x, last=True).sum().backward()
    assert x.grad.reshape(4).tolist() == [0.0, 0.0, 1.0, 0.0]
    _moved('tie to the last maximum', x.grad.reshape(4).numpy(), ggold['tie_grad'])


def test_bite_counting_nan_elements_in_n(ggold):
    pred, target = lc.wing_inputs(3, 68, 'nan')
    _moved('NaN counted in n', lg.wing_grad(pred, target, count_nan=True), ggold['g_wing_B3_n68_nan'])


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


def test_refusals_that_need_no_device():
    from synergynet_amd import abi
    lib = abi.lib()
    buf = np.full(8, 7.0, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for g_s, g_p in ((p, None), (None, p)):                  # exactly one g_* NULL, with a NULL handle: refused whichever check comes first
        assert lib.syn_synergy_losses_backward(None, p, p, p, 1, g_s, g_p, p, p, None) == abi.SYN_ERR_INVALID
        assert b'syn_synergy_losses_backward' in lib.syn_last_error()
    for name, call in (('syn_synergy_losses_backward', lambda: lib.syn_synergy_losses_backward(None, p, p, p, 1, None, None, p, p, None)),
                       ('syn_wing_loss_backward', lambda: lib.syn_wing_loss_backward(None, p, p, 1, 1, 10.0, 2.0, None, p, None)),
                       ('syn_param_loss_backward', lambda: lib.syn_param_loss_backward(None, p, p, 1, 0, None, p, p, None))):
        assert call() == abi.SYN_ERR_INVALID, name
        assert name.encode() in lib.syn_last_error() and b'NULL' in lib.syn_last_error()
    assert (buf == 7.0).all()


def test_python_surface_names():
    from synergynet_amd import synergy3DMM as s
    import torch
    for f in (s._WingLossFn, s._ParamLossFn, s._LossHeadFn):
        assert issubclass(f, torch.autograd.Function)
    for m in ('loss_head', 'loss_total_grad', '_wing_loss_backward', '_param_loss_backward'):
        assert callable(getattr(s.SynergyNet, m)), m
