"""The loss head under BatchNorm batch statistics without a GPU: the float64 restatement of tests/loss_train_cases.py against
the REAL reference in train() as recorded in tests/golden/loss_train_golden.npz (bar 1e-5: losses relative, S2 / refined landmarks
relative to the max of the tensor, statistics and running statistics relative to the max of their BatchNorm's tensor), the bite of the
fixture -- each wrong port misses the bar on some recorded field, and by how much is printed --, the new symbols in header / ctypes table
/ library, the channel count and the refusals that touch no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import loss_cases as lc
import loss_grad_cases as lg
import loss_train_cases as lt
from conftest import ROOT

NEW_SYMBOLS = ('syn_synergy_bn_channels', 'syn_synergy_losses_train', 'syn_export_synergy_flat')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(lt.GOLDEN, allow_pickle=False))


@pytest.fixture(scope='module')
def state(gold):
    from synergynet_amd import synth
    g = dict(np.load(os.path.join(lg.HERE, 'golden', 'reference_outputs.npz'), allow_pickle=False))
    return synth.make_3dmm(int(g['seeds'][1])), synth.make_synergy_state(int(gold['graph_seed']))


def test_fixture_is_data_and_small(gold):
    assert all(v.dtype.kind in 'iufU' for v in gold.values())
    assert os.path.getsize(lt.GOLDEN) <= 512 << 10
    assert np.array_equal(gold['channels'], lt.recorded_channels())
    assert sum(n for _, n in lt.bn_order()) == lt.BN_CHANNELS
    for s in lt.STATES:
        for B in lt.BATCHES:
            assert all(lt.case_key(s, B, f) in gold for f in lt.RECORDED_FIELDS)


def test_edge_state_has_negative_and_zero_gamma_in_every_batchnorm(state):
    edge = lt.edge_state(state[1])
    for name, n in lt.bn_order():
        g = edge[name + '.weight']
        assert (g < 0).any() and (g == 0).any() and (g > 0).any(), name
        assert (state[1][name + '.weight'] > 0).all()


@pytest.mark.parametrize('which', lt.STATES)
@pytest.mark.parametrize('B', lt.BATCHES)
def test_restatement_matches_the_recording(gold, state, which, B):
    got = lt.run_case(lt.TrainHead(state[0], lt.state_of(state[1], which)), B)
    want = lt.recorded(gold, which, B)
    for f in lt.RECORDED_FIELDS:
        g = np.asarray(got[f])[gold['channels']] if f in lt.PER_CHANNEL else got[f]
        print(f'{which} B={B} {f}: off by {lt.rel(g, want[f], f, gold["channels"]):.3g}')
    e, at = lt.worst(got, want, channels=gold['channels'])
    assert e <= lt.CPU_BAR, (at, e)


@pytest.mark.parametrize('wrong', lt.WRONG)
def test_fixture_bites(gold, state, wrong):
    """edge state, B = 5: every wrong variant moves at least one recorded field past the bar"""
    got = lt.run_case(lt.TrainHead(state[0], lt.state_of(state[1], 'edge'), wrong=wrong), 5)
    e, at = lt.worst(got, lt.recorded(gold, 'edge', 5), channels=gold['channels'])
    print(f'{wrong}: misses the recording by {e:.3g} on {at} (bar {lt.CPU_BAR:g})')
    assert e > 10 * lt.CPU_BAR


def test_momentum_none_leaves_the_running_statistics(state):
    h = lt.TrainHead(*state, momentum=None)
    before = h.running()
    h.forward(*lt.inputs(3))
    after = h.running()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


def test_new_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import build_library
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    for s in NEW_SYMBOLS:
        assert s in abi.EXPORTED_SYMBOLS and hasattr(l, s), s
        decl = re.search(r'\b(?:int|size_t) ' + s + r'\(([^;]*)\);', hdr)
        assert decl, s
        args = re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).strip()
        assert (0 if args == 'void' else len(args.split(','))) == len(abi._SIGS[s][1]), s


def test_bn_channels():
    from synergynet_amd import abi
    assert abi.lib().syn_synergy_bn_channels() == lt.BN_CHANNELS == 2243 + 1406


def test_refusals_that_need_no_device():
    from synergynet_amd import abi
    lib = abi.lib()
    buf = np.full(8, 7.0, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    call = lib.syn_synergy_losses_train
    for args in ((None, p, p, p, 2, p, p, None, None, 0.1, None), (None, p, p, p, 1, p, p, None, p, 0.1, None)):
        assert call(*args) == abi.SYN_ERR_INVALID
        assert b'syn_synergy_losses_train' in lib.syn_last_error()
    assert lib.syn_export_synergy_flat(None, p, lib.syn_synergy_flat_count(), None) == abi.SYN_ERR_INVALID
    assert b'syn_export_synergy_flat' in lib.syn_last_error() and b'NULL' in lib.syn_last_error()
    assert (buf == 7.0).all()


def test_python_surface_names():
    import inspect
    from synergynet_amd import synergy3DMM as s
    for m in ('loss_head', 'forward', 'recalibrate_synergy_bn', '_losses_train', 'synergy_state_dict'):
        assert callable(getattr(s.SynergyNet, m)), m
    for m in ('loss_head', 'forward'):
        sig = inspect.signature(getattr(s.SynergyNet, m))
        assert sig.parameters['bn'].default == 'running' and sig.parameters['momentum'].default == 0.1, m
