"""GPU parity of the loss head under BatchNorm batch statistics (syn_synergy_losses_train, syn_export_synergy_flat,
SynergyNet.loss_head(bn='batch') / recalibrate_synergy_bn) against the float64 restatement of tests/loss_train_cases.py and
the recording of the reference in train() (tests/golden/loss_train_golden.npz).  Bar: loss_cases.TOL = 1e-4 -- losses relative, batch
and running statistics relative to the max of their BatchNorm's tensor; order, repeatability and hand-over claims are equality of bits.
Figures are printed before they are asserted.  Shapes: B = 2, 3, 5, 16, 17 faces = 136 / 204 / 340 / 1088 / 1156 rows = 8.5, 12.75,
21.25, exactly 68 and 72.25 tiles of 16 rows (1088 and 1156 rows: five blocks of 256 rows, the last ragged), the heads see 2, 3, 5,
exactly 16 and 16 + 1 faces; other block sizes through the train_rows knob in child processes."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import loss_cases as lc
import loss_grad_cases as lg
import loss_train_cases as lt
import loss_wgrad_cases as lw
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

SIG = getattr(abi, '_SIGS')['syn_synergy_losses_train']             # KeyError without the feature
GUARD = 16
BATCH_SIZES = (2, 3, 5, 16, 17)
N_BN = lt.BN_CHANNELS


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(lt.GOLDEN, allow_pickle=False))


@pytest.fixture(scope='module')
def sd(gold):
    from synergynet_amd import synth
    return synth.make_synergy_state(int(gold['graph_seed']))


def _model(pack, backbone_sd, sd):
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    m.load_synergy_state(sd)
    return m


@pytest.fixture(scope='module')
def model(pack, backbone_sd, sd):
    return _model(pack, backbone_sd, sd)


@pytest.fixture(scope='module')
def second(pack, backbone_sd, sd):
    return _model(pack, backbone_sd, sd)


@functools.lru_cache(maxsize=None)
def _want_cached(which, B, momentum):
    """float64 restatement of CALLS calls: computed once per case, shared, never modified"""
    return lt.run_case(lt.TrainHead(_want_cached.pack, lt.state_of(_want_cached.sd, which), momentum=momentum), B)


@pytest.fixture(scope='module')
def want(pack, sd):
    _want_cached.pack, _want_cached.sd = pack, sd
    return _want_cached


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, value=7.0, dtype=None):
    import torch
    dtype = dtype or torch.float32
    whole = torch.full((n + 2 * GUARD,), value, dtype=dtype, device='cuda')
    return whole, whole.data_ptr() + whole.element_size() * GUARD


def _inside(whole, value=7.0):
    h = whole.cpu().numpy()
    assert (h[:GUARD] == value).all() and (h[-GUARD:] == value).all(), 'guard words overwritten'
    return h[GUARD:-GUARD].copy()


def _train(m, param, pool, target, momentum=-1.0, stats=True, meter=None):
    """syn_synergy_losses_train on host arrays, every output between guard words -> dict of numpy: the five losses, mean, var"""
    B = param.shape[0]
    pt, pot, tt = _cuda(param), _cuda(pool), _cuda(target)
    (w0, p0), (w1, p1), (w2, p2) = _guarded(2), _guarded(3 * B), _guarded(2 * N_BN)
    abi.check(m._lib.syn_synergy_losses_train(m._h, pt.data_ptr(), tt.data_ptr(), pot.data_ptr(), B, p0, p1, meter, p2 if stats else None,
                                              momentum, m._stream()))
    sc, pf, bs = _inside(w0), _inside(w1).reshape(3, B), _inside(w2)
    if not stats:
        assert (bs == 7.0).all()
    out = dict(zip(lc.LOSS_NAMES, (sc[0:1], sc[1:2], pf[0], pf[1], pf[2])))
    out.update(mean=bs[:N_BN], var=bs[N_BN:])
    return out


def _export(m):
    import torch
    n = int(m._lib.syn_synergy_flat_count())
    whole, p = _guarded(n)
    abi.check(m._lib.syn_export_synergy_flat(m._h, p, n, m._stream()))
    torch.cuda.synchronize()
    return _inside(whole)


def _running(m):
    r = lt.running_of_flat(_export(m))
    return dict(zip(('mean', 'var'), r))


def _load(m, state):
    """puts the handle (and the Python side) back to `state`"""
    m.load_synergy_state(state)


def _eval_outputs(m, B=5):
    """what the eval() entries give, as bytes: syn_synergy_losses, syn_refine_landmarks, syn_landmarks_to_param"""
    param, pool, target = lt.inputs(B)
    d = m._losses(_cuda(param), _cuda(pool), _cuda(target))
    ref = m.refine_landmarks(param, pool)
    return (b''.join(d[k].cpu().numpy().tobytes() for k in lc.LOSS_NAMES), ref.cpu().numpy().tobytes(), m.landmarks_to_param(ref).cpu().numpy().tobytes())


def _report(what, got, want, fields, channels=None):
    worst = (0.0, '')
    for f in fields:
        g = np.asarray(got[f])[channels] if (channels is not None and f in lt.PER_CHANNEL) else got[f]
        e = lt.rel(g, want[f], f, channels)
        if not e <= worst[0]:
            worst = (e, f)
    print(f'{what}: worst field off by {worst[0]:.3g} ({worst[1]}; bar {lt.TOL:g})')
    return worst[0]


LOSS_AND_STATS = lc.LOSS_NAMES + ('mean', 'var')


# ------------------------------------------------------------------ 1. accuracy, shapes, the edge state, three successive calls
@pytest.mark.parametrize('which', lt.STATES)
@pytest.mark.parametrize('B', BATCH_SIZES)
def test_losses_statistics_and_three_running_updates(model, sd, want, gold, which, B):
    state = lt.state_of(sd, which)
    if which == 'edge':
        for name, _ in lt.bn_order():
            assert (state[name + '.weight'] < 0).any() and (state[name + '.weight'] == 0).any(), name
    w = want(which, B, lt.MOMENTUM)
    try:
        _load(model, state)
        got = None
        for call in range(1, lt.CALLS + 1):
            r = _train(model, *lt.inputs(B), momentum=lt.MOMENTUM)
            if call == 1:
                got = r
            if call in (1, lt.CALLS):
                run = _running(model)
                got[f'run{call}_mean'], got[f'run{call}_var'] = run['mean'], run['var']
        assert all(np.isfinite(v).all() for v in got.values())
        fields = lc.LOSS_NAMES + lt.PER_CHANNEL
        e = _report(f'{which} B={B} against the float64 restatement', got, w, fields)
        assert e <= lt.TOL
        if B in lt.BATCHES:
            e = _report(f'{which} B={B} against the recording', got, lt.recorded(gold, which, B), fields, gold['channels'])
            assert e <= lt.TOL
    finally:
        _load(model, sd)


# ------------------------------------------------------------------ 2. row-block boundaries
CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import loss_train_cases as lt
import test_gpu_loss_train as t
from synergynet_amd import synth
from synergynet_amd.synergy3DMM import SynergyNet
g = dict(np.load(sys.argv[3], allow_pickle=False))
pack = synth.make_3dmm(int(g['seeds'][1]))
gold = dict(np.load(lt.GOLDEN, allow_pickle=False))
m = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_backbone_state(int(g['seeds'][0])))
m.load_synergy_state(lt.state_of(synth.make_synergy_state(int(gold['graph_seed'])), 'edge'))
out = t._train(m, *lt.inputs(int(sys.argv[5])), momentum=lt.MOMENTUM)
run = t._running(m)
np.savez(sys.argv[4], run1_mean=run['mean'], run1_var=run['var'], **out)
'''


@pytest.mark.parametrize('knobs,B', [('train_rows=144', 5), ('train_rows=100', 5), ('train_rows=16', 17)])
def test_row_blocks_fold_in_order(model, sd, want, tmp_path, knobs, B):
    """train_rows = 144 and B = 5 (340 rows): blocks of 144, 144 and 52 rows -- three, the last ragged.  train_rows = 100: a block size
    that is neither a multiple of 68 nor of the 16-row tile (blocks of 6.25 tiles; 100, 100, 100, 40 rows).  train_rows = 16 and B = 17:
    73 blocks of one tile, and the heads' 17 faces in two blocks (16 + 1)."""
    out = str(tmp_path / 'child.npz')
    env = dict(os.environ, SYNERGY_HIP_TEST_KNOBS=knobs)
    from conftest import ROOT
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT, os.path.join(ROOT, 'tests'), os.path.join(lg.HERE, 'golden', 'reference_outputs.npz'), out,
                        str(B)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    child = dict(np.load(out))
    fields = lc.LOSS_NAMES + ('mean', 'var', 'run1_mean', 'run1_var')
    e = _report(f'{knobs} B={B} against the float64 restatement', child, want('edge', B, lt.MOMENTUM), fields)
    assert e <= lt.TOL
    try:
        _load(model, lt.state_of(sd, 'edge'))
        dflt = _train(model, *lt.inputs(B), momentum=-1.0)
        same = all(child[f].tobytes() == dflt[f].tobytes() for f in LOSS_AND_STATS)
        print(knobs, 'against the default blocks of 256 rows: bits equal:', same, 'worst %.3g' % max(lt.rel(child[f], dflt[f], f) for f in LOSS_AND_STATS))
    finally:
        _load(model, sd)


# ------------------------------------------------------------------ 3. degenerate variance: the centred form, position independence
def test_two_identical_faces_give_relu_beta_exactly(model, sd):
    """Two identical faces: every head channel of MLP_rev sees two equal values, so its variance is exactly 0, rstd = 316, and S2 must be
    relu(beta) exactly -- which holds only if the two rows' z are bit-equal (position independence) and the normalisation is centred.
    The entry returns no S2; it is read through loss_Param_S2: the target's [12:62] is set to relu(beta)[:50], so that loss is exactly
    0.0 for a face if and only if its S2[:50] equals relu(beta)[:50] bit for bit (an fp32 difference is 0 only for equal values)."""
    param, pool, target = lt.degenerate_inputs()
    beta = np.concatenate([np.asarray(sd[f'reverseDirection.bn6_{i}.bias'], dtype=np.float32) for i in (1, 2, 3)])
    target = target.copy()
    target[:, 12:62] = np.maximum(beta, 0)[:50]
    off, _ = lt.bn_offsets()['reverseDirection.bn6_1']
    before = _running(model)
    try:
        got = _train(model, param, pool, target, momentum=lt.MOMENTUM)
        after = _running(model)
        assert all(np.isfinite(got[f]).all() for f in LOSS_AND_STATS)
        print('loss_Param_S2 of the two faces:', got['loss_Param_S2'].tolist(), '; largest head variance:', float(got['var'][off:off + 62].max()))
        assert (got['var'][off:off + 62] == 0).all()
        assert (got['loss_Param_S2'] == 0).all()
        assert all(got[k][0].tobytes() == got[k][1].tobytes() for k in lc.LOSS_NAMES[2:])
        m = np.float64(np.float32(lt.MOMENTUM))
        moved = ((1.0 - m) * before['var'][off:off + 62].astype(np.float64)).astype(np.float32)
        assert after['var'][off:off + 62].tobytes() == moved.tobytes()           # towards 0 by exactly the momentum
        assert np.isfinite(after['mean']).all() and np.isfinite(after['var']).all()
    finally:
        _load(model, sd)


# ------------------------------------------------------------------ 4. running statistics: negative momentum, recalibration
def test_negative_momentum_touches_nothing(model, sd):
    _load(model, sd)
    flat0, eval0 = _export(model), _eval_outputs(model)
    a = _train(model, *lt.inputs(5), momentum=-1.0)
    assert _export(model).tobytes() == flat0.tobytes()
    assert _eval_outputs(model) == eval0
    b = _train(model, *lt.inputs(5), momentum=-0.5, stats=False)
    assert all(a[k].tobytes() == b[k].tobytes() for k in lc.LOSS_NAMES)
    assert _export(model).tobytes() == flat0.tobytes()


def test_recalibration_is_the_mean_of_the_batches_statistics(model, sd, pack):
    param, pool, target = lg.candidate_inputs()
    cuts = ((0, 2), (2, 7), (7, 10))                                              # batches of 2, 5 and 3 faces
    batches = [(param[a:b], pool[a:b], target[a:b]) for a, b in cuts]
    h = lt.TrainHead(pack, sd, momentum=None)
    means, uvars = [], []
    for p, po, t in batches:
        r = h.forward(p, po, t)
        n = np.concatenate([np.full(c, p.shape[0] * (1 if 'bn6_' in name else 68)) for name, c in lt.bn_order()]).astype(np.float64)
        means.append(r['mean'])
        uvars.append(r['var'] * n / (n - 1))
    w = dict(mean=np.mean(means, 0), var=np.mean(uvars, 0))
    try:
        _load(model, sd)
        assert model.recalibrate_synergy_bn(batches) == 3
        got = _running(model)
        e = max(lt.rel(got[f], w[f], f) for f in ('mean', 'var'))
        print(f'recalibration over batches of 2, 5, 3 faces: running statistics off by {e:.3g} from the mean of the batches (bar {lt.TOL:g})')
        assert e <= lt.TOL
        sdict = model.synergy_state_dict()
        r = lt.running_of_flat(lw_flat(sdict))
        assert r[0].tobytes() == got['mean'].tobytes() and r[1].tobytes() == got['var'].tobytes()
    finally:
        _load(model, sd)


def lw_flat(sdict):
    from synergynet_amd import synth
    return synth.flatten_synergy({k: v.cpu().numpy() for k, v in sdict.items()})


# ------------------------------------------------------------------ 5. hand-over to the eval() entries
def test_eval_entries_see_the_moved_statistics(model, second, sd):
    try:
        _load(model, sd)
        before = _eval_outputs(model)
        _train(model, *lt.inputs(5), momentum=lt.MOMENTUM)
        flat = _export(model)
        assert flat.tobytes() != synth_flat(sd).tobytes()
        abi.check(second._lib.syn_load_synergy(second._h, flat.ctypes.data_as(ctypes.c_void_p), flat.size))      # FROM THE HOST
        after, host = _eval_outputs(model), _eval_outputs(second)
        assert after != before
        for what, a, b in zip(('syn_synergy_losses', 'syn_refine_landmarks', 'syn_landmarks_to_param'), after, host):
            print(f'{what} after a call that moved the statistics: bit-equal to a host load of the exported flat: {a == b}')
            assert a == b
    finally:
        _load(model, sd)
        _load(second, sd)


def synth_flat(sd):
    from synergynet_amd import synth
    return synth.flatten_synergy(sd)


# ------------------------------------------------------------------ 6. bits
def test_same_bits_on_every_call_and_handle_and_no_scratch_history(model, second, sd):
    try:
        _load(model, sd)
        _load(second, sd)
        a = _train(model, *lt.inputs(17), momentum=lt.MOMENTUM)
        fa = _export(model)
        _load(model, sd)
        b = _train(model, *lt.inputs(17), momentum=lt.MOMENTUM)
        c = _train(second, *lt.inputs(17), momentum=lt.MOMENTUM)
        assert all(a[f].tobytes() == b[f].tobytes() == c[f].tobytes() for f in LOSS_AND_STATS)
        assert fa.tobytes() == _export(model).tobytes() == _export(second).tobytes()
        _load(model, sd)
        _load(second, sd)
        _train(model, *lt.inputs(17))
        small, fresh = _train(model, *lt.inputs(3)), _train(second, *lt.inputs(3))          # B = 3 after B = 17 against B = 3 first
        assert all(small[f].tobytes() == fresh[f].tobytes() for f in LOSS_AND_STATS)
    finally:
        _load(model, sd)
        _load(second, sd)


# ------------------------------------------------------------------ 7. conventions, guards, refusals
def test_nan_target_element_is_not_counted_and_the_meter_adds_the_batch(model, sd, pack):
    import torch
    param, pool, target = lt.inputs(5)
    target = target.copy()
    target[1, 20] = np.nan
    w = lt.TrainHead(pack, sd, momentum=None).forward(param, pool, target)
    _load(model, sd)
    got = _train(model, param, pool, target)
    for k in lc.LOSS_NAMES:
        assert lg.same_classes(got[k], w[k]), k
        fin = np.isfinite(w[k].reshape(-1))
        e = float((np.abs(got[k].reshape(-1)[fin] - w[k].reshape(-1)[fin]) / np.abs(w[k].reshape(-1)[fin])).max()) if fin.any() else 0.0
        print(f'NaN target element, {k}: off by {e:.3g} on the finite entries; NaN entries: {int((~fin).sum())}')
        assert e <= lt.TOL
    assert np.isfinite(got['loss_LMK_f0']).all()                                  # the NaN elements are not counted, not summed
    param, pool, target = lt.inputs(5)
    mw, mp = _guarded(8, 0.0, torch.float64)
    got = _train(model, param, pool, target, meter=mp)
    meter = _inside(mw, 0.0)
    means = [float(np.asarray(got[k], dtype=np.float32).mean(dtype=np.float64)) for k in lc.LOSS_NAMES]
    assert meter[6] == 5 and meter[7] == 1
    assert np.allclose(meter[:5], np.array(means) * 5, rtol=1e-6) and np.isclose(meter[5], sum(means) * 5, rtol=1e-6)


def test_refusals_leave_the_outputs_untouched(model, sd, pack, backbone_sd):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    lib, s = model._lib, model._stream()
    _load(model, sd)
    flat0 = _export(model)
    param, pool, target = lt.inputs(3)
    pt, pot, tt = _cuda(param), _cuda(pool), _cuda(target)
    (w0, p0), (w1, p1), (w2, p2) = _guarded(2), _guarded(9), _guarded(2 * N_BN)
    P, T, PO, h = pt.data_ptr(), tt.data_ptr(), pot.data_ptr(), model._h
    call = lib.syn_synergy_losses_train
    for args in ((None, T, PO, 3, p0, p1, None, p2, 0.1), (P, None, PO, 3, p0, p1, None, p2, 0.1), (P, T, None, 3, p0, p1, None, p2, 0.1),
                 (P, T, PO, 3, None, p1, None, p2, 0.1), (P, T, PO, 3, p0, None, None, p2, 0.1),
                 (P, T, PO, 1, p0, p1, None, p2, 0.1), (P, T, PO, 0, p0, p1, None, p2, 0.1), (P, T, PO, -3, p0, p1, None, p2, 0.1),
                 (P, T, PO, 3, p0, p1, None, p2, 1.5), (P, T, PO, 3, p0, p1, None, p2, float('nan')),
                 (P, T, PO, 3, p0, p0 + 4, None, p2, 0.1), (P, T, PO, 3, p0, p1, None, p1 + 8, 0.1)):
        assert call(h, *args, s) == abi.SYN_ERR_INVALID, args
        assert b'syn_synergy_losses_train' in lib.syn_last_error()
    assert call(h, P, T, PO, 1, p0, p1, None, p2, 0.1, s) == abi.SYN_ERR_INVALID
    assert b'Expected more than 1 value per channel when training, got input size [1, 12, 1]' in lib.syn_last_error()
    unloaded = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    assert call(unloaded._h, P, T, PO, 3, p0, p1, None, p2, 0.1, s) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_export_synergy_flat(unloaded._h, p2, lib.syn_synergy_flat_count(), s) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_export_synergy_flat(h, p2, 5, s) == abi.SYN_ERR_INVALID
    rn = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_resnet50_state(), arch='resnet50')
    assert call(rn._h, P, T, PO, 3, p0, p1, None, p2, 0.1, s) == abi.SYN_ERR_INVALID
    assert b'1280-d' in lib.syn_last_error() and b'resnet50' in lib.syn_last_error()
    assert (_inside(w0) == 7.0).all() and (_inside(w1) == 7.0).all() and (_inside(w2) == 7.0).all()
    assert _export(model).tobytes() == flat0.tobytes()


# ------------------------------------------------------------------ 8. the Python surface
def test_python_surface(pack, backbone_sd, sd, second):
    import torch
    m = _model(pack, backbone_sd, sd)
    _load(second, sd)
    param, pool, target = lt.inputs(5)
    # the default path gives today's bits and moves nothing
    flat0 = _export(m)
    d0 = m.loss_head(param, pool, target)
    base = second._losses(_cuda(param), _cuda(pool), _cuda(target))
    assert all(torch.equal(d0[k], base[k]) for k in lc.LOSS_NAMES)
    assert all(torch.equal(m.loss_head(param, pool, target, bn='running')[k], base[k]) for k in lc.LOSS_NAMES)
    assert _export(m).tobytes() == flat0.tobytes()
    # bn='batch': the reference's dict with the C entry's bits; momentum None moves nothing
    d = m.loss_head(param, pool, target, bn='batch', momentum=None)
    c = _train(second, param, pool, target, momentum=-1.0)
    assert list(d) == list(lc.LOSS_NAMES) and d['loss_LMK_f0'].dim() == 0 and tuple(d['loss_Param_S2'].shape) == (5,)
    assert all(d[k].cpu().numpy().reshape(-1).tobytes() == c[k].tobytes() for k in lc.LOSS_NAMES)
    assert _export(m).tobytes() == flat0.tobytes()
    # whatever requires grad raises: never the eval() gradients
    for p, po in ((_cuda(param).requires_grad_(True), _cuda(pool)), (_cuda(param), _cuda(pool).requires_grad_(True))):
        with pytest.raises(RuntimeError, match='no backward under BatchNorm batch statistics'):
            m.loss_head(p, po, target, bn='batch')
    with pytest.raises(RuntimeError, match='more than 1 value per channel'):
        m.loss_head(param[:1], pool[:1], target[:1], bn='batch')
    with pytest.raises(RuntimeError, match='momentum'):
        m.loss_head(param, pool, target, bn='batch', momentum=1.5)
    with pytest.raises(RuntimeError, match="'running' or 'batch'"):
        m.loss_head(param, pool, target, bn='train')
    assert _export(m).tobytes() == flat0.tobytes()
    # a call that moves the statistics: synergy_state_dict() returns them (before synergy_parameters() exists: through the export)
    m.loss_head(param, pool, target, bn='batch')
    _train(second, param, pool, target, momentum=0.1)
    flat1 = _export(second)
    assert _export(m).tobytes() == flat1.tobytes() != flat0.tobytes()
    assert lw_flat(m.synergy_state_dict()).tobytes() == flat1.tobytes()
    # with synergy_parameters(): they require grad, so bn='batch' needs no_grad; the running_* tensors follow and nothing stale goes up
    ws = m.synergy_parameters()
    assert lw_flat({**m.synergy_state_dict()}).tobytes() == flat1.tobytes()
    with pytest.raises(RuntimeError, match='no backward under BatchNorm batch statistics'):
        m.loss_head(param, pool, target, bn='batch')
    with torch.no_grad():
        m.loss_head(param, pool, target, bn='batch')
        ws['forwardDirection.bn3.bias'].add_(0.0)                                   # a version bump: the next call uploads the Python tensors
        e1 = m.loss_head(param, pool, target)
    _train(second, param, pool, target, momentum=0.1)
    flat2 = _export(second)
    assert flat2.tobytes() != flat1.tobytes()
    assert _export(m).tobytes() == flat2.tobytes()                                  # the upload carried the MOVED statistics, not stale ones
    assert lw_flat(m.synergy_state_dict()).tobytes() == flat2.tobytes()
    e2 = second._losses(_cuda(param), _cuda(pool), _cuda(target))
    assert all(torch.equal(e1[k], e2[k]) for k in lc.LOSS_NAMES)
    # model(input, target, bn='batch') goes through the same entry
    from synergynet_amd import synth
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(3, seed=3))).cuda()
    with torch.no_grad():
        pr, pl = m.forward_test(x, return_pool=True)
        f = m(x, target[:3], bn='batch', momentum=None)
        g = m.loss_head(pr, pl, target[:3], bn='batch', momentum=None)
    assert all(torch.equal(f[k], g[k]) for k in lc.LOSS_NAMES)
    _load(second, sd)
