"""GPU parity of the loss head's weight gradients (syn_synergy_losses_backward_weights, syn_update_synergy_device,
SynergyNet.synergy_parameters / loss_head / synergy_state_dict) against torch autograd through the reference as recorded in
tests/golden/loss_wgrad_golden.npz and against the float64 restatement of tests/loss_wgrad_cases.py.  Bar: 1e-4 x max |g| per tensor
(loss_cases.TOL); a tensor whose expected maximum is 0 must be exactly 0; order and repeatability claims are equality of bits.  Figures are
printed before they are asserted.  Shapes: 1 face (68 rows = 17 whole steps of the matrix instruction's K), 3 and 5 faces (the per-face
products pad their last step of four faces), 17 = 16 + 1 (five chunks of the per-point products), 30; passes of 4, 4 and 1 faces and chunks of 2 and 1 faces through the wgrad_pass /
wgrad_chunk knobs in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import loss_cases as lc
import loss_grad_cases as lg
import loss_wgrad_cases as lw
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

SIG = getattr(abi, '_SIGS')['syn_synergy_losses_backward_weights']             # KeyError without the feature
GUARD = 16
BATCH_SIZES = (1, 3, 4, 5, 9, 17, 30)


@pytest.fixture(scope='module')
def wgold():
    return dict(np.load(lw.GOLDEN, allow_pickle=False))


@pytest.fixture(scope='module')
def sd(wgold):
    from synergynet_amd import synth
    return synth.make_synergy_state(int(wgold['graph_seed']))


@pytest.fixture(scope='module')
def model(pack, backbone_sd, sd):
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    m.load_synergy_state(sd)
    return m


@pytest.fixture(scope='module')
def second(pack, backbone_sd, sd):
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    m.load_synergy_state(sd)
    return m


@pytest.fixture(scope='module')
def h64(pack, sd):
    return lw.WHead(pack, sd)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, value=7.0):
    import torch
    whole = torch.full((n + 2 * GUARD,), value, dtype=torch.float32, device='cuda')
    return whole, whole.data_ptr() + 4 * GUARD


def _inside(whole, value=7.0):
    h = whole.cpu().numpy()
    assert (h[:GUARD] == value).all() and (h[-GUARD:] == value).all(), 'guard words overwritten'
    return h[GUARD:-GUARD]


def _wbwd(m, param, pool, target, gs=None, gp=None, data=True):
    """syn_synergy_losses_backward_weights on host arrays, outputs between guard words -> (d_flat, d_param or None, d_pool or None)"""
    B = param.shape[0]
    pt, pot, tt = _cuda(param), _cuda(pool), _cuda(target)
    gst, gpt = (_cuda(gs), _cuda(gp)) if gs is not None else (None, None)
    (w0, p0), (w1, p1), (w2, p2) = _guarded(B * 62), _guarded(B * 1280), _guarded(int(m._lib.syn_synergy_flat_count()))
    abi.check(m._lib.syn_synergy_losses_backward_weights(m._h, pt.data_ptr(), tt.data_ptr(), pot.data_ptr(), B,
                                                         gst.data_ptr() if gs is not None else None, gpt.data_ptr() if gs is not None else None,
                                                         p0 if data else None, p1 if data else None, p2, m._stream()))
    dp, dpo = _inside(w0), _inside(w1)
    if not data:
        assert (dp == 7.0).all() and (dpo == 7.0).all()
    return _inside(w2).copy(), dp.reshape(B, 62).copy() if data else None, dpo.reshape(B, 1280).copy() if data else None


def _bwd(m, param, pool, target, gs=None, gp=None):
    B = param.shape[0]
    pt, pot, tt = _cuda(param), _cuda(pool), _cuda(target)
    gst, gpt = (_cuda(gs), _cuda(gp)) if gs is not None else (None, None)
    (w0, p0), (w1, p1) = _guarded(B * 62), _guarded(B * 1280)
    abi.check(m._lib.syn_synergy_losses_backward(m._h, pt.data_ptr(), tt.data_ptr(), pot.data_ptr(), B, gst.data_ptr() if gs is not None else None,
                                                 gpt.data_ptr() if gs is not None else None, p0, p1, m._stream()))
    return _inside(w0).reshape(B, 62).copy(), _inside(w1).reshape(B, 1280).copy()


def _one_hot(i, B):
    gs, gp = np.zeros(2, dtype=np.float32), np.zeros((3, B), dtype=np.float32)
    if i < 2:
        gs[i] = 1.0
    else:
        gp[i - 2] = np.float32(1.0) / np.float32(B)
    return gs, gp


def _running_slots_are_zero(flat):
    for k, (at, shape) in lw.flat_slices().items():
        if 'running_' in k:
            assert not flat[at:at + int(np.prod(shape))].any(), k


def _report(what, got_flat, want, keys=None):
    got = lw.split_flat(got_flat)
    e, at = lw.worst_rel(got, want, keys or lw.learnable_keys())
    print(f'{what}: worst tensor off by {e:.3g} x max |g| ({at}; bar {lw.TOL:g})')
    fam = {}
    for k in (keys or lw.learnable_keys()):                  # per family of tensors, for DESIGN 5.19
        name = ('conv ' if '.conv' in k else 'bn ') + k.rsplit('.', 1)[1]
        fam[name] = max(fam.get(name, 0.0), lw.worst_rel(got, want, [k])[0])
    print('    per family:', ', '.join(f'{n} {v:.2g}' for n, v in fam.items()))
    return e


# ------------------------------------------------------------------ 1. the recorded faces
def test_weight_gradients_match_the_recording_and_the_restatement(model, wgold, h64):
    param, pool, target = lg.graph_inputs()
    restated = h64.wgrads(param, pool, target)
    keys = lw.learnable_keys()
    for name in lw.RECORDED:
        i = (lc.LOSS_NAMES + ('total',)).index(name)
        flat, _, _ = _wbwd(model, param, pool, target, *(_one_hot(i, 5) if i < 5 else (None, None)))
        assert np.isfinite(flat).all()
        _running_slots_are_zero(flat)
        got = lw.split_flat(flat)
        rec_got = {k: lw.recorded_part(got[k]) for k in keys}
        rec_want = {k: wgold[lw.fixture_key(name, k)] for k in keys}
        e0, at0 = lw.worst_rel(rec_got, rec_want)
        print(f'{name}: worst tensor off by {e0:.3g} x max |g| from the recording ({at0})')
        e1 = _report(f'{name} against the float64 restatement', flat, restated[name])
        assert max(e0, e1) <= lw.TOL, name
    for i, name in enumerate(lc.LOSS_NAMES):                                    # the two losses that reach no weight: exactly 0
        if name in lw.ZERO_LOSSES:
            flat, _, _ = _wbwd(model, param, pool, target, *_one_hot(i, 5))
            assert not flat.any(), name


# ------------------------------------------------------------------ 2. batch sizes
@pytest.mark.parametrize('B', BATCH_SIZES)
def test_weight_gradients_at_batch_shapes(model, wgold, h64, B):
    param, pool, target = lw.wgrad_inputs(wgold['wgrad_faces'], B)
    gs, gp = lg.head_upstream(B)
    flat, dp, dpo = _wbwd(model, param, pool, target, gs, gp)
    assert np.isfinite(flat).all()
    e = _report(f'B {B}, random upstream', flat, h64.wvjp(param, pool, target, gs, gp))
    flat0, _, _ = _wbwd(model, param, pool, target, data=False)
    e0 = _report(f'B {B}, loss_total (NULL / NULL)', flat0, h64.wvjp(param, pool, target, *lw.total_upstream(B)))
    assert max(e, e0) <= lw.TOL
    want = _bwd(model, param, pool, target, gs, gp)                             # the data gradients keep the existing entry's bits
    assert dp.tobytes() == want[0].tobytes() and dpo.tobytes() == want[1].tobytes()


# ------------------------------------------------------------------ 3. pass boundary (child process: the knob is read once)
CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import loss_wgrad_cases as lw
import test_gpu_loss_wgrad as t
from synergynet_amd import synth
from synergynet_amd.synergy3DMM import SynergyNet
g = dict(np.load(sys.argv[3], allow_pickle=False))
pack = synth.make_3dmm(int(g['seeds'][1]))
w = dict(np.load(lw.GOLDEN, allow_pickle=False))
m = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_backbone_state(int(g['seeds'][0])))
m.load_synergy_state(synth.make_synergy_state(int(w['graph_seed'])))
param, pool, target = lw.wgrad_inputs(w['wgrad_faces'], int(sys.argv[5]))
flat, dp, dpo = t._wbwd(m, param, pool, target)
np.savez(sys.argv[4], flat=flat, dp=dp, dpo=dpo)
'''


@pytest.mark.parametrize('knobs,B', [('wgrad_pass=4', 9), ('wgrad_chunk=2', 3), ('wgrad_pass=4,wgrad_chunk=3', 9)])
def test_passes_and_chunks_accumulate_in_order(model, wgold, h64, tmp_path, knobs, B):
    """wgrad_pass = 4 and B = 9: passes of 4, 4 and 1 faces.  wgrad_chunk = 2 and B = 3: the per-point products of a pass are cut into
    chunks of 2 and 1 faces whose partial sums are folded in chunk order.  Both together: chunks of 3 and 1 faces in each pass of 4."""
    out = str(tmp_path / 'child.npz')
    env = dict(os.environ, SYNERGY_HIP_TEST_KNOBS=knobs)
    from conftest import ROOT
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT, os.path.join(ROOT, 'tests'), os.path.join(lg.HERE, 'golden', 'reference_outputs.npz'), out,
                        str(B)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    child = np.load(out)
    param, pool, target = lw.wgrad_inputs(wgold['wgrad_faces'], B)
    e = _report(knobs, child['flat'], h64.wvjp(param, pool, target, *lw.total_upstream(B)))
    assert e <= lw.TOL
    flat, dp, dpo = _wbwd(model, param, pool, target)
    assert child['dp'].tobytes() == dp.tobytes() and child['dpo'].tobytes() == dpo.tobytes()
    print(knobs, 'against the defaults: d_flat bits equal:', child['flat'].tobytes() == flat.tobytes(),
          'worst %.3g x max |g|' % lw.worst_rel(lw.split_flat(child['flat']), lw.split_flat(flat), lw.learnable_keys())[0])


# ------------------------------------------------------------------ 4. additivity across faces
def test_weight_gradient_is_additive_across_faces(model, wgold):
    param, pool, target = lw.wgrad_inputs(wgold['wgrad_faces'], 7)
    gs, gp = np.zeros(2, dtype=np.float32), lg.head_upstream(7)[1]              # no count couples the faces
    joint, _, _ = _wbwd(model, param, pool, target, gs, gp)
    a, _, _ = _wbwd(model, param[:3], pool[:3], target[:3], gs, np.ascontiguousarray(gp[:, :3]))
    b, _, _ = _wbwd(model, param[3:], pool[3:], target[3:], gs, np.ascontiguousarray(gp[:, 3:]))
    e = _report('faces 0-2 + faces 3-6 against the joint call', (a.astype(np.float64) + b), lw.split_flat(joint))
    assert e <= lw.TOL


# ------------------------------------------------------------------ 5. bit identities
def test_same_bits_on_every_call_and_every_handle_and_the_existing_entry_is_untouched(model, second, wgold):
    param, pool, target = lw.wgrad_inputs(wgold['wgrad_faces'], 9)
    before = _bwd(model, param, pool, target)
    first = _wbwd(model, param, pool, target)
    for m in (model, second, model):
        again = _wbwd(m, param, pool, target)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, first))
    assert first[1].tobytes() == before[0].tobytes() and first[2].tobytes() == before[1].tobytes()
    alone, _, _ = _wbwd(model, param, pool, target, data=False)                 # d_param / d_pool NULL: the same d_flat
    assert alone.tobytes() == first[0].tobytes()
    after = _bwd(model, param, pool, target)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()


# ------------------------------------------------------------------ 6. conventions
def test_a_tie_of_the_max_pool_goes_to_the_first_point(pack, backbone_sd, wgold, sd):
    import torch
    from synergynet_amd.synergy3DMM import SynergyNet
    ggold = dict(np.load(lg.GOLDEN, allow_pickle=False))
    tpack, tsd, param, pool, target = lg.tie_case(pack, sd, ggold['batch_faces'])
    first = lw.WHead(tpack, tsd).wgrads(param, pool, target, ('total',))['total']
    last = lw.WHead(tpack, tsd).wgrads(param, pool, target, ('total',), max_last=True)['total']
    f32 = lw.WHead(tpack, tsd, torch.float32).wgrads(param, pool, target, ('total',))['total']
    front = [f'forwardDirection.{c}{i}.{t}' for i in range(1, 6) for c, t in (('conv', 'weight'), ('conv', 'bias'), ('bn', 'weight'), ('bn', 'bias'))]
    assert lw.worst_rel(f32, first, front)[0] <= lw.CPU_BAR
    # the tied points have the same activations in every layer, so conv5 .. conv2 get the same weight gradient from either routing;
    # conv1's input is the landmark itself, whose x and y differ between the tied points: its columns 0:2 tell the routings apart
    where = 'forwardDirection.conv1.weight'
    moved = lg.rel_to_max(last[where], first[where])
    print('routing to the last maximum moves %s by %.3g x max |g| (conv5.weight by %.3g)' %
          (where, moved, lg.rel_to_max(last['forwardDirection.conv5.weight'], first['forwardDirection.conv5.weight'])))
    assert moved > 10 * lw.TOL
    m = SynergyNet(device='cuda:0', pack=tpack, backbone_state=backbone_sd)
    m.load_synergy_state(tsd)
    flat, _, _ = _wbwd(m, param, pool, target)
    got = lw.split_flat(flat)
    e = _report('tie, conv5 and the tensors in front of it against first-maximum routing', flat, first, front)
    away = lg.rel_to_max(got[where], last[where])
    print('tie: %s is %.3g x max |g| away from last-maximum routing' % (where, away))
    assert e <= lw.TOL and away > 10 * lw.TOL
    assert lg.rel_to_max(got[where].reshape(-1), wgold['tie|' + where]) <= lw.TOL
    rec = wgold['tie|forwardDirection.conv5.weight']
    assert lg.rel_to_max(lw.recorded_part(got['forwardDirection.conv5.weight'], lw.TIE_SAMPLE), rec) <= lw.TOL


def test_nan_target_is_not_counted_and_an_identical_face_is_nan_where_torch_has_it(model, wgold, h64):
    param, pool, target = lw.wgrad_inputs(wgold['wgrad_faces'], 5)
    # loss_LMK_pointNet alone with a NaN in one target row: that landmark element is not counted; no NaN reaches d_flat
    t2 = target.copy()
    t2[1, 3] = np.nan                                                           # an offset entry: NaN in one landmark row of that face
    gs, gp = np.array([0, 1], dtype=np.float32), np.zeros((3, 5), dtype=np.float32)
    flat, _, _ = _wbwd(model, param, pool, t2, gs, gp)
    assert np.isfinite(flat).all()
    e = _report('NaN target element, loss_LMK_pointNet', flat, h64.wvjp(param, pool, t2, gs, gp))
    assert e <= lw.TOL
    # a face whose param equals its target: loss_Param_In is NaN for its row of d param, and reaches no weight
    t3 = target.copy()
    t3[2] = param[2]
    flat, dp, _ = _wbwd(model, param, pool, t3)
    want = h64.wvjp(param, pool, t3, *lw.total_upstream(5))
    got = lw.split_flat(flat)
    nan_keys = [k for k in lw.learnable_keys() if np.isnan(want[k]).any()]
    print('identical face: torch has NaN in', nan_keys or 'no weight gradient', '; the device in',
          [k for k in lw.learnable_keys() if np.isnan(got[k]).any()] or 'none')
    for k in lw.learnable_keys():
        assert lg.same_classes(got[k], want[k]), k
    assert np.isnan(dp[2]).all()
    assert _report('identical face', flat, want) <= lw.TOL


# ------------------------------------------------------------------ 7. guards and refusals
def test_refusals_leave_the_outputs_untouched(model, second_unloaded, wgold):
    lib, s = model._lib, model._stream()
    param, pool, target = lw.wgrad_inputs(wgold['wgrad_faces'], 3)
    pt, pot, tt = _cuda(param), _cuda(pool), _cuda(target)
    gs, gp = (_cuda(a) for a in lg.head_upstream(3))
    (w0, p0), (w1, p1), (w2, p2) = _guarded(3 * 62), _guarded(3 * 1280), _guarded(int(lib.syn_synergy_flat_count()))
    P, T, PO, h = pt.data_ptr(), tt.data_ptr(), pot.data_ptr(), model._h
    for args in ((None, T, PO, 3, None, None, p0, p1, p2), (P, None, PO, 3, None, None, p0, p1, p2), (P, T, None, 3, None, None, p0, p1, p2),
                 (P, T, PO, 3, None, None, p0, p1, None), (P, T, PO, 0, None, None, p0, p1, p2), (P, T, PO, -2, None, None, p0, p1, p2),
                 (P, T, PO, 3, gs.data_ptr(), None, p0, p1, p2), (P, T, PO, 3, None, gp.data_ptr(), p0, p1, p2)):
        assert lib.syn_synergy_losses_backward_weights(h, *args, s) == abi.SYN_ERR_INVALID, args
        assert b'syn_synergy_losses_backward_weights' in lib.syn_last_error()
    assert lib.syn_synergy_losses_backward_weights(second_unloaded._h, P, T, PO, 3, None, None, p0, p1, p2, s) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_update_synergy_device(second_unloaded._h, p2, lib.syn_synergy_flat_count(), s) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_update_synergy_device(h, p2, 5, s) == abi.SYN_ERR_INVALID
    assert lib.syn_update_synergy_device(h, None, lib.syn_synergy_flat_count(), s) == abi.SYN_ERR_INVALID
    assert (_inside(w0) == 7.0).all() and (_inside(w1) == 7.0).all() and (_inside(w2) == 7.0).all()


@pytest.fixture(scope='module')
def second_unloaded(pack, backbone_sd):
    from synergynet_amd.synergy3DMM import SynergyNet
    return SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)


# ------------------------------------------------------------------ 8. syn_update_synergy_device
def test_update_on_the_device_equals_a_load_from_the_host(model, second, wgold):
    from synergynet_amd import synth
    other = synth.make_synergy_state(int(wgold['graph_seed']) + 1)
    flat = synth.flatten_synergy(other)
    param, pool, _ = lw.wgrad_inputs(wgold['wgrad_faces'], 5)
    try:
        second.load_synergy_state(other)
        want_l = second.refine_landmarks(param, pool).cpu().numpy()
        want_p = second.landmarks_to_param(second.refine_landmarks(param, pool)).cpu().numpy()
        dev = _cuda(flat)
        abi.check(model._lib.syn_update_synergy_device(model._h, dev.data_ptr(), dev.numel(), model._stream()))
        got_l = model.refine_landmarks(param, pool).cpu().numpy()
        got_p = model.landmarks_to_param(model.refine_landmarks(param, pool)).cpu().numpy()
        for what, g, w in (('refined landmarks', got_l, want_l), ('landmarks_to_param', got_p, want_p)):
            d = np.abs(g.astype(np.float64) - w).max() / np.abs(w).max()
            print(f'{what} after the device update: bit-equal to a host load: {g.tobytes() == w.tobytes()}, off by {d:.3g} x max |value|')
            assert d <= 1e-6
    finally:
        from synergynet_amd import synth as s2
        state = s2.make_synergy_state(int(wgold['graph_seed']))
        model.load_synergy_state(state)
        second.load_synergy_state(state)


# ------------------------------------------------------------------ 9. the Python surface
def test_python_surface(pack, backbone_sd, sd, wgold):
    import torch
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    m.load_synergy_state(sd)
    param, pool, target = lg.graph_inputs()
    # without synergy_parameters(): today's path
    p, po = _cuda(param).requires_grad_(True), _cuda(pool).requires_grad_(True)
    d0 = m.loss_head(p, po, target)
    sum(v.mean() for v in d0.values()).backward()
    base = (p.grad.clone(), po.grad.clone(), {k: v.detach().clone() for k, v in d0.items()})
    n_state, n_par = len(m.state_dict()), len(list(m.parameters()))
    ws = m.synergy_parameters()
    assert list(ws) == lw.learnable_keys() and all(isinstance(w, torch.nn.Parameter) and w.is_cuda for w in ws.values())
    assert all(tuple(ws[k].shape) == tuple(np.asarray(sd[k]).shape) for k in ws)
    assert len(m.state_dict()) == n_state and len(list(m.parameters())) == n_par            # not registered
    # gradients per key = the C call's slices, bit for bit; the input gradients are unchanged
    p, po = _cuda(param).requires_grad_(True), _cuda(pool).requires_grad_(True)
    d = m.loss_head(p, po, target)
    assert all(d[k].grad_fn is not None and torch.equal(d[k].detach(), base[2][k]) for k in lc.LOSS_NAMES)
    gs, gp = lg.head_upstream(5)
    (_cuda(gs)[0] * d['loss_LMK_f0'] + _cuda(gs)[1] * d['loss_LMK_pointNet'] + sum((_cuda(gp)[i] * d[k]).sum() for i, k in enumerate(lc.LOSS_NAMES[2:]))).backward()
    flat, dp, dpo = _wbwd(m, param, pool, target, gs, gp)
    got = lw.split_flat(flat)
    for k, w in ws.items():
        assert w.grad.cpu().numpy().tobytes() == got[k].tobytes(), k
    assert p.grad.cpu().numpy().tobytes() == dp.tobytes() and po.grad.cpu().numpy().tobytes() == dpo.tobytes()
    for w in ws.values():
        w.grad = None
    p, po = _cuda(param).requires_grad_(True), _cuda(pool).requires_grad_(True)
    sum(v.mean() for v in m.loss_head(p, po, target).values()).backward()
    assert torch.equal(p.grad, base[0]) and torch.equal(po.grad, base[1])
    # three SGD steps against the float64 restatement: the re-upload happens, and values stay put when nothing changed
    for w in ws.values():
        w.grad = None
    opt = torch.optim.SGD(list(ws.values()), lr=lw.SGD_LR)
    want = lw.WHead(pack, sd).sgd(param, pool, target)
    for step in range(lw.SGD_STEPS):
        opt.zero_grad()
        sum(v.mean() for v in m.loss_head(param, pool, target).values()).backward()
        opt.step()
        with torch.no_grad():
            a = [float(v.mean()) for v in m.loss_head(param, pool, target).values()]
            b = [float(v.mean()) for v in m.loss_head(param, pool, target).values()]      # nothing changed in between: the same values
        assert a == b
        rel = max(abs(x - y) / abs(y) for x, y in zip(a, want[step]))
        print(f'SGD step {step + 1}: five losses off by {rel:.3g} relative from the float64 restatement; total {sum(a):.6f} (was {float(sum(v.mean() for v in base[2].values())):.6f})')
        assert rel <= 1e-4
    assert sum(want[-1]) < float(sum(v.mean() for v in base[2].values()))                  # the steps did move the loss
    # the fine-tuned state round-trips
    state = m.synergy_state_dict()
    assert list(state) == [k for k, _ in lw.layers()]
    fresh = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    fresh.load_synergy_state(state)
    with torch.no_grad():
        x, y = m.loss_head(param, pool, target), fresh.loss_head(param, pool, target)
    for k in lc.LOSS_NAMES:
        d = float((x[k] - y[k]).abs().max() / y[k].abs().max())
        print(f'{k}: device-updated against freshly loaded state: bit-equal {torch.equal(x[k], y[k])}, off by {d:.3g}')
        assert d <= 1e-6
