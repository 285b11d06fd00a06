"""GPU parity of the losses of the training graph's forward (syn_wing_loss / syn_param_loss / syn_synergy_losses, SynergyNet.forward /
validate) and of CenterCrop / extract_param, against the reference's recorded results (tests/golden/loss_golden.npz) and the float64
restatement of tests/loss_cases.py.  Bar: 1e-4 relative (TOL of tests/test_gpu_parity.py); NaN / inf by class; the exact zero with ==;
fixed-order and batch-independence claims are equality of bits.  The graph-level bar is derived in test_graph_losses_match_the_recording.
Figures are printed before they are asserted."""

import numpy as np
import pytest

import loss_cases as lc
from conftest import rel_max
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

SIG = getattr(abi, '_SIGS')['syn_synergy_losses']                              # KeyError without the feature


@pytest.fixture(scope='module')
def lgold():
    return dict(np.load(lc.GOLDEN, allow_pickle=False))


def _with_synergy(m, lgold):
    from synergynet_amd import synth
    m.load_synergy_state(synth.make_synergy_state(int(lgold['graph_seed'])))
    return m


@pytest.fixture(scope='module')
def model(lgold, pack, backbone_sd):
    from synergynet_amd.synergy3DMM import SynergyNet
    return _with_synergy(SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd), lgold)


@pytest.fixture(scope='module')
def ghost(lgold, pack):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    return _with_synergy(SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_ghostnet_state(), arch='ghostnet'), lgold)


@pytest.fixture(scope='module')
def models(model, ghost):
    return {'mobilenet_v2': model, 'ghostnet': ghost}


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(shape, value=7.0, dtype=None):
    import torch
    return torch.full(shape, value, dtype=dtype or torch.float32, device='cuda')


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _wing(m, pred, target, omega=10.0, epsilon=2.0):
    """syn_wing_loss through the C ABI on host arrays -> the float"""
    pt, tt = _cuda(pred), _cuda(target)
    out = _filled((1,), float('nan'))
    abi.check(m._lib.syn_wing_loss(m._h, pt.data_ptr(), tt.data_ptr(), pred.shape[0], pred.shape[2], omega, epsilon, out.data_ptr(), m._stream()))
    return out.cpu().numpy()[0]


def _param(m, a, b, mode):
    at, bt = _cuda(a), _cuda(b)
    out = _filled((a.shape[0],), float('nan'))
    abi.check(m._lib.syn_param_loss(m._h, at.data_ptr(), bt.data_ptr(), a.shape[0], mode, out.data_ptr(), m._stream()))
    return out.cpu().numpy()


# ---- kernel level ----
@pytest.mark.parametrize('name', lc.wing_case_names())
def test_wing_loss_matches_the_recording_and_the_restatement(model, lgold, name):
    B, n, v = lc.parse_wing_case(name)
    pred, target = lc.wing_inputs(B, n, v)
    got, want, restated = _wing(model, pred, target), lgold[name], lc.wing(pred, target)
    print(name, 'got', got, 'recorded', want, 'restated', restated)
    assert got.dtype == np.float32
    assert lc.same_class(got, want) and lc.same_class(got, restated), name
    if np.isfinite(want):
        e = (_rel(got, want), _rel(got, restated))
        print(name, 'rel to the recording %.3g, to the restatement %.3g' % e)
        assert max(e) <= lc.TOL
    # the Python method is the same call
    assert model.wing_loss(pred, target).cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize('B', lc.PARAM_B)
@pytest.mark.parametrize('mode', ['normal', 'only_3dmm'])
def test_param_loss_matches_the_recording_and_the_restatement(model, lgold, B, mode):
    for same in (False, True):
        a, b = lc.param_inputs(B, same)
        got = _param(model, a, b, ('normal', 'only_3dmm').index(mode))
        want, restated = lgold[f'param_B{B}_{mode}' + ('_same' if same else '')], lc.param_loss(a, b, mode)
        e = (_rel(got, want), _rel(got, restated))
        print(B, mode, same, 'rel to the recording %.3g, to the restatement %.3g' % e)
        assert got.shape == (B,) and max(e) <= lc.TOL
        if same and mode == 'normal':
            assert (got == 0).all()                                            # input == target: exactly 0
        assert model.param_loss(a, b, mode=mode).cpu().numpy().tobytes() == got.tobytes()


# ---- fixed order ----
def test_param_loss_of_a_face_has_the_same_bits_alone_and_anywhere_in_a_batch(model):
    import torch
    a, b = lc.param_inputs(257)
    for mode in (0, 1):
        alone = _param(model, a[100:101], b[100:101], mode)
        for pos in (0, 128, 256):
            a2, b2 = a.copy(), b.copy()
            a2[pos], b2[pos] = a[100], b[100]
            assert torch.equal(torch.from_numpy(_param(model, a2, b2, mode)[pos:pos + 1]), torch.from_numpy(alone)), (mode, pos)


def test_wing_loss_has_the_same_bits_on_every_call_and_every_handle(model, ghost):
    for B, n in ((1025, 68), (257, 1), (1, 1), (2571, 68)):                     # the last: 257 chunks of 2048 for 256 folding threads
        pred, target = lc.wing_inputs(B, n)
        first = _wing(model, pred, target)
        assert _rel(first, lc.wing(pred, target)) <= lc.TOL, (B, n)
        for m in (model, model, ghost, model, ghost):
            assert _wing(m, pred, target).tobytes() == first.tobytes(), (B, n)


# ---- graph level ----
def _graph_inputs(lgold):
    return tuple(_cuda(lgold['graph_' + k]) for k in ('param', 'target', 'pool'))


def _synergy_losses(m, param, target, pool, meter=None):
    B = param.shape[0]
    scalars, per_face = _filled((2,), float('nan')), _filled((3, B), float('nan'))
    abi.check(m._lib.syn_synergy_losses(m._h, param.data_ptr(), target.data_ptr(), pool.data_ptr(), B, scalars.data_ptr(), per_face.data_ptr(),
                                        meter.data_ptr() if meter is not None else None, m._stream()))
    s, p = scalars.cpu().numpy(), per_face.cpu().numpy()
    return dict(zip(lc.LOSS_NAMES, (s[0], s[1], p[0], p[1], p[2])))


@pytest.mark.parametrize('arch', ['mobilenet_v2', 'ghostnet'])
def test_graph_losses_match_the_recording(models, lgold, arch):
    """The losses are functions of the graph's intermediates, which differ from the reference's by the landmark and MLP parity errors.
    WingLoss is (omega / eps) = 5-Lipschitz in the max-norm of its landmarks, ParamLoss at most sqrt(2)-Lipschitz in the max-norm of its
    inputs, so   |loss - recorded| <= weight * Lipschitz * (largest deviation of the loss's inputs from the recorded intermediates,
    measured here) + 1e-4 |recorded|,   after the intermediates themselves passed the 1e-4 bar."""
    m = models[arch]
    g = lambda k: lgold['graph_' + k]
    param, target, pool = _graph_inputs(lgold)
    refined, lmk = m.refine_landmarks(param, pool, return_coarse=True)
    lmk_gt, _ = m.landmarks_and_pose(target, transform=True)
    param_rev = m.landmarks_to_param(refined)
    inter = dict(lmk=lmk, lmk_gt=lmk_gt, lmk_refined=refined, param_rev=param_rev)
    dev = {}
    for k, t in inter.items():
        got = t.cpu().numpy()
        dev[k] = float(np.abs(got.astype(np.float64) - g(k)).max())
        print(arch, k, 'rel_max %.3g, largest deviation %.3g' % (rel_max(got, g(k)), dev[k]))
        assert rel_max(got, g(k)) <= lc.TOL, k
    slack = dict(loss_LMK_f0=lc.WING_LIPSCHITZ * max(dev['lmk'], dev['lmk_gt']),
                 loss_LMK_pointNet=lc.WING_LIPSCHITZ * max(dev['lmk_refined'], dev['lmk_gt']),
                 loss_Param_In=0.0, loss_Param_S2=lc.PARAM_LIPSCHITZ * dev['param_rev'], loss_Param_S1S2=lc.PARAM_LIPSCHITZ * dev['param_rev'])
    got = _synergy_losses(m, param, target, pool)
    restated = lc.graph_losses(g('param'), g('target'), *(inter[k].cpu().numpy() for k in ('lmk', 'lmk_gt', 'lmk_refined', 'param_rev')))
    for name, w, r in zip(lc.LOSS_NAMES, lc.WEIGHTS, restated):
        want = g(name)
        err = float(np.abs(np.asarray(got[name], dtype=np.float64) - want).max())
        bar = w * slack[name] + lc.TOL * float(np.abs(want).max())
        print(arch, name, 'error %.3g, bar %.3g; rel to the restatement on the device intermediates %.3g' % (err, bar, _rel(got[name], r)))
        assert got[name].shape == want.shape and np.isfinite(got[name]).all()
        assert err <= bar, name
        assert _rel(got[name], r) <= lc.TOL, name


@pytest.mark.parametrize('B', [8, 9, 37, 2049])
def test_graph_losses_across_workgroups(model, lgold, B):
    """kLossFaces = 8 faces per workgroup: one full workgroup, one face more, several with a ragged tail, and 257 chunk sums for the 256
    threads that fold them.  The recorded faces repeat; the scalars are held to the restatement on the device's own intermediates, the
    per-face losses to the bits of the 5-face call, the meter to its documented words."""
    import torch
    idx = torch.arange(B, device='cuda') % 5
    param, target, pool = (t[idx].contiguous() for t in _graph_inputs(lgold))
    five = _synergy_losses(model, *_graph_inputs(lgold))
    meter = torch.zeros(8, dtype=torch.float64, device='cuda')
    got = _synergy_losses(model, param, target, pool, meter=meter)
    again = _synergy_losses(model, param, target, pool, meter=meter)
    refined, lmk = model.refine_landmarks(param, pool, return_coarse=True)
    lmk_gt, _ = model.landmarks_and_pose(target, transform=True)
    n = lambda t: t.cpu().numpy()
    restated = lc.graph_losses(n(param), n(target), n(lmk), n(lmk_gt), n(refined), n(model.landmarks_to_param(refined)))
    for name, r in zip(lc.LOSS_NAMES, restated):
        print(B, name, 'rel to the restatement %.3g' % _rel(got[name], r))
        assert _rel(got[name], r) <= lc.TOL, name
        assert got[name].tobytes() == again[name].tobytes(), name
    for name in lc.LOSS_NAMES[2:]:
        assert got[name].tobytes() == five[name][n(idx)].tobytes(), name
    mw = meter.cpu().numpy()
    means = [float(np.mean(np.asarray(got[k], dtype=np.float64))) for k in lc.LOSS_NAMES]
    for i in range(5):
        assert abs(mw[i] - 2 * B * means[i]) <= 1e-12 * abs(mw[i]), i
    assert abs(mw[5] - 2 * B * sum(means)) <= 1e-12 * abs(mw[5]) and mw[6] == 2 * B and mw[7] == 2


@pytest.mark.parametrize('arch', ['mobilenet_v2', 'ghostnet'])
def test_forward_returns_the_reference_dict_from_device_arithmetic(models, arch):
    import torch
    from synergynet_amd import synth
    m = models[arch]
    crops = synth.make_crops(5, seed=3)
    x = torch.from_numpy(synth.normalize_crops(crops)).cuda()
    target = _cuda(synth.make_params(5, lc.SEED_GRAPH_TARGET))
    out = m(x, target)                                                         # through nn.Module.__call__
    assert list(out) == list(lc.LOSS_NAMES) == list(m.get_losses())
    assert all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
    assert [tuple(v.shape) for v in out.values()] == [(), (), (5,), (5,), (5,)]
    # the same bits as the C entry on the backbone's own outputs, and the restatement on the graph's tensors
    param, pool = m.forward_test(x, return_pool=True)
    direct = _synergy_losses(m, param, target, pool)
    syn = m.forward_synergy(x)
    lmk_gt = m.reconstruct(target, dense=False)
    n = lambda t: t.cpu().numpy()
    restated = lc.graph_losses(n(syn['param']), n(target), n(syn['lmk']), n(lmk_gt), n(syn['lmk_refined']), n(syn['param_rev']))
    for name, r in zip(lc.LOSS_NAMES, restated):
        assert n(out[name]).tobytes() == direct[name].tobytes(), name
        print(arch, name, 'rel to the restatement %.3g' % _rel(n(out[name]), r))
        assert _rel(n(out[name]), r) <= lc.TOL, name
    u8 = m.losses_crops_u8(crops, target)
    p8, pool8 = m.forward_crops_u8(crops, return_pool=True)
    d8 = _synergy_losses(m, p8, target, pool8)
    assert all(n(u8[k]).tobytes() == d8[k].tobytes() for k in lc.LOSS_NAMES)
    # a face's per-face losses do not depend on the batch it is in
    for i in (0, 3, 4):
        one = _synergy_losses(m, param[i:i + 1].contiguous(), target[i:i + 1].contiguous(), pool[i:i + 1].contiguous())
        for k in lc.LOSS_NAMES[2:]:
            assert torch.equal(torch.from_numpy(one[k]), torch.from_numpy(direct[k][i:i + 1])), (k, i)


# ---- meter ----
def test_validate_is_the_average_meter_over_the_batches(model):
    """AverageMeter.update(mean, B): every batch's MEAN weighs in with the batch size.  For the per-face losses that is the mean over all
    134 faces, whatever the batching; the two landmark losses are means over a batch's elements already, so batches of 3, 1 and 130 give
    (3 L_a + 1 L_b + 130 L_c) / 134 -- not the landmark loss of one batch of 134, whose NaN-free count and branch shares differ."""
    import torch
    from synergynet_amd import synth
    sizes = (3, 1, 130)
    crops = torch.from_numpy(synth.make_crops(134, seed=11)).cuda()
    target = _cuda(synth.make_params(134, 177))
    cuts = np.cumsum((0,) + sizes)
    batches = [(crops[a:b], target[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    got = model.validate(batches)
    dicts = [{k: v.cpu().numpy() for k, v in model.losses_crops_u8(c, t).items()} for c, t in batches]
    want = lc.average_meter(dicts, sizes)
    assert list(got) == list(lc.LOSS_NAMES) + ['loss_total']
    for k in got:
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    whole = {k: v.cpu().numpy() for k, v in model.losses_crops_u8(crops, target).items()}
    one = model.validate([(crops, target)])
    for k in lc.LOSS_NAMES[2:]:                # per-face losses: batching does not matter (beyond the backbone's schedule, which may
        assert abs(one[k] - float(np.mean(whole[k].astype(np.float64)))) <= 1e-12 * abs(one[k]), k     # change with the batch size)
        assert abs(got[k] - one[k]) <= lc.TOL * abs(got[k]), k
    for k in lc.LOSS_NAMES[:2]:                # landmark losses: batch means weighted by batch size -- not the loss of the one batch
        assert abs(one[k] - float(whole[k])) <= 1e-12 * abs(one[k]), k
        print(k, 'three batches', got[k], 'one batch', one[k])
    # float input goes through forward, the meter words are the documented ones
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(4, seed=3))).cuda()
    meter = torch.zeros(8, dtype=torch.float64, device='cuda')
    d1, d2 = model(x, target[:4], meter=meter), model(x[:2], target[:2], meter=meter)
    mw = meter.cpu().numpy()
    means = [[float(np.mean(v.cpu().numpy().astype(np.float64))) for v in d.values()] for d in (d1, d2)]
    for i in range(5):
        assert abs(mw[i] - (means[0][i] * 4 + means[1][i] * 2)) <= 1e-12 * abs(mw[i])
    assert abs(mw[5] - (sum(means[0]) * 4 + sum(means[1]) * 2)) <= 1e-12 * abs(mw[5]) and mw[6] == 6 and mw[7] == 2


# ---- CenterCrop / extract_param ----
def _crop(m, img, margin, in_place=False):
    """syn_center_crop_u8 between 64 guard words on either side of `out` -> (result, guards untouched)"""
    import torch
    n = img.size
    buf = torch.full((256 + n + 256,), 0xA5, dtype=torch.uint8, device='cuda')
    out = buf[256:256 + n]
    src = out if in_place else _cuda(img).reshape(-1)
    if in_place:
        out.copy_(_cuda(img).reshape(-1))
    B, H, W, Cn = img.shape
    abi.check(m._lib.syn_center_crop_u8(m._h, src.data_ptr(), B, H, W, Cn, margin, out.data_ptr(), m._stream()))
    host = buf.cpu().numpy()
    return host[256:256 + n].reshape(img.shape), bool((host[:256] == 0xA5).all() and (host[256 + n:] == 0xA5).all())


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('margin', lc.CROP_MARGINS)
def test_center_crop_is_the_recording_bit_for_bit(model, lgold, margin, in_place):
    got, guards = _crop(model, lc.ramp(), margin, in_place)
    assert guards
    assert np.array_equal(got[0], lgold[f'crop_m{margin}'])
    if margin >= 59:
        assert int(got.any(3).sum()) == (4 if margin == 59 else 0)


@pytest.mark.parametrize('shape', [(3, 7, 5, 3), (2, 9, 13, 1), (1, 1, 1, 1), (5, 120, 120, 3)])
def test_center_crop_odd_shapes_and_unaligned_buffers(model, shape):
    import torch
    img = lc.ramp(*shape)
    for margin in (0, 1, 2, 4):
        got, guards = _crop(model, img, margin)
        assert guards and np.array_equal(got, lc.center_crop(img, margin)), (shape, margin)
    # buffers that start at an odd address take the byte path
    n = img.size
    src, dst = torch.zeros(n + 3, dtype=torch.uint8, device='cuda'), torch.full((n + 8,), 0xA5, dtype=torch.uint8, device='cuda')
    src[1:1 + n] = _cuda(img).reshape(-1)
    B, H, W, Cn = shape
    abi.check(model._lib.syn_center_crop_u8(model._h, src.data_ptr() + 1, B, H, W, Cn, 1, dst.data_ptr() + 3, model._stream()))
    host = dst.cpu().numpy()
    assert np.array_equal(host[3:3 + n].reshape(shape), lc.center_crop(img, 1)) and (host[:3] == 0xA5).all() and (host[3 + n:] == 0xA5).all()


def test_extract_param_and_benchmark(model, golden):
    import torch
    from synergynet_amd import evaluate, synth
    crops = synth.make_crops(130, seed=21)                                     # 128 + a ragged batch of 2
    zeroed = lc.center_crop(crops, 5)
    assert not np.array_equal(zeroed, crops)
    assert torch.equal(evaluate.center_crop(model, crops, 5).cpu(), torch.from_numpy(zeroed))
    got = evaluate.extract_param(model, crops, batch_size=128, center_crop=5)
    assert got.shape == (130, 62) and got.dtype == np.float32
    want = torch.cat([model.forward_crops_u8(zeroed[:128]), model.forward_crops_u8(zeroed[128:])]).cpu()
    assert torch.equal(torch.from_numpy(got), want)
    plain = evaluate.extract_param(model, crops, batch_size=128, center_crop=None)
    assert torch.equal(torch.from_numpy(plain), torch.cat([model.forward_crops_u8(crops[:128]), model.forward_crops_u8(crops[128:])]).cpu())
    assert not np.array_equal(plain, got)
    # crops through to the NME and FOE tuples
    rng = np.random.default_rng(5)
    pts = model.reconstruct(torch.from_numpy(got), dense=False).cpu().numpy() + rng.standard_normal((130, 3, 68)).astype(np.float32)
    roi = np.tile(np.array([0, 0, 120, 120, 1], dtype=np.float32), (130, 1))
    yaws, pose_gt, skip = rng.uniform(-90, 90, 130), rng.uniform(-30, 30, (128, 3)), [7, 99]
    nme, foe = evaluate.benchmark(model, crops, pts, roi, yaws, pose_gt, skip)
    assert nme == evaluate.benchmark_aflw2000_params(model, got, pts, roi, yaws) and len(nme) == 5 and np.isfinite(nme).all()
    assert foe == evaluate.benchmark_FOE(model, got, pose_gt, skip) and len(foe) == 4 and np.isfinite(foe).all()


# ---- refusals ----
def test_refusals_leave_the_outputs_untouched(model, lgold, pack):
    import torch
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    lib = model._lib
    param, target, pool = _graph_inputs(lgold)
    scalars, per_face, one = _filled((2,)), _filled((3, 5)), _filled((5,))
    meter = _filled((8,), dtype=torch.float64)
    s = model._stream()

    def losses(m, B=5, p=param, t=target, po=pool, sc=scalars, pf=per_face):
        ptr = lambda x: x.data_ptr() if x is not None else None
        return lib.syn_synergy_losses(m._h, ptr(p), ptr(t), ptr(po), B, ptr(sc), ptr(pf), meter.data_ptr(), m._stream())
    # a backbone whose pooled feature is not 1280-d
    rn = _with_synergy(SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_resnet_basic_state('resnet18'), arch='resnet18'), lgold)
    assert losses(rn) == abi.SYN_ERR_INVALID
    assert b'1280-d' in lib.syn_last_error() and b'resnet18' in lib.syn_last_error()
    assert b'(512-d)' in lib.syn_last_error()          # the width of the pool THIS handle has
    with pytest.raises(RuntimeError, match='1280-d'):
        rn(torch.zeros(1, 3, 120, 120), target[:1])
    # ... while the two modules on their own work with any backbone
    pred, tgt = lc.wing_inputs(3, 68)
    assert _wing(rn, pred, tgt).tobytes() == _wing(model, pred, tgt).tobytes()
    a, b = lc.param_inputs(3)
    assert _param(rn, a, b, 1).tobytes() == _param(model, a, b, 1).tobytes()
    # before syn_load_synergy
    bare = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_backbone_state())
    assert losses(bare) == abi.SYN_ERR_NOT_LOADED and b'synergy weights not loaded' in lib.syn_last_error()
    with pytest.raises(RuntimeError, match='synergy weights not loaded'):
        bare(torch.zeros(1, 3, 120, 120), target[:1])
    # bad arguments
    assert losses(model, B=0) == abi.SYN_ERR_INVALID and b'B=0' in lib.syn_last_error()
    assert losses(model, B=-3) == abi.SYN_ERR_INVALID
    for kw in (dict(p=None), dict(t=None), dict(po=None), dict(sc=None), dict(pf=None)):
        assert losses(model, **kw) == abi.SYN_ERR_INVALID and b'NULL' in lib.syn_last_error()
    assert lib.syn_param_loss(model._h, param.data_ptr(), target.data_ptr(), 5, 2, one.data_ptr(), s) == abi.SYN_ERR_INVALID
    assert b'mode=2' in lib.syn_last_error()
    assert lib.syn_param_loss(model._h, param.data_ptr(), target.data_ptr(), 0, 0, one.data_ptr(), s) == abi.SYN_ERR_INVALID
    assert lib.syn_param_loss(model._h, None, target.data_ptr(), 5, 0, one.data_ptr(), s) == abi.SYN_ERR_INVALID
    lm = _filled((5, 3, 68))
    assert lib.syn_wing_loss(model._h, lm.data_ptr(), lm.data_ptr(), 5, 0, 10.0, 2.0, one.data_ptr(), s) == abi.SYN_ERR_INVALID
    assert b'n_points=0' in lib.syn_last_error()
    assert lib.syn_wing_loss(model._h, lm.data_ptr(), lm.data_ptr(), 0, 68, 10.0, 2.0, one.data_ptr(), s) == abi.SYN_ERR_INVALID
    assert lib.syn_wing_loss(model._h, lm.data_ptr(), None, 5, 68, 10.0, 2.0, one.data_ptr(), s) == abi.SYN_ERR_INVALID
    assert lib.syn_wing_loss(model._h, lm.data_ptr(), lm.data_ptr(), 5, 68, 10.0, 0.0, one.data_ptr(), s) == abi.SYN_ERR_INVALID
    u8 = torch.full((4, 4, 3), 7, dtype=torch.uint8, device='cuda')
    assert lib.syn_center_crop_u8(model._h, u8.data_ptr(), 1, 4, 4, 3, -1, u8.data_ptr(), s) == abi.SYN_ERR_INVALID
    assert lib.syn_center_crop_u8(model._h, u8.data_ptr(), 0, 4, 4, 3, 1, u8.data_ptr(), s) == abi.SYN_ERR_INVALID
    assert lib.syn_center_crop_u8(model._h, u8.data_ptr(), 1, 4, 4, 3, 1, None, s) == abi.SYN_ERR_INVALID
    torch.cuda.synchronize()
    for t in (scalars, per_face, one, meter, lm):
        assert (t == 7.0).all()
    assert (u8 == 7).all()
    # mismatched shapes in Python
    x = torch.zeros(2, 3, 120, 120)
    with pytest.raises(RuntimeError, match='target must be'):
        model(x, target[:3])
    with pytest.raises(RuntimeError, match='target must be'):
        model(x, torch.zeros(2, 61))
    for bad in (torch.zeros(8, device='cuda'), torch.zeros(7, dtype=torch.float64, device='cuda'), torch.zeros(8, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match='meter must be'):
            model(x, target[:2], meter=bad)
    with pytest.raises(RuntimeError, match='target must have the shape of pred'):
        model.wing_loss(torch.zeros(2, 3, 68), torch.zeros(2, 3, 67))
    with pytest.raises(RuntimeError, match=r'pred must be \[B,3,n\]'):
        model.wing_loss(torch.zeros(2, 68), torch.zeros(2, 68))
    with pytest.raises(RuntimeError, match='same number of faces'):
        model.param_loss(torch.zeros(2, 62), torch.zeros(3, 62))
    with pytest.raises(RuntimeError, match='mode must be'):
        model.param_loss(torch.zeros(2, 62), torch.zeros(2, 62), mode='both')
    with pytest.raises(ValueError, match='uint8 crops'):
        from synergynet_amd import evaluate
        evaluate.extract_param(model, np.zeros((2, 120, 120, 3), dtype=np.float32))
