"""GPU parity of the synergy refinement: syn_refine_points / syn_refine_landmarks / syn_landmarks_to_param through the C ABI and the
Python surface built on them, against the reference's recorded outputs (tests/golden/synergy_golden.npz, made by the reference's own
MLP_for / MLP_rev).  Bar: 1e-4 on conftest's two measures; batch independence and the device-resident chain are equality of bits.
Every output buffer starts poisoned (NaN)."""
import ctypes as C

import numpy as np
import pytest

import synergy_cases as sc
from conftest import rel_l2, rel_max
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

SIG = getattr(abi, '_SIGS')['syn_refine_points']                               # KeyError without the feature


@pytest.fixture(scope='module')
def sgold():
    return dict(np.load(sc.GOLDEN, allow_pickle=False))


@pytest.fixture(scope='module')
def model(sgold, pack, backbone_sd):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    assert not m.has_synergy
    m.load_synergy_state(synth.make_synergy_state(int(sgold['seed'])))
    assert m.has_synergy
    return m


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _poison(*shape):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def _refine_points(m, lmk, pool, param):
    """syn_refine_points on host arrays -> (lmk_refined, global_feat); the inputs are checked to be unmodified"""
    import torch
    B = lmk.shape[0]
    lt, pt, qt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (lmk, pool, param))
    out, gf = _poison(B, 3, 68), _poison(B, 1024)
    abi.check(m._lib.syn_refine_points(m._h, lt.data_ptr(), pt.data_ptr(), qt.data_ptr(), B, out.data_ptr(), gf.data_ptr(), m._stream()))
    got = out.cpu().numpy(), gf.cpu().numpy()
    assert _same(lt.cpu().numpy(), lmk) and _same(pt.cpu().numpy(), pool) and _same(qt.cpu().numpy(), param)
    return got


def _to_param(m, lmk):
    import torch
    B = lmk.shape[0]
    lt = torch.from_numpy(np.ascontiguousarray(lmk)).cuda()
    out = _poison(B, 62)
    abi.check(m._lib.syn_landmarks_to_param(m._h, lt.data_ptr(), B, out.data_ptr(), m._stream()))
    got = out.cpu().numpy()
    assert _same(lt.cpu().numpy(), lmk)
    return got


def _within_bar(name, got, want):
    e = (rel_l2(got, want), rel_max(got, want))
    print(name, 'rel_l2 %.3g rel_max %.3g' % e)
    assert np.isfinite(got).all(), name
    assert max(e) <= sc.BAR, (name, e)


@pytest.mark.parametrize('case', sc.CASES)
def test_golden_cases(model, sgold, case):
    g = lambda k: sgold[f'{case}_{k}']
    lr, gf = _refine_points(model, g('lmk_coarse'), g('pool'), g('param'))
    _within_bar(case + ' lmk_refined', lr, g('lmk_refined'))
    _within_bar(case + ' global_feat', gf, g('global_features'))
    _within_bar(case + ' param_rev', _to_param(model, g('lmk_refined')), g('param_rev'))


@pytest.fixture(scope='module')
def faces(sgold):
    """all nine golden faces in one pool: (lmk, pool, param, golden lmk_refined)"""
    cat = lambda k: np.concatenate([sgold[f'{c}_{k}'] for c in sc.CASES])
    return cat('lmk_coarse'), cat('pool'), cat('param'), cat('lmk_refined')


@pytest.fixture(scope='module')
def singles(model, faces):
    """every face alone (B = 1): the bits a batch must reproduce"""
    lmk, pool, param, lref = faces
    out = []
    for i in range(lmk.shape[0]):
        lr, gf = _refine_points(model, lmk[i:i + 1], pool[i:i + 1], param[i:i + 1])
        out.append((lr[0], gf[0], _to_param(model, lref[i:i + 1])[0]))
    return out


@pytest.mark.parametrize('B', sc.BATCH_SIZES)
def test_batch_sizes_bit_identical_to_single_faces(model, faces, singles, B):
    lmk, pool, param, lref = faces
    idx = np.arange(B) % lmk.shape[0]
    lr, gf = _refine_points(model, lmk[idx], pool[idx], param[idx])
    pr = _to_param(model, lref[idx])
    for k, i in enumerate(idx):
        assert _same(lr[k], singles[i][0]) and _same(gf[k], singles[i][1]) and _same(pr[k], singles[i][2]), (B, k, int(i))


@pytest.mark.parametrize('order', [(0, 1), (1, 0)])
def test_zero_face_next_to_an_ordinary_one_in_both_orders(model, sgold, singles, order):
    g = lambda k: sgold[f'c_{k}'][list(order)]
    lr, gf = _refine_points(model, g('lmk_coarse'), g('pool'), g('param'))
    _within_bar('c lmk_refined', lr, g('lmk_refined'))
    _within_bar('c global_feat', gf, g('global_features'))
    pr = _to_param(model, g('lmk_refined'))
    _within_bar('c param_rev', pr, g('param_rev'))
    first = 5 + 1                                                    # faces a (5) and b (1) precede case c in the pool
    for k, o in enumerate(order):
        assert _same(lr[k], singles[first + o][0]) and _same(gf[k], singles[first + o][1]) and _same(pr[k], singles[first + o][2])


@pytest.mark.parametrize('with_roi', [False, True])
def test_reconstruction_and_roi(model, sgold, with_roi):
    import torch
    param, pool, roi = sgold['a_param'], sgold['a_pool'], sgold['a_roi']
    B = param.shape[0]
    pt, qt, rt = (torch.from_numpy(a).cuda() for a in (param, pool, roi))
    coarse, refined, gf = _poison(B, 3, 68), _poison(B, 3, 68), _poison(B, 1024)
    abi.check(model._lib.syn_refine_landmarks(model._h, pt.data_ptr(), qt.data_ptr(), B, 1, rt.data_ptr() if with_roi else None,
                                              coarse.data_ptr(), refined.data_ptr(), gf.data_ptr(), model._stream()))
    want_c, want_r = sgold['a_lmk_coarse'], sgold['a_lmk_refined']
    if with_roi:
        want_c, want_r = sc.roi_affine(want_c, roi), sc.roi_affine(want_r, roi)
    _within_bar('lmk_coarse', coarse.cpu().numpy(), want_c)
    _within_bar('lmk_refined', refined.cpu().numpy(), want_r)
    _within_bar('global_feat', gf.cpu().numpy(), sgold['a_global_features'])
    lmk, _ = model.landmarks_and_pose(pt, roi=rt if with_roi else None, transform=True)
    assert _same(coarse.cpu().numpy(), lmk.cpu().numpy())
    assert _same(pt.cpu().numpy(), param) and _same(qt.cpu().numpy(), pool) and _same(rt.cpu().numpy(), roi)
    # the Python method is the same call
    r2, c2 = model.refine_landmarks(pt, qt, roi=rt if with_roi else None, return_coarse=True)
    assert _same(r2.cpu().numpy(), refined.cpu().numpy()) and _same(c2.cpu().numpy(), coarse.cpu().numpy())


def test_forward_synergy_equals_the_three_calls(model):
    import torch
    from synergynet_amd import synth
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(4, seed=3))).cuda()
    out = model.forward_synergy(x)
    param, pool = model.forward_test(x, return_pool=True)
    refined, coarse = model.refine_landmarks(param, pool, return_coarse=True)
    prev = model.landmarks_to_param(refined)
    n = lambda t: t.cpu().numpy()
    assert sorted(out) == ['lmk', 'lmk_refined', 'param', 'param_rev'] and all(v.is_cuda for v in out.values())
    assert _same(n(out['param']), n(param)) and _same(n(out['lmk']), n(coarse))
    assert _same(n(out['lmk_refined']), n(refined)) and _same(n(out['param_rev']), n(prev))
    assert np.isfinite(n(out['param_rev'])).all() and (n(out['lmk_refined']) >= n(out['lmk'])).all()      # the residual is relu'd
    assert _same(n(model.refine_points(coarse, pool, param)), n(refined))


def test_get_all_outputs_refine(model, monkeypatch):
    from synergynet_amd import synth
    frame = synth.make_frame(360, 480, seed=5)
    rects = lambda: [[40.0, 30.0, 220.0, 230.0, 0.99], [250.0, 100.0, 400.0, 260.0, 0.98]]
    plain = model.get_all_outputs(frame, rects())
    off = model.get_all_outputs(frame, rects(), refine=False)
    for i in range(2):                                                             # refine=False is today's path, byte for byte
        assert _same(plain[0][i], off[0][i]) and _same(plain[1][i], off[1][i])
        assert plain[2][i][0] == off[2][i][0] and _same(plain[2][i][1], off[2][i][1])
    assert len(plain[0]) == len(off[0]) == len(plain[1]) == len(off[1]) == 2
    seen = {}
    real_fwd, real_ref = model.forward_crops_u8, model.refine_landmarks

    def spy_fwd(crops, return_pool=False):
        r = real_fwd(crops, return_pool=return_pool)
        seen['param'], seen['pool'] = r
        return r

    def spy_ref(param, pool, roi=None, **kw):
        seen['roi'] = roi
        return real_ref(param, pool, roi=roi, **kw)
    monkeypatch.setattr(model, 'forward_crops_u8', spy_fwd)
    monkeypatch.setattr(model, 'refine_landmarks', spy_ref)
    on = model.get_all_outputs(frame, rects(), refine=True)
    monkeypatch.undo()
    want = model.refine_landmarks(seen['param'], seen['pool'], roi=seen['roi'], transform=True).cpu().numpy()
    assert all(_same(on[0][i], want[i]) for i in range(2))
    assert not any(_same(on[0][i], plain[0][i]) for i in range(2))                 # the first list did change ...
    assert all(_same(on[1][i], plain[1][i]) for i in range(2))                     # ... meshes and poses did not
    for i in range(2):
        assert on[2][i][0] == plain[2][i][0] and _same(on[2][i][1], plain[2][i][1])


def test_errors(model, sgold, pack):
    import torch
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    lib = model._lib
    bare = SynergyNet(device='cuda:0', load_constants=False)
    lt, pt, qt = (torch.from_numpy(sgold[f'd_{k}']).cuda() for k in ('lmk_coarse', 'pool', 'param'))
    out = _poison(1, 3, 68)
    for call in (lambda: lib.syn_refine_points(bare._h, lt.data_ptr(), pt.data_ptr(), qt.data_ptr(), 1, out.data_ptr(), None, bare._stream()),
                 lambda: lib.syn_refine_landmarks(bare._h, qt.data_ptr(), pt.data_ptr(), 1, 1, None, None, out.data_ptr(), None, bare._stream()),
                 lambda: lib.syn_landmarks_to_param(bare._h, lt.data_ptr(), 1, out.data_ptr(), bare._stream())):
        assert call() == abi.SYN_ERR_NOT_LOADED
        assert b'synergy weights not loaded' in lib.syn_last_error()
    assert lib.syn_refine_points(model._h, lt.data_ptr(), pt.data_ptr(), qt.data_ptr(), 0, out.data_ptr(), None, model._stream()) == abi.SYN_ERR_INVALID
    assert lib.syn_refine_points(model._h, None, pt.data_ptr(), qt.data_ptr(), 1, out.data_ptr(), None, model._stream()) == abi.SYN_ERR_INVALID
    assert b'NULL' in lib.syn_last_error()
    assert lib.syn_landmarks_to_param(model._h, lt.data_ptr(), 1, None, model._stream()) == abi.SYN_ERR_INVALID
    assert torch.isnan(out).all()                                                  # nothing was written by the refused calls
    with pytest.raises(RuntimeError, match='synergy weights not loaded'):
        bare.get_all_outputs(synth.make_frame(64, 64, seed=1), [[4.0, 4.0, 60.0, 60.0, 0.9]], refine=True)
    with pytest.raises(RuntimeError, match='synergy weights not loaded'):
        bare.refine_points(lt, pt, qt)
    rn = SynergyNet(device='cuda:0', load_constants=False, arch='resnet50')
    rn.load_synergy_state(synth.make_synergy_state(int(sgold['seed'])))
    with pytest.raises(RuntimeError, match='1280-d pooled feature'):
        rn.refine_points(lt, pt, qt)
    # the C entry refuses a handle whose backbone is resnet50 by itself (include/synergy_hip.h)
    rn50 = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_resnet50_state(), arch='resnet50')
    rn50.load_synergy_state(synth.make_synergy_state(int(sgold['seed'])))
    assert lib.syn_refine_points(rn50._h, lt.data_ptr(), pt.data_ptr(), qt.data_ptr(), 1, out.data_ptr(), None, rn50._stream()) == abi.SYN_ERR_INVALID
    assert b'1280-d pooled feature' in lib.syn_last_error() and b'resnet50' in lib.syn_last_error()
    assert lib.syn_landmarks_to_param(rn50._h, lt.data_ptr(), 1, out.data_ptr(), rn50._stream()) == abi.SYN_ERR_INVALID
    assert torch.isnan(out).all()
    # overlapping outputs of syn_refine_landmarks
    two = _poison(2, 3, 68)
    assert lib.syn_refine_landmarks(model._h, qt.data_ptr(), pt.data_ptr(), 1, 1, None, two.data_ptr(), two.data_ptr(), None, model._stream()) == abi.SYN_ERR_INVALID
    assert b'overlaps' in lib.syn_last_error() and torch.isnan(two).all()
    with pytest.raises(RuntimeError, match='1280-d pooled feature'):
        rn.get_all_outputs(synth.make_frame(64, 64, seed=1), [[4.0, 4.0, 60.0, 60.0, 0.9]], refine=True)
