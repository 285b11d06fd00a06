"""GPU parity of the GhostNet backbone (arch = 'ghostnet'): the HIP path against the reference module's recorded outputs
(tests/golden/ghostnet_outputs.npz) and against the torch restatement of tests/ghostnet_cases.py, which tests/test_ghostnet_cpu.py
holds against the same recording -- never against the library itself.  Bar: rel_max < 1e-4 (TOL of tests/test_gpu_parity.py); the two
schedules of the network, both exact fp32 and summing in the same order, agree bit for bit."""
import os
import warnings

import numpy as np
import pytest

import ghostnet_cases as gc
from ghostnet_cases import TOL, rel_max

pytestmark = pytest.mark.gpu
SHAPES = gc.block_shapes()
FUSED_EXISTS = [b for b in range(16) if SHAPES[b]['hout'] <= 15]          # blocks with at least one fused GhostModule (3.0 onward)


@pytest.fixture(scope='module')
def state():
    from synergynet_amd import synth
    return synth.make_ghostnet_state(gc.SEED)


@pytest.fixture(scope='module')
def model(pack, state):
    """the model on the default schedule; constructing it must not warn (there is no range verdict to report)"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd.synergy3DMM import SynergyNet
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = SynergyNet(device='cuda:0', pack=pack, backbone_state=state, arch='ghostnet')
    assert m.arch == 'ghostnet' and m.pool_dim == 1280
    return m


@pytest.fixture(scope='module')
def per_layer_model(pack, state):
    """the per-layer schedule, selected the documented way"""
    from synergynet_amd.synergy3DMM import SynergyNet
    os.environ['SYNERGY_HIP_FUSION'] = '0'
    try:
        return SynergyNet(device='cuda:0', pack=pack, backbone_state=state, arch='ghostnet')
    finally:
        os.environ.pop('SYNERGY_HIP_FUSION', None)


_REF = {}


def _want(state, tag, x_norm, faces):
    """restatement outputs (param62, pool) of the given faces of a named input, computed once per face"""
    todo = [i for i in faces if (tag, i) not in _REF]
    if todo:
        out, pool = gc.ghostnet_forward(state, x_norm[todo])
        for k, i in enumerate(todo):
            _REF[tag, i] = (out[k, :62], pool[k])
    return np.stack([_REF[tag, i][0] for i in faces]), np.stack([_REF[tag, i][1] for i in faces])


def test_golden_parity(model):
    import torch
    from synergynet_amd import synth
    g = np.load(gc.GOLDEN)
    x = synth.normalize_crops(synth.make_crops(2, seed=int(g['crops_seed'])))
    param, pool = model.forward_test(torch.from_numpy(x).cuda(), return_pool=True)
    assert tuple(param.shape) == (2, 62) and tuple(pool.shape) == (2, 1280)
    e_param, e_pool = rel_max(param.cpu().numpy(), g['out102'][:, :62]), rel_max(pool.cpu().numpy(), g['pool'])
    print(f'param {e_param:.3g}, pool {e_pool:.3g}')
    assert e_param < TOL and e_pool < TOL


def _run_block(m, block, fused, x, guard=0):
    """syn_ghostnet_block on a host NHWC array -> (out, aux or None, guard floats before and after `out` as uint32)"""
    import torch
    from synergynet_amd import abi
    s = SHAPES[block]
    B = x.shape[0]
    n_out = B * (62 if block == 17 else s['hout'] ** 2 * s['cout'])
    xd = torch.from_numpy(x).cuda().contiguous()
    buf = torch.full((n_out + 2 * guard,), float('nan'), device='cuda')
    if guard:
        buf.view(torch.int32)[:] = 0x7fc00001
    out = buf[guard:guard + n_out]
    aux = torch.full((B * s['aux'],), float('nan'), device='cuda') if s['aux'] else None
    abi.check(m._lib.syn_ghostnet_block(m._h, block, int(fused), xd.data_ptr(), B, xd.numel(), out.data_ptr(), n_out,
                                        aux.data_ptr() if aux is not None else None, aux.numel() if aux is not None else 0, m._stream()))
    torch.cuda.synchronize()
    shape = (B, 62) if block == 17 else (B, s['hout'], s['hout'], s['cout'])
    pads = (buf[:guard].view(torch.int32).cpu().numpy(), buf[guard + n_out:].view(torch.int32).cpu().numpy())
    return out.cpu().numpy().reshape(shape), None if aux is None else aux.cpu().numpy().reshape(B, s['aux']), pads


def _block_cases():
    cases = []
    for block in range(18):
        batches = [1, 3] + ([5] if block in (7, 10, 13) else [])      # 6.1, 6.4 and 8.1: one face more than the four of a 4^2 workgroup
        for B in batches:
            for fused in ([0, 1] if block in FUSED_EXISTS else [0]):
                cases.append((block, fused, B))
    # the one batch threshold of the fused kernel: 8^2 maps take two faces per workgroup from 1024 faces on (kGnTwoFacesMinBatch), one
    # below; 1025 = the other path with a last workgroup that holds one face.  6.1 (ragged channel tiles 92 / 40) and 6.3 (SE gate, shortcut)
    cases += [(7, 1, 1025), (9, 1, 1025)]
    return cases


@pytest.mark.parametrize('block,fused,B', _block_cases())
def test_every_block_alone(model, state, block, fused, B):
    """Random N(0,1) NHWC input (negative inputs are legitimate for the kernels) through the launches of the forward, against the float64
    restatement.  B = 1: 3600 / 900 / 225 / 64 / 16 pixels, every partly empty tile; B = 3: 675 and 48 pixels, tiles straddling faces
    and three different gates; ragged channel tiles (12, 20, 36, 92, 100), K = 8 mod 16, both 5x5 s2 shapes, the odd-input 3x3 s2, all five
    convolutional shortcuts and the several-faces-per-workgroup path at 8^2 and 4^2 are all among the blocks."""
    s = SHAPES[block]
    rng = np.random.default_rng(9000 + 100 * block + B)
    x = rng.standard_normal((B, s['hin'], s['hin'], s['cin'])).astype(np.float32)
    want, want_aux = gc.block_reference(state, block, x)
    got, aux, _ = _run_block(model, block, fused, x)
    e = rel_max(got, want)
    e_aux = rel_max(aux, want_aux) if want_aux is not None else 0.0
    print(f'block {block} ({s["key"]}) fused={fused} B={B}: out {e:.3g}, aux {e_aux:.3g}')
    assert np.isfinite(got).all() and e < TOL and e_aux < TOL
    assert (aux is None) == (want_aux is None)


@pytest.mark.parametrize('block,fused', [(1, 0), (7, 0), (7, 1)])
def test_output_guard(model, state, block, fused):
    """64 floats of 0x7fc00001 on either side of `out` are unchanged afterwards: a ragged-tile store out of range would show."""
    s = SHAPES[block]
    x = np.random.default_rng(77 + block).standard_normal((3, s['hin'], s['hin'], s['cin'])).astype(np.float32)
    got, _, (before, after) = _run_block(model, block, fused, x, guard=64)
    assert before.size == 64 and after.size == 64 and (before == 0x7fc00001).all() and (after == 0x7fc00001).all()
    assert rel_max(got, gc.block_reference(state, block, x)[0]) < TOL


def test_block_hook_refuses_wrong_sizes(model):
    import torch
    from synergynet_amd import abi
    lib, h = model._lib, model._h
    x = torch.zeros(80 * 64, device='cuda')
    out = torch.full((80 * 64,), 7.0, device='cuda')
    for args in ((7, 0, 1, x.numel() - 4, out.numel(), 0), (7, 0, 1, x.numel(), out.numel() + 4, 0), (19, 0, 1, x.numel(), out.numel(), 0),
                 (7, 2, 1, x.numel(), out.numel(), 0), (7, 0, 0, x.numel(), out.numel(), 0)):
        block, fused, B, ni, no, na = args
        assert lib.syn_ghostnet_block(h, block, fused, x.data_ptr(), B, ni, out.data_ptr(), no, None, na, None) == abi.SYN_ERR_INVALID
        assert b'syn_ghostnet_block' in lib.syn_last_error() and b'expected' in lib.syn_last_error()
    assert lib.syn_ghostnet_block(h, 7, 0, x.data_ptr(), 1, x.numel(), out.data_ptr(), out.numel(), x.data_ptr(), 184, None) == abi.SYN_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize('B', [1, 7, 33])
def test_ragged_batches(model, state, B):
    from synergynet_amd import synth
    crops = synth.make_crops(B, seed=700 + B)
    want, want_pool = _want(state, f'ragged{B}', gc.normalize_u8(crops), list(range(B)))
    for sched in (2, 1):
        prev = model._lib.syn_set_schedule(model._h, sched)
        try:
            got, got_pool = model.forward_crops_u8(crops, return_pool=True)
        finally:
            model._lib.syn_set_schedule(model._h, prev)
        assert tuple(got.shape) == (B, 62) and tuple(got_pool.shape) == (B, 1280)
        e_param, e_pool = rel_max(got.cpu().numpy(), want), rel_max(got_pool.cpu().numpy(), want_pool)
        print(f'B={B} schedule {sched}: param {e_param:.3g}, pool {e_pool:.3g}')
        assert e_param < TOL and e_pool < TOL


def test_borders_and_neighbouring_faces(model, state):
    """Constant 0, constant 255 and one-pixel checkerboards, every batch slot different from its neighbours: a pad that were pixel 0
    instead of normalised 0, or a gate or a depthwise tap taken from the neighbouring face, shows here.  Both inputs, both schedules."""
    import torch
    crops = gc.border_crops()
    x = gc.normalize_u8(crops)
    want, want_pool = _want(state, 'borders', x, list(range(len(crops))))
    runs = []
    for sched in (2, 0):
        prev = model._lib.syn_set_schedule(model._h, sched)
        try:
            runs += [(f'u8 schedule {sched}', model.forward_crops_u8(crops, return_pool=True)),
                     (f'fp32 schedule {sched}', model.forward_test(torch.from_numpy(x).cuda(), return_pool=True))]
        finally:
            model._lib.syn_set_schedule(model._h, prev)
    for name, (got, got_pool) in runs:
        for i in range(len(crops)):
            e_param, e_pool = rel_max(got[i:i + 1].cpu().numpy(), want[i:i + 1]), rel_max(got_pool[i:i + 1].cpu().numpy(), want_pool[i:i + 1])
            print(f'{name} slot {i}: param {e_param:.3g}, pool {e_pool:.3g}')
            assert e_param < TOL and e_pool < TOL, f'{name} slot {i}'
        g = got.cpu().numpy()
        assert rel_max(g[0:1], g[5:6]) < 1e-5 and rel_max(g[0:1], g[1:2]) > 1e-3, name
    assert rel_max(want[0:1], want[5:6]) < 1e-5 and rel_max(want[0:1], want[1:2]) > 1e-3


@pytest.mark.parametrize('B', [5, 130])
def test_schedules_agree(model, per_layer_model, B):
    """The fused GhostModules (primary in LDS) against one launch per layer (primary through HBM): the same sums in the same order, so the
    same bits, from either ingest."""
    import torch
    from synergynet_amd import synth
    assert model._lib.syn_backbone_launch_count(model._h) == 79
    assert per_layer_model._lib.syn_backbone_launch_count(per_layer_model._h) == 104
    crops = synth.make_crops(B, seed=810 + B)
    cd = torch.from_numpy(crops).cuda()
    xd = torch.from_numpy(gc.normalize_u8(crops)).cuda()
    for name, run in (('u8', lambda m: m.forward_crops_u8(cd, return_pool=True)), ('fp32', lambda m: m.forward_test(xd, return_pool=True))):
        (a, ap), (b, bp) = run(model), run(per_layer_model)
        e_param, e_pool = rel_max(a.cpu().numpy(), b.cpu().numpy()), rel_max(ap.cpu().numpy(), bp.cpu().numpy())
        print(f'B={B} {name}: param {e_param:.3g}, pool {e_pool:.3g}, bit-identical {torch.equal(a, b) and torch.equal(ap, bp)}')
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(ap, bp)
    prev = model._lib.syn_set_schedule(model._h, 0)
    try:
        assert model._lib.syn_backbone_launch_count(model._h) == 104
        c, cp = model.forward_crops_u8(cd, return_pool=True)
    finally:
        model._lib.syn_set_schedule(model._h, prev)
    d, dp = per_layer_model.forward_crops_u8(cd, return_pool=True)
    assert torch.equal(c, d) and torch.equal(cp, dp)


def test_a_face_does_not_depend_on_its_batch(model, state):
    import torch
    from synergynet_amd import synth
    seq = synth.make_crops(40, seed=5200)
    x = gc.normalize_u8(seq)
    got = {B: model.forward_crops_u8(torch.from_numpy(seq[:B]).cuda()).cpu().numpy() for B in (4, 40)}
    for B in (4, 40):
        faces = [0, 1, B - 1]
        want, _ = _want(state, 'sequence', x, faces)
        for k, i in enumerate(faces):
            e = rel_max(got[B][i:i + 1], want[k:k + 1])
            print(f'B={B} face {i}: {e:.3g}')
            assert e < TOL, f'B={B} face {i}'
    assert rel_max(got[4], got[40][:4]) < 1e-5


def test_numerics_entry_points_have_nothing_to_report(model):
    from synergynet_amd import synth
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        n, text = model.numerics_report()
        assert n == 0 and text.count('\n') == 1 and 'ghostnet' in text and 'exact fp32' in text
        model.forward_crops_u8(synth.make_crops(3, seed=5))
        assert model.range_status(fallback=True)[0] == 0
        assert model.calibrate(synth.make_crops(3, seed=5)) == 0


def test_constants_export_import(model, pack, backbone_sd):
    import torch
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    crops = torch.from_numpy(synth.make_crops(5, seed=91)).cuda()
    bare = SynergyNet(device='cuda:0', load_constants=False)
    v2 = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    for src in (model, v2, model):                                   # one bare handle: ghostnet -> mobilenet_v2 -> ghostnet
        bare.import_constants(src.export_constants())
        assert bare.arch == src.arch and bare.pool_dim == src.pool_dim == 1280
        (a, ap), (b, bp) = src.forward_crops_u8(crops, return_pool=True), bare.forward_crops_u8(crops, return_pool=True)
        assert torch.equal(a, b) and torch.equal(ap, bp)
    assert bare.arch == 'ghostnet'


def test_refinement_is_accepted(model, pack, backbone_sd):
    """The refinement does not depend on the backbone: the same param / pool give the same landmarks, bit for bit, on a mobilenet_v2
    handle; forward_synergy runs on the ghostnet handle."""
    import torch
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    syn_sd = synth.make_synergy_state(1)
    model.load_synergy_state(syn_sd)
    v2 = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    v2.load_synergy_state(syn_sd)
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(3, seed=17))).cuda()
    param, pool = model.forward_test(x, return_pool=True)
    a, b = model.refine_landmarks(param, pool), v2.refine_landmarks(param, pool)
    assert tuple(a.shape) == (3, 3, 68) and torch.isfinite(a).all() and torch.equal(a, b)
    out = model.forward_synergy(x)
    assert all(torch.isfinite(out[k]).all() for k in ('param', 'lmk', 'lmk_refined', 'param_rev'))
    assert torch.equal(out['param'], param)
    res = model.get_all_outputs(synth.make_frame(160, 160, seed=1), [[20.0, 20.0, 140.0, 140.0, 0.9]], refine=True)
    assert np.isfinite(np.asarray(res[0][0])).all()


def test_whole_path_on_frames(model):
    """get_all_outputs_batch on two synthetic frames with given rects: the geometry stage and the front end do not depend on the backbone."""
    from oracle.preproc_numpy import crop_img, resize_lanczos4
    from synergynet_amd import synth
    m = model
    frames = [synth.make_frame(200, 260, seed=3), synth.make_frame(180, 180, seed=4)]
    rects = [[[30.0, 20.0, 150.0, 160.0, 0.99], [120.0, 60.0, 240.0, 190.0, 0.9]], [[-10.0, 15.0, 120.0, 150.0, 0.95]]]
    res = m.get_all_outputs_batch(frames, [[list(r) for r in fr] for fr in rects])
    assert [len(t[0]) for t in res] == [2, 1]
    crops, rois = [], []
    for fr, rs in zip(frames, rects):
        for r in rs:
            r = list(r)
            hc, wc = (r[1] + r[3]) / 2, (r[0] + r[2]) / 2
            h = (r[3] - r[1]) * 1.2 // 2
            r[0], r[1], r[2], r[3] = wc - h, hc - h, wc + h, hc + h
            crops.append(resize_lanczos4(crop_img(fr, r), 120, 120)); rois.append(r)
    p = m.forward_crops_u8(np.stack(crops))
    want = m.landmarks_and_pose(p, roi=np.asarray(rois, np.float32))[0].cpu().numpy()
    lm = [l for t in res for l in t[0]]
    mesh = [v for t in res for v in t[1]]
    assert np.array_equal(np.stack(lm), want)
    assert all(l.shape == (3, 68) and np.isfinite(l).all() for l in lm)
    assert all(v.shape == (3, m._n_vert) and np.isfinite(v).all() for v in mesh) and len(mesh) == 3
    one = m.get_all_outputs(frames[1], [list(r) for r in rects[1]])
    assert np.array_equal(one[0][0], lm[2])
