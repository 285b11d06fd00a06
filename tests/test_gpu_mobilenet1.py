"""GPU parity of the MobileNetV1 backbones (arch = mobilenet_1 / mobilenet_05 / mobilenet_2): the HIP path against the reference
module's recorded outputs (tests/golden/mobilenet1_outputs.npz) and against the torch restatement of tests/mobilenet1_cases.py, which
tests/test_mobilenet1_cpu.py holds against the same recording.  Bar: rel_max < 1e-4 (TOL of tests/test_gpu_parity.py); the two
schedules of one network, both exact fp32, agree to 1e-5."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import mobilenet1_cases as mc
from mobilenet1_cases import TOL, rel_max

pytestmark = pytest.mark.gpu
ARCHS = ['mobilenet_1', 'mobilenet_05', 'mobilenet_2']


def _state(arch):
    from synergynet_amd import synth
    w = mc.WIDTHS[arch]
    return synth.make_mobilenet1_state(mc.SEEDS[w], w)


@pytest.fixture(scope='module')
def models(pack):
    """arch -> model on the default schedule, built on first use; constructing one must not warn (there is no range verdict to report)"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd.synergy3DMM import SynergyNet
    made = {}

    def get(arch):
        if arch not in made:
            with warnings.catch_warnings():
                warnings.simplefilter('error')
                made[arch] = SynergyNet(device='cuda:0', pack=pack, backbone_state=_state(arch), arch=arch)
        return made[arch]
    return get


@pytest.fixture(scope='module')
def per_layer_model(pack):
    """mobilenet_1 on the per-layer schedule, selected the documented way"""
    from synergynet_amd.synergy3DMM import SynergyNet
    os.environ['SYNERGY_HIP_FUSION'] = '0'
    try:
        return SynergyNet(device='cuda:0', pack=pack, backbone_state=_state('mobilenet_1'), arch='mobilenet_1')
    finally:
        os.environ.pop('SYNERGY_HIP_FUSION', None)


_REF = {}


def _want(arch, tag, x_norm, faces):
    """restatement outputs (param62, pool) of the given faces of a named input, computed once per face"""
    todo = [i for i in faces if (arch, tag, i) not in _REF]
    if todo:
        out, pool = mc.mobilenet1_forward(_state(arch), x_norm[todo], mc.WIDTHS[arch])
        for k, i in enumerate(todo):
            _REF[arch, tag, i] = (out[k, :62], pool[k])
    return np.stack([_REF[arch, tag, i][0] for i in faces]), np.stack([_REF[arch, tag, i][1] for i in faces])


@pytest.mark.parametrize('arch', ['mobilenet_1', 'mobilenet_05', 'mobilenet_2'])
def test_golden_parity(models, arch):
    import torch
    from synergynet_amd import synth
    g = np.load(mc.GOLDEN)
    t = mc.TAG[mc.WIDTHS[arch]]
    x = synth.normalize_crops(synth.make_crops(2, seed=int(g['crops_seed'])))
    param, pool = models(arch).forward_test(torch.from_numpy(x).cuda(), return_pool=True)
    assert tuple(param.shape) == (2, 62) and tuple(pool.shape) == (2, int(1024 * mc.WIDTHS[arch]))
    e_param, e_pool = rel_max(param.cpu().numpy(), g[f'out102_{t}'][:, :62]), rel_max(pool.cpu().numpy(), g[f'pool_{t}'])
    print(f'{arch}: param {e_param:.3g}, pool {e_pool:.3g}')
    assert e_param < TOL and e_pool < TOL


@pytest.mark.parametrize('arch,B', [('mobilenet_1', 1), ('mobilenet_1', 7), ('mobilenet_1', 33), ('mobilenet_05', 1), ('mobilenet_05', 7),
                                    ('mobilenet_2', 1), ('mobilenet_2', 7)])
def test_ragged_batches(models, arch, B):
    """B = 1: every 64-pixel tile is partly empty (the 4x4 layers are one 16-pixel MFMA tile); B = 7: B * 225 and B * 16 pixels are no
    multiples of the tile, so tiles straddle faces; mobilenet_05 has K = 16 in its first block, mobilenet_2 K = 2048 (16 chunks).
    These batches are below the 128 faces from which the default schedule runs the fused launches, so each goes through the default
    schedule AND through the fused launches forced on (syn_set_schedule(h, 1))."""
    from synergynet_amd import synth
    m = models(arch)
    crops = synth.make_crops(B, seed=700 + B)
    want, want_pool = _want(arch, f'ragged{B}', mc.normalize_u8(crops), list(range(B)))
    for sched in (2, 1):
        prev = m._lib.syn_set_schedule(m._h, sched)
        try:
            got, got_pool = m.forward_crops_u8(crops, return_pool=True)
        finally:
            m._lib.syn_set_schedule(m._h, prev)
        assert tuple(got.shape) == (B, 62) and tuple(got_pool.shape) == (B, m.pool_dim) and m.pool_dim == int(1024 * mc.WIDTHS[arch])
        e_param, e_pool = rel_max(got.cpu().numpy(), want), rel_max(got_pool.cpu().numpy(), want_pool)
        print(f'{arch} B={B} schedule {sched}: param {e_param:.3g}, pool {e_pool:.3g}')
        assert e_param < TOL and e_pool < TOL


def test_batch_sizes_across_the_launcher_threshold(models):
    """The launchers have ONE batch-size threshold (csrc/syn_internal.h kMb1FusedMinBatch = 128, csrc/synergy_abi.hip run_mobilenet1):
    the default schedule runs the per-layer launches below 128 faces and the fused launches from 128 on.  Inside the fused kernel the
    pixel tile (64), the K chunk (128) and the channel tiles per wave (by the layer's width) do not depend on the batch.  One batch on
    each side, faces 0, 1, B // 2 and B - 1 of a fixed sequence against the restatement; a face's result does not depend on the batch
    it rides in."""
    import torch
    from synergynet_amd import synth
    seq = synth.make_crops(128, seed=5100)
    x = mc.normalize_u8(seq)
    got = {}
    for B in (127, 128):
        got[B] = models('mobilenet_1').forward_crops_u8(torch.from_numpy(seq[:B]).cuda()).cpu().numpy()
        faces = sorted({0, 1, B // 2, B - 1})
        want, _ = _want('mobilenet_1', 'threshold', x, faces)
        for k, i in enumerate(faces):
            e = rel_max(got[B][i:i + 1], want[k:k + 1])
            print(f'B={B} face {i}: {e:.3g}')
            assert e < TOL, f'B={B} face {i}'
    assert rel_max(got[127], got[128][:127]) < 1e-5


@pytest.mark.parametrize('arch', ARCHS)
def test_borders_and_neighbouring_faces(models, arch):
    """Constant 0, constant 255 and one-pixel checkerboards, every batch slot different from its neighbours: a pad that were pixel 0
    (-0.996 after normalisation) instead of 0, or a depthwise tap that read the next face, would show here.  Both input paths."""
    import torch
    crops = mc.border_crops()
    x = mc.normalize_u8(crops)
    want, want_pool = _want(arch, 'borders', x, list(range(len(crops))))
    m = models(arch)
    runs = [('u8', m.forward_crops_u8(crops, return_pool=True)), ('fp32', m.forward_test(torch.from_numpy(x).cuda(), return_pool=True))]
    prev = m._lib.syn_set_schedule(m._h, 1)                          # six faces: the fused launches have to be asked for
    try:
        runs += [('u8 fused', m.forward_crops_u8(crops, return_pool=True)), ('fp32 fused', m.forward_test(torch.from_numpy(x).cuda(), return_pool=True))]
    finally:
        m._lib.syn_set_schedule(m._h, prev)
    for name, (got, got_pool) in runs:
        for i in range(len(crops)):
            e_param, e_pool = rel_max(got[i:i + 1].cpu().numpy(), want[i:i + 1]), rel_max(got_pool[i:i + 1].cpu().numpy(), want_pool[i:i + 1])
            print(f'{arch} {name} slot {i}: param {e_param:.3g}, pool {e_pool:.3g}')
            assert e_param < TOL and e_pool < TOL, f'{name} slot {i}'
    assert rel_max(want[0:1], want[5:6]) < 1e-5 and rel_max(want[0:1], want[1:2]) > 1e-3      # slots 0 and 5 are the same image; the cases do tell 0 from 255


@pytest.mark.parametrize('B', [5, 33, 130])
def test_fused_and_per_layer_schedules_agree(models, per_layer_model, B):
    """The fused launches (one per block, depthwise output in LDS) against SYNERGY_HIP_FUSION=0 (depthwise and pointwise launches
    through HBM), uint8 and fp32 input: both exact fp32 -- 1e-5, the bound tests/test_gpu_parity.py uses for two exact-fp32 schedules
    of one network.  B = 130 is the default schedule as it is; at B = 5 and 33 the default schedule IS the per-layer one, so the fused
    launches are forced on (schedule 1)."""
    import torch
    from synergynet_amd import synth
    fused = models('mobilenet_1')
    assert fused._lib.syn_backbone_launch_count(fused._h) == 15 and per_layer_model._lib.syn_backbone_launch_count(per_layer_model._h) == 28
    crops = synth.make_crops(B, seed=810 + B)
    cd = torch.from_numpy(crops).cuda()
    xd = torch.from_numpy(mc.normalize_u8(crops)).cuda()
    prev = fused._lib.syn_set_schedule(fused._h, 2 if B >= 128 else 1)
    try:
        for name, run in (('u8', lambda m: m.forward_crops_u8(cd, return_pool=True)), ('fp32', lambda m: m.forward_test(xd, return_pool=True))):
            (a, ap), (b, bp) = run(fused), run(per_layer_model)
            e_param, e_pool = rel_max(a.cpu().numpy(), b.cpu().numpy()), rel_max(ap.cpu().numpy(), bp.cpu().numpy())
            print(f'B={B} {name}: param {e_param:.3g}, pool {e_pool:.3g}')
            assert torch.isfinite(a).all() and e_param < 1e-5 and e_pool < 1e-5
    finally:
        fused._lib.syn_set_schedule(fused._h, prev)
    # syn_set_schedule(h, 0) switches the same handle to what SYNERGY_HIP_FUSION=0 selects
    prev = fused._lib.syn_set_schedule(fused._h, 0)
    try:
        c = fused.forward_crops_u8(cd)
    finally:
        fused._lib.syn_set_schedule(fused._h, prev)
    assert torch.equal(c, per_layer_model.forward_crops_u8(cd))
    if B < 128:                                                      # ... and below the threshold the default schedule is that one
        assert torch.equal(fused.forward_crops_u8(cd), c)


def test_numerics_entry_points_have_nothing_to_report(models):
    from synergynet_amd import synth
    m = models('mobilenet_05')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        n, text = m.numerics_report()
        assert n == 0 and text.count('\n') == 1 and 'mobilenet_05' in text and 'exact fp32' in text
        m.forward_crops_u8(synth.make_crops(3, seed=5))
        assert m.range_status(fallback=True)[0] == 0
        assert m.calibrate(synth.make_crops(3, seed=5)) == 0


def test_constants_export_import(models, pack, backbone_sd):
    import torch
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    crops = torch.from_numpy(synth.make_crops(5, seed=91)).cuda()
    bare = SynergyNet(device='cuda:0', load_constants=False)
    assert bare.arch == 'mobilenet_v2'
    for arch in ('mobilenet_2', 'mobilenet_1'):                      # one handle, one architecture after the other
        src = models(arch)
        bare.import_constants(src.export_constants())
        assert bare.arch == arch and bare.pool_dim == src.pool_dim == int(1024 * mc.WIDTHS[arch])
        (a, ap), (b, bp) = src.forward_crops_u8(crops, return_pool=True), bare.forward_crops_u8(crops, return_pool=True)
        assert torch.equal(a, b) and torch.equal(ap, bp)
        assert torch.equal(src.reconstruct(a, dense=False), bare.reconstruct(b, dense=False))
    v2 = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    bare.import_constants(v2.export_constants())
    assert bare.arch == 'mobilenet_v2' and bare.pool_dim == 1280
    (a, ap), (b, bp) = v2.forward_crops_u8(crops, return_pool=True), bare.forward_crops_u8(crops, return_pool=True)
    assert torch.equal(a, b) and torch.equal(ap, bp)


def test_whole_path_on_frames(models):
    """get_all_outputs_batch on two synthetic frames with given rects: the geometry stage and the front end do not depend on the backbone."""
    from oracle.preproc_numpy import crop_img, resize_lanczos4
    from synergynet_amd import synth
    m = models('mobilenet_1')
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
    poses = [q for t in res for q in t[2]]
    assert np.array_equal(np.stack(lm), want)
    assert all(l.shape == (3, 68) and np.isfinite(l).all() for l in lm)
    assert all(v.shape == (3, m._n_vert) and np.isfinite(v).all() for v in mesh) and len(mesh) == 3
    assert all(len(q[0]) == 3 and np.isfinite(q[0]).all() and np.isfinite(q[1]).all() for q in poses)
    one = m.get_all_outputs(frames[1], [list(r) for r in rects[1]])
    assert np.array_equal(one[0][0], lm[2])


def test_refinement_is_refused(models, pack):
    import torch
    from synergynet_amd import abi, synth
    m = models('mobilenet_05')
    lib = m._lib
    m.load_synergy_state(synth.make_synergy_state(1))
    param = torch.zeros((1, 62), device='cuda')
    pool = torch.zeros((1, 1280), device='cuda')
    out = torch.full((1, 3, 68), float('nan'), device='cuda')
    with pytest.raises(RuntimeError, match='1280-d pooled feature'):
        m.refine_landmarks(param, pool)
    rc = lib.syn_refine_landmarks(m._h, param.data_ptr(), pool.data_ptr(), 1, 1, None, None, out.data_ptr(), None, m._stream())
    assert rc == abi.SYN_ERR_INVALID
    err = lib.syn_last_error()
    assert b'1280-d pooled feature' in err and b'mobilenet_05' in err and b'512-d' in err
    assert torch.isnan(out).all()
    with pytest.raises(RuntimeError, match='1280-d pooled feature'):
        m.get_all_outputs(synth.make_frame(64, 64, seed=1), [[4.0, 4.0, 60.0, 60.0, 0.9]], refine=True)
