"""GPU parity of the ResNeSt-50 backbone (arch = 'resnest50'): the HIP path against the reference module's recorded outputs
(tests/golden/resnest50_outputs.npz) and against the torch restatement of tests/resnest_cases.py, which tests/test_resnest_cpu.py
holds against the same recording -- never against the library itself.  Bar: rel_max < 1e-4 (TOL of tests/test_gpu_parity.py); the two
schedules of the network run the same operations in the same order per output element and must agree bit for bit."""
import os
import warnings

import numpy as np
import pytest

import resnest_cases as rc
from resnest_cases import TOL, rel_max

pytestmark = pytest.mark.gpu
SHAPES = rc.block_shapes()
NAMES = [s['key'] for s in SHAPES]
LAUNCHES = {1: 74, 0: 95}          # fused, per-layer


@pytest.fixture(scope='module')
def state():
    from synergynet_amd import synth
    return synth.make_resnest50_state(rc.SEED)


@pytest.fixture(scope='module')
def model(pack, state):
    """one model for the whole module, on the default schedule; constructing it must not warn (there is no range verdict to report)"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd.synergy3DMM import SynergyNet
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = SynergyNet(device='cuda:0', pack=pack, backbone_state=state, arch='resnest50')
    assert m.arch == 'resnest50' and m.pool_dim == 2048
    return m


class _schedule:
    """syn_set_schedule for the length of a with block"""

    def __init__(self, m, code):
        self.m, self.code = m, code

    def __enter__(self):
        self.prev = self.m._lib.syn_set_schedule(self.m._h, self.code)

    def __exit__(self, *a):
        self.m._lib.syn_set_schedule(self.m._h, self.prev)


_REF = {}


def _want(state, tag, x_norm, faces):
    """restatement outputs (param62, pool) of the given faces of a named input, computed once per face"""
    todo = [i for i in faces if (tag, i) not in _REF]
    if todo:
        out, pool = rc.resnest_forward(state, x_norm[todo])
        for k, i in enumerate(todo):
            _REF[tag, i] = (out[k], pool[k])
    return np.stack([_REF[tag, i][0] for i in faces]), np.stack([_REF[tag, i][1] for i in faces])


def test_golden_parity(model):
    """the 2 crops of the golden file, fp32 and uint8 ingest, both schedules, against the reference module's recording"""
    import torch
    from synergynet_amd import synth
    g = np.load(rc.GOLDEN)
    crops = rc.golden_crops()
    x = torch.from_numpy(synth.normalize_crops(crops)).cuda()
    for sched in (1, 0):
        with _schedule(model, sched):
            runs = (('fp32', model.forward_test(x, return_pool=True)), ('u8', model.forward_crops_u8(crops, return_pool=True)))
        for name, (param, pool) in runs:
            assert tuple(param.shape) == (2, 62) and tuple(pool.shape) == (2, 2048)
            e_param, e_pool = rel_max(param.cpu().numpy(), g['out62']), rel_max(pool.cpu().numpy(), g['pool'])
            print(f'schedule {sched} {name}: param {e_param:.3g}, pool {e_pool:.3g}')
            assert e_param < TOL and e_pool < TOL


def _run_block(m, block, fused, x, guard=0):
    """syn_resnest50_block on a host NHWC array -> (out, aux or None, guard words before / after `out` and `aux` as int32)"""
    import torch
    from synergynet_amd import abi
    s = SHAPES[block]
    B = x.shape[0]
    n_out = B * (62 if block == 17 else s['hout'] ** 2 * s['cout'])
    n_aux = B * s['aux']
    xd = torch.from_numpy(x).cuda().contiguous()

    def guarded(n):
        buf = torch.full((n + 2 * guard,), float('nan'), device='cuda')
        if guard:
            buf.view(torch.int32)[:] = 0x7fc00001
        return buf, buf[guard:guard + n]

    obuf, out = guarded(n_out)
    abuf, aux = guarded(n_aux) if n_aux else (None, None)
    abi.check(m._lib.syn_resnest50_block(m._h, block, int(fused), xd.data_ptr(), B, xd.numel(), out.data_ptr(), n_out,
                                         aux.data_ptr() if aux is not None else None, n_aux, m._stream()))
    torch.cuda.synchronize()
    shape = (B, 62) if block == 17 else (B, s['hout'], s['hout'], s['cout'])
    pads = [b[:guard].view(torch.int32).cpu().numpy() for b in (obuf, abuf) if b is not None]
    pads += [b[b.numel() - guard:].view(torch.int32).cpu().numpy() for b in (obuf, abuf) if b is not None] if guard else []
    return out.cpu().numpy().reshape(shape), None if aux is None else aux.cpu().numpy().reshape(B, s['aux']), pads


_BLOCK_REF = {}


def _block_case(state, block, B):
    """input and float64 reference of a block at a batch size, computed once and shared by both schedules"""
    if (block, B) not in _BLOCK_REF:
        s = SHAPES[block]
        rng = np.random.default_rng(9000 + 100 * block + B)
        x = rng.standard_normal((B, s['hin'], s['hin'], s['cin'])).astype(np.float32)
        if block == 0:
            x = np.clip(x, -1.0, 1.0)
        _BLOCK_REF[block, B] = (x,) + rc.block_reference(state, block, x)
    return _BLOCK_REF[block, B]


@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('block', range(18))
def test_every_block_alone(model, state, block, B, fused):
    """Random N(0,1) NHWC input (negative inputs are legitimate for the kernels) through the launches of the forward, against the float64
    restatement.  B = 1: 900 / 225 / 64 / 16 pixels, every partly empty tile; B = 3: 2700, 675, 192 and 48 pixels, tiles that straddle
    faces on the 30^2 and 15^2 maps and three different attentions.  The three avd blocks (30 -> 15, 15 -> 8 with its one-sample windows,
    8 -> 4), the identity-pool downsample of layer1.0 and all four gate widths are among the blocks."""
    s = SHAPES[block]
    x, want, want_aux = _block_case(state, block, B)
    got, aux, _ = _run_block(model, block, fused, x)
    e = rel_max(got, want)
    e_aux = rel_max(aux, want_aux) if want_aux is not None else 0.0
    print(f'block {block} ({s["key"]}) fused={fused} B={B}: out {e:.3g}, aux {e_aux:.3g}')
    assert np.isfinite(got).all() and e < TOL and e_aux < TOL
    assert (aux is None) == (want_aux is None)


@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('name', ['layer1.0', 'layer3.0', 'layer4.2'])
def test_output_guard(model, state, name, fused):
    """64 words of 0x7fc00001 on either side of `out` and of `aux` are unchanged afterwards: a ragged-tile store out of range would show.
    layer1.0: no avd, identity-pool downsample; layer3.0: 15 -> 8, both pools, partial windows; layer4.2: 16 pixels per face."""
    block = NAMES.index(name)
    x, want, want_aux = _block_case(state, block, 3)
    got, aux, pads = _run_block(model, block, fused, x, guard=64)
    assert len(pads) == 4 and all(p.size == 64 and (p == 0x7fc00001).all() for p in pads)
    assert rel_max(got, want) < TOL and rel_max(aux, want_aux) < TOL


def test_fused_tail_without_channel_split(model, state):
    """The fused tail splits its channels over workgroups until the grid has 1024 of them; layer4.2 at 1100 faces (16 pixels per
    workgroup) is past that, so one workgroup walks all 2048 channels.  Input made on the device; the per-layer launches, held against the
    float64 restatement on the first two faces here and on every small case above, are the reference for the rest: the same bits."""
    import torch
    from synergynet_amd import abi
    block, B = NAMES.index('layer4.2'), 1100
    gen = torch.Generator(device='cuda').manual_seed(4242)
    x = torch.randn((B, 4, 4, 2048), device='cuda', generator=gen)
    outs = []
    for fused in (0, 1):
        out, att = torch.full((B, 4, 4, 2048), float('nan'), device='cuda'), torch.full((B, 1024), float('nan'), device='cuda')
        abi.check(model._lib.syn_resnest50_block(model._h, block, fused, x.data_ptr(), B, x.numel(), out.data_ptr(), out.numel(),
                                                 att.data_ptr(), att.numel(), model._stream()))
        torch.cuda.synchronize()
        outs.append((out, att))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want, want_att = rc.block_reference(state, block, x[:2].cpu().numpy())
    assert rel_max(outs[1][0][:2].cpu().numpy(), want) < TOL and rel_max(outs[1][1][:2].cpu().numpy(), want_att) < TOL


def test_block_hook_refuses_wrong_sizes(model):
    import torch
    from synergynet_amd import abi
    lib, h = model._lib, model._h
    block = NAMES.index('layer4.2')                                  # [B,4,4,2048] -> [B,4,4,2048], aux [B,1024]
    x = torch.zeros(16 * 2048, device='cuda')
    out = torch.full((16 * 2048,), 7.0, device='cuda')
    aux = torch.full((1024,), 7.0, device='cuda')
    n = x.numel()
    for blk, fused, B, ni, no, na in ((block, 0, 1, n - 4, n, 0), (block, 0, 1, n, n + 4, 0), (18, 0, 1, n, n, 0), (-1, 0, 1, n, n, 0),
                                      (block, 2, 1, n, n, 0), (block, 0, 0, n, n, 0), (block, 0, 65537, n, n, 0), (block, 1, 1, n, n, 1024)):
        assert lib.syn_resnest50_block(h, blk, fused, x.data_ptr(), B, ni, out.data_ptr(), no, None, na, None) == abi.SYN_ERR_INVALID
        assert b'syn_resnest50_block' in lib.syn_last_error() and b'expected' in lib.syn_last_error()
    assert lib.syn_resnest50_block(h, block, 0, x.data_ptr(), 1, n, out.data_ptr(), n, aux.data_ptr(), 1020, None) == abi.SYN_ERR_INVALID
    img = torch.zeros(43200, device='cuda')                          # aux where none exists: the stem
    assert lib.syn_resnest50_block(h, 0, 0, img.data_ptr(), 1, 43200, out.data_ptr(), 57600, aux.data_ptr(), 1024, None) == abi.SYN_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((aux == 7.0).all())


def test_block_hook_refuses_another_arch(model, pack, backbone_sd):
    import torch
    from synergynet_amd import abi
    from synergynet_amd.synergy3DMM import SynergyNet
    v2 = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    x = torch.zeros(16 * 2048, device='cuda')
    out = torch.full((62,), 7.0, device='cuda')
    assert v2._lib.syn_resnest50_block(v2._h, 17, 0, x.data_ptr(), 1, x.numel(), out.data_ptr(), 62, None, 0, None) == abi.SYN_ERR_INVALID
    assert b'expected resnest50' in v2._lib.syn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize('B', [1, 7, 33])
def test_ragged_batches(model, state, B):
    """B = 1: grids smaller than the 8 XCDs, the fused tail splits its channels over workgroups; B = 33: 33 * 16 and 33 * 64 pixel rows,
    ragged for every tile height.  The default schedule (the fused one) and the per-layer one."""
    from synergynet_amd import synth
    crops = synth.make_crops(B, seed=700 + B)
    want, want_pool = _want(state, f'ragged{B}', rc.normalize_u8(crops), list(range(B)))
    for sched in (2, 0):
        with _schedule(model, sched):
            got, got_pool = model.forward_crops_u8(crops, return_pool=True)
        assert tuple(got.shape) == (B, 62) and tuple(got_pool.shape) == (B, 2048)
        e_param, e_pool = rel_max(got.cpu().numpy(), want), rel_max(got_pool.cpu().numpy(), want_pool)
        print(f'B={B} schedule {sched}: param {e_param:.3g}, pool {e_pool:.3g}')
        assert e_param < TOL and e_pool < TOL


def test_borders_and_neighbouring_faces(model, state):
    """Constant 0, constant 255 and one-pixel checkerboards, every batch slot different from its neighbours: a pad that were pixel 0
    instead of normalised 0, or an attention or a pool tap taken from the neighbouring face, shows here.  Both inputs, both schedules."""
    import torch
    crops = rc.border_crops()
    x = rc.normalize_u8(crops)
    want, want_pool = _want(state, 'borders', x, list(range(len(crops))))
    runs = []
    for sched in (1, 0):
        with _schedule(model, sched):
            runs += [(f'u8 schedule {sched}', model.forward_crops_u8(crops, return_pool=True)),
                     (f'fp32 schedule {sched}', model.forward_test(torch.from_numpy(x).cuda(), return_pool=True))]
    for name, (got, got_pool) in runs:
        for i in range(len(crops)):
            e_param, e_pool = rel_max(got[i:i + 1].cpu().numpy(), want[i:i + 1]), rel_max(got_pool[i:i + 1].cpu().numpy(), want_pool[i:i + 1])
            print(f'{name} slot {i}: param {e_param:.3g}, pool {e_pool:.3g}')
            assert e_param < TOL and e_pool < TOL, f'{name} slot {i}'
        g = got.cpu().numpy()
        assert np.array_equal(g[0], g[5]) and np.array_equal(g[1], g[4]) and rel_max(g[0:1], g[1:2]) > 1e-3, name
    assert rel_max(want[0:1], want[1:2]) > 1e-3


@pytest.mark.parametrize('B', [5, 130])
def test_schedules_agree_bit_for_bit(model, B):
    """The fused tail (operands built in LDS) against one launch per layer (operands through HBM): the same bits.  At 5 faces the fused
    tail splits the channels of layer3 and layer4 over workgroups, at 130 it does not; the default schedule (2) is the fused one."""
    import torch
    from synergynet_amd import synth
    crops = synth.make_crops(B, seed=810 + B)
    cd = torch.from_numpy(crops).cuda()
    xd = torch.from_numpy(rc.normalize_u8(crops)).cuda()
    got = {}
    for sched in (0, 1, 2):
        with _schedule(model, sched):
            assert model._lib.syn_backbone_launch_count(model._h) == LAUNCHES[min(sched, 1)]
            got[sched] = model.forward_crops_u8(cd, return_pool=True) + model.forward_test(xd, return_pool=True)
    assert all(torch.isfinite(t).all() for t in got[0])
    for sched in (1, 2):
        for a, b in zip(got[0], got[sched]):
            assert torch.equal(a, b), f'schedule {sched} differs from the per-layer one by {rel_max(a.cpu().numpy(), b.cpu().numpy()):.3g}'
    assert float(got[0][0].abs().max()) > 1e-2


def test_environment_knob_selects_the_schedule(pack, state):
    """SYNERGY_HIP_FUSION, the documented way: 0 = per-layer, 1 = fused (what the default, 2, runs as well)."""
    from synergynet_amd.synergy3DMM import SynergyNet
    for knob, launches in (('0', 95), ('1', 74)):
        os.environ['SYNERGY_HIP_FUSION'] = knob
        try:
            m = SynergyNet(device='cuda:0', load_constants=False, arch='resnest50')
            flat = np.zeros(m._lib.syn_resnest50_flat_count(), np.float32)
            assert m._lib.syn_load_backbone_resnest50(m._h, flat.ctypes.data, flat.size) == 0
            assert m._lib.syn_backbone_launch_count(m._h) == launches
        finally:
            os.environ.pop('SYNERGY_HIP_FUSION', None)


def test_a_face_does_not_depend_on_its_batch(model, state):
    """One face alone, first, in the middle and last in a batch of 33: the same bits, in both schedules (the gate's sums are per face in
    a fixed order, and no tile shares anything between faces)."""
    import torch
    from synergynet_amd import synth
    seq = synth.make_crops(33, seed=5200)
    want, _ = _want(state, 'sequence', rc.normalize_u8(seq), [0])
    for sched in (0, 1):
        with _schedule(model, sched):
            alone, alone_pool = model.forward_crops_u8(torch.from_numpy(seq[:1]).cuda(), return_pool=True)
            assert rel_max(alone.cpu().numpy(), want) < TOL
            for pos in (0, 16, 32):
                batch = seq.copy()
                batch[[0, pos]] = batch[[pos, 0]]
                got, got_pool = model.forward_crops_u8(torch.from_numpy(batch).cuda(), return_pool=True)
                assert torch.equal(got[pos], alone[0]) and torch.equal(got_pool[pos], alone_pool[0]), f'schedule {sched} position {pos}'


def test_numerics_entry_points_have_nothing_to_report(model):
    from synergynet_amd import synth
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        n, text = model.numerics_report()
        assert n == 0 and text.count('\n') == 1 and 'resnest50' in text and 'exact fp32' in text
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
    for src in (model, v2, model):                                   # one bare handle: resnest50 -> mobilenet_v2 -> resnest50
        bare.import_constants(src.export_constants())
        assert bare.arch == src.arch and bare.pool_dim == src.pool_dim
        (a, ap), (b, bp) = src.forward_crops_u8(crops, return_pool=True), bare.forward_crops_u8(crops, return_pool=True)
        assert torch.equal(a, b) and torch.equal(ap, bp)
    assert bare.arch == 'resnest50' and bare.pool_dim == 2048


def test_refinement_is_refused(model):
    import torch
    from synergynet_amd import abi, synth
    model.load_synergy_state(synth.make_synergy_state(1))
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(2, seed=17))).cuda()
    param, pool = model.forward_test(x, return_pool=True)
    with pytest.raises(RuntimeError, match='1280-d pooled feature'):
        model.refine_landmarks(param, pool)
    out = torch.full((2, 3, 68), 7.0, device='cuda')
    rc_ = model._lib.syn_refine_landmarks(model._h, param.data_ptr(), pool.data_ptr(), 2, 1, None, None, out.data_ptr(), None, model._stream())
    assert rc_ == abi.SYN_ERR_INVALID and b'1280-d' in model._lib.syn_last_error() and b'resnest50' in model._lib.syn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_whole_path_on_frames(model):
    """get_all_outputs_frames (FaceBoxes on the device, detections kept there) on two small synthetic frames equals get_all_outputs_batch
    on the same frames array for array, and get_all_outputs with given rects runs: the front end and the geometry stage do not depend
    on the backbone."""
    from synergynet_amd import synth
    from synergynet_amd.faceboxes import FaceBoxes
    m = model
    frames = [synth.make_frame(300, 420, seed=300), synth.make_frame(240, 320, seed=302)]
    prev = m.face_detector
    m.face_detector = FaceBoxes(state_dict=synth.make_faceboxes_state())
    try:
        want = m.get_all_outputs_batch(frames)
        got = m.get_all_outputs_frames(frames)
    finally:
        m.face_detector = prev
    assert len(got) == len(want) == 2 and sum(len(t[0]) for t in want) > 0
    for (l, v, p), (l2, v2, p2) in zip(got, want):
        assert len(l) == len(l2) and len(v) == len(v2) and len(p) == len(p2)
        assert all(np.array_equal(a, b) and np.isfinite(a).all() for a, b in zip(l, l2))
        assert all(np.array_equal(a, b) and a.shape == (3, m._n_vert) for a, b in zip(v, v2))
    one = m.get_all_outputs(synth.make_frame(180, 180, seed=4), [[-10.0, 15.0, 120.0, 150.0, 0.95]])
    assert one[0][0].shape == (3, 68) and np.isfinite(one[0][0]).all() and np.isfinite(np.asarray(one[1][0])).all()
