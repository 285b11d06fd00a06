"""GPU parity of the BasicBlock ResNets (arch = 'resnet18' / 'resnet34'): the HIP path against the reference modules' recorded outputs
(tests/golden/resnet_basic_outputs.npz) and against the torch restatement of tests/resnet_basic_cases.py, which
tests/test_resnet_basic_cpu.py holds against the same recording -- never against the library itself.  Bar: rel_max < 1e-4 (TOL of
tests/test_gpu_parity.py); the two schedules issue the same MFMA sequence per output element and must agree bit for bit."""
import os
import warnings

import numpy as np
import pytest

import resnet_basic_cases as bc
from resnet_basic_cases import TOL, rel_max

pytestmark = pytest.mark.gpu
SHAPES = {a: bc.block_shapes(a) for a in bc.ARCHS}
NAMES = {a: [s['key'] for s in SHAPES[a]] for a in bc.ARCHS}
LAUNCHES = {'resnet18': {1: 19, 0: 22}, 'resnet34': {1: 35, 0: 38}}          # LDS-tiled, per-layer
ALL_BLOCKS = [(a, b) for a in bc.ARCHS for b in range(len(SHAPES[a]))]

_STATE, _MODEL = {}, {}


def _state(arch):
    from synergynet_amd import synth
    if arch not in _STATE:
        _STATE[arch] = synth.make_resnet_basic_state(arch, bc.SEED)
    return _STATE[arch]


@pytest.fixture(scope='module')
def models(pack):
    """arch -> one model for the whole module, on the default schedule, built on first use; constructing it must not warn (there is no
    range verdict to report)"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd.synergy3DMM import SynergyNet

    def get(arch):
        if arch not in _MODEL:
            with warnings.catch_warnings():
                warnings.simplefilter('error')
                _MODEL[arch] = SynergyNet(device='cuda:0', pack=pack, backbone_state=_state(arch), arch=arch)
            assert _MODEL[arch].arch == arch and _MODEL[arch].pool_dim == 512
        return _MODEL[arch]
    yield get
    _MODEL.clear()


class _schedule:
    """syn_set_schedule for the length of a with block"""

    def __init__(self, m, code):
        self.m, self.code = m, code

    def __enter__(self):
        self.prev = self.m._lib.syn_set_schedule(self.m._h, self.code)

    def __exit__(self, *a):
        self.m._lib.syn_set_schedule(self.m._h, self.prev)


_REF = {}


def _want(arch, tag, x_norm, faces):
    """restatement outputs (param62, pool) of the given faces of a named input, computed once per face"""
    todo = [i for i in faces if (arch, tag, i) not in _REF]
    if todo:
        out, pool = bc.resnet_basic_forward(_state(arch), arch, x_norm[todo])
        for k, i in enumerate(todo):
            _REF[arch, tag, i] = (out[k], pool[k])
    return np.stack([_REF[arch, tag, i][0] for i in faces]), np.stack([_REF[arch, tag, i][1] for i in faces])


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_golden_parity(models, arch):
    """the 2 crops of the golden file, fp32 and uint8 ingest, both schedules, against the reference module's recording"""
    import torch
    from synergynet_amd import synth
    model = models(arch)
    g = np.load(bc.GOLDEN)
    crops = bc.golden_crops()
    x = torch.from_numpy(synth.normalize_crops(crops)).cuda()
    for sched in (1, 0):
        with _schedule(model, sched):
            runs = (('fp32', model.forward_test(x, return_pool=True)), ('u8', model.forward_crops_u8(crops, return_pool=True)))
        for name, (param, pool) in runs:
            assert tuple(param.shape) == (2, 62) and tuple(pool.shape) == (2, 512)
            e_param, e_pool = rel_max(param.cpu().numpy(), g[arch + '_out102'][:, :62]), rel_max(pool.cpu().numpy(), g[arch + '_pool'])
            print(f'{arch} schedule {sched} {name}: param {e_param:.3g}, pool {e_pool:.3g}')
            assert e_param < TOL and e_pool < TOL


def _shape(arch, block, B, out):
    s = SHAPES[arch][block]
    if out:
        return (B, 62) if block == len(SHAPES[arch]) - 1 else (B, s['hout'], s['hout'], s['cout'])
    return (B, 3, 120, 120) if block == 0 else (B, s['hin'], s['hin'], s['cin'])


def _run_block_dev(m, block, fused, xd, guard=0):
    """syn_resnet_basic_block on a device tensor -> (out on the device, guard words before / after `out` as int32)"""
    import torch
    from synergynet_amd import abi
    B = xd.shape[0]
    shape = _shape(m.arch, block, B, True)
    n_out = int(np.prod(shape))
    buf = torch.full((n_out + 2 * guard,), float('nan'), device='cuda')
    if guard:
        buf.view(torch.int32)[:] = 0x7fc00001
    out = buf[guard:guard + n_out]
    abi.check(m._lib.syn_resnet_basic_block(m._h, block, int(fused), xd.data_ptr(), B, xd.numel(), out.data_ptr(), n_out, m._stream()))
    torch.cuda.synchronize()
    pads = [buf[:guard].view(torch.int32).cpu().numpy(), buf[buf.numel() - guard:].view(torch.int32).cpu().numpy()] if guard else []
    return out.view(shape), pads


def _run_block(m, block, fused, x, guard=0):
    import torch
    out, pads = _run_block_dev(m, block, fused, torch.from_numpy(x).cuda().contiguous(), guard)
    return out.cpu().numpy(), pads


_BLOCK_REF = {}


def _block_case(arch, block, B):
    """input and float64 reference of a block at a batch size, computed once and shared by both schedules"""
    if (arch, block, B) not in _BLOCK_REF:
        rng = np.random.default_rng(9000 + 100 * block + B + (0 if arch == 'resnet18' else 50))
        x = rng.standard_normal(_shape(arch, block, B, False)).astype(np.float32)
        if block == 0:
            x = np.clip(x, -1.0, 1.0)
        _BLOCK_REF[arch, block, B] = (x, bc.block_reference(_state(arch), arch, block, x))
    return _BLOCK_REF[arch, block, B]


@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('arch,block', ALL_BLOCKS)
def test_every_block_alone(models, arch, block, B, fused):
    """Random N(0,1) NHWC input (negative inputs are legitimate for the kernels) through the launches of the forward, against the float64
    restatement.  B = 1: 900 / 225 / 64 / 16 pixels, every partly empty tile (and on 30^2 the last band of 2 rows under bands of 4);
    B = 3: tiles (per-layer) and bands (LDS-tiled) next to another face.  The three stride-2 blocks are among them: 30 -> 15, 15 -> 8 (the
    odd map: the last output row and column have one padded tap, the downsample's last pixel is (14, 14)) and 8 -> 4.  The downsample
    output -- in the LDS-tiled schedule made by conv1's centre tap -- is the residual of the block's output, half of what is compared
    (test_resnet_basic_cpu.py: reading it one pixel off moves the output by 0.88)."""
    s = SHAPES[arch][block]
    x, want = _block_case(arch, block, B)
    got, _ = _run_block(models(arch), block, fused, x)
    e = rel_max(got, want)
    print(f'{arch} block {block} ({s["key"]}) fused={fused} B={B}: out {e:.3g}')
    assert got.shape == want.shape and np.isfinite(got).all() and e < TOL


def test_the_stride2_blocks_are_among_the_cases():
    for arch in bc.ARCHS:
        strided = [(s['key'], s['hin'], s['hout']) for s in SHAPES[arch] if s['down']]
        assert strided == [('layer2.0', 30, 15), ('layer3.0', 15, 8), ('layer4.0', 8, 4)]
        assert len(SHAPES[arch]) == {'resnet18': 10, 'resnet34': 18}[arch]


@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('name', ['layer1.0', 'layer3.0', 'tail'])
@pytest.mark.parametrize('arch', bc.ARCHS)
def test_output_guard(models, arch, name, fused):
    """64 words of 0x7fc00001 on either side of `out` are unchanged afterwards: a ragged-tile or ragged-band store out of range would
    show.  layer1.0: bands of 4 rows and a last one of 2; layer3.0: 15 -> 8, the downsample inside conv1; the last block: [B,62]."""
    block = NAMES[arch].index(name)
    x, want = _block_case(arch, block, 3)
    got, pads = _run_block(models(arch), block, fused, x, guard=64)
    assert len(pads) == 2 and all(p.size == 64 and (p == 0x7fc00001).all() for p in pads)
    assert rel_max(got, want) < TOL


GRID_CASES = bc.GRID_CASES          # every grid-shape branch of the LDS kernel's launcher (bb_lds_grid): tests/resnet_basic_cases.py


@pytest.mark.parametrize('name,B,what', GRID_CASES, ids=[f'{n}-B{b}' for n, b, _ in GRID_CASES])
def test_launcher_grids(models, name, B, what):
    """Input made on the device; the per-layer launches, held against the float64 restatement on the first two faces here and on every
    small case above, are the reference for the rest: the same bits."""
    import torch
    arch = 'resnet18'
    m = models(arch)
    block = NAMES[arch].index(name)
    gen = torch.Generator(device='cuda').manual_seed(4242 + B)
    x = torch.randn(_shape(arch, block, B, False), device='cuda', generator=gen)
    plain, _ = _run_block_dev(m, block, 0, x)
    tiled, _ = _run_block_dev(m, block, 1, x)
    assert torch.equal(plain, tiled), what
    n = min(B, 2)
    want = bc.block_reference(_state(arch), arch, block, x[:n].cpu().numpy())
    assert rel_max(tiled[:n].cpu().numpy(), want) < TOL and float(tiled[-1].abs().max()) > 1e-2


def test_block_hook_refuses_wrong_sizes(models):
    import torch
    from synergynet_amd import abi
    model = models('resnet18')
    lib, h = model._lib, model._h
    block = NAMES['resnet18'].index('layer4.1')                      # [B,4,4,512] -> [B,4,4,512]
    x = torch.zeros(16 * 512, device='cuda')
    out = torch.full((16 * 512,), 7.0, device='cuda')
    n = x.numel()
    for blk, fused, B, ni, no in ((block, 0, 1, n - 4, n), (block, 0, 1, n, n + 4), (10, 0, 1, n, n), (-1, 0, 1, n, n), (block, 2, 1, n, n),
                                  (block, 0, 0, n, n), (block, 0, 65537, n, n), (9, 1, 1, n, 102)):
        assert lib.syn_resnet_basic_block(h, blk, fused, x.data_ptr(), B, ni, out.data_ptr(), no, None) == abi.SYN_ERR_INVALID
        assert b'syn_resnet_basic_block' in lib.syn_last_error() and b'expected' in lib.syn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # resnet34 has blocks 10 .. 17; resnet18's 9 is its pool + heads
    m34 = models('resnet34')
    o62 = torch.full((62,), 7.0, device='cuda')
    assert m34._lib.syn_resnet_basic_block(m34._h, 9, 0, x.data_ptr(), 1, n, o62.data_ptr(), 62, None) == abi.SYN_ERR_INVALID
    assert m34._lib.syn_resnet_basic_block(m34._h, 18, 0, x.data_ptr(), 1, n, o62.data_ptr(), 62, None) == abi.SYN_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((o62 == 7.0).all())


def test_block_hook_refuses_another_arch(models, pack, backbone_sd):
    import torch
    from synergynet_amd import abi
    from synergynet_amd.synergy3DMM import SynergyNet
    v2 = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    x = torch.zeros(16 * 512, device='cuda')
    out = torch.full((62,), 7.0, device='cuda')
    assert v2._lib.syn_resnet_basic_block(v2._h, 9, 0, x.data_ptr(), 1, x.numel(), out.data_ptr(), 62, None) == abi.SYN_ERR_INVALID
    assert b'expected resnet18 or resnet34' in v2._lib.syn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize('B', [1, 7, 33])
@pytest.mark.parametrize('arch', bc.ARCHS)
def test_ragged_batches(models, arch, B):
    """B = 1: grids smaller than the 8 XCDs, the LDS kernel splits its channels over workgroups on 8^2 and 4^2; B = 7 and 33: ragged for
    every tile height of the per-layer kernels.  The default schedule and the per-layer one."""
    from synergynet_amd import synth
    model = models(arch)
    crops = synth.make_crops(B, seed=700 + B)
    want, want_pool = _want(arch, f'ragged{B}', bc.normalize_u8(crops), list(range(B)))
    for sched in (2, 0):
        with _schedule(model, sched):
            got, got_pool = model.forward_crops_u8(crops, return_pool=True)
        assert tuple(got.shape) == (B, 62) and tuple(got_pool.shape) == (B, 512)
        e_param, e_pool = rel_max(got.cpu().numpy(), want), rel_max(got_pool.cpu().numpy(), want_pool)
        print(f'{arch} B={B} schedule {sched}: param {e_param:.3g}, pool {e_pool:.3g}')
        assert e_param < TOL and e_pool < TOL


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_borders_and_neighbouring_faces(models, arch):
    """Constant 0, constant 255 and one-pixel checkerboards, every batch slot different from its neighbours: a halo that were pixel 0
    instead of normalised 0, or a tap taken from the neighbouring face, shows here.  Both inputs, both schedules."""
    import torch
    model = models(arch)
    crops = bc.border_crops()
    x = bc.normalize_u8(crops)
    want, want_pool = _want(arch, 'borders', x, list(range(len(crops))))
    runs = []
    for sched in (1, 0):
        with _schedule(model, sched):
            runs += [(f'u8 schedule {sched}', model.forward_crops_u8(crops, return_pool=True)),
                     (f'fp32 schedule {sched}', model.forward_test(torch.from_numpy(x).cuda(), return_pool=True))]
    for name, (got, got_pool) in runs:
        for i in range(len(crops)):
            e_param, e_pool = rel_max(got[i:i + 1].cpu().numpy(), want[i:i + 1]), rel_max(got_pool[i:i + 1].cpu().numpy(), want_pool[i:i + 1])
            print(f'{arch} {name} slot {i}: param {e_param:.3g}, pool {e_pool:.3g}')
            assert e_param < TOL and e_pool < TOL, f'{name} slot {i}'
        g = got.cpu().numpy()
        assert np.array_equal(g[0], g[5]) and np.array_equal(g[1], g[4]) and rel_max(g[0:1], g[1:2]) > 1e-3, name
    assert rel_max(want[0:1], want[1:2]) > 1e-3


@pytest.mark.parametrize('B', [5, 130])
@pytest.mark.parametrize('arch', bc.ARCHS)
def test_schedules_agree_bit_for_bit(models, arch, B):
    """The LDS-tiled convolutions (and the downsample from conv1's centre tap) against one launch per layer with the taps from global
    memory: the same bits, both ingests.  At 5 faces the LDS kernel runs bands everywhere, at 130 whole faces on 8^2 and 4^2 (two faces per
    workgroup there); it splits the channels of layer3 and layer4 over workgroups at both sizes."""
    import torch
    from synergynet_amd import synth
    model = models(arch)
    crops = synth.make_crops(B, seed=810 + B)
    cd = torch.from_numpy(crops).cuda()
    xd = torch.from_numpy(bc.normalize_u8(crops)).cuda()
    got = {}
    for sched in (0, 1, 2):
        with _schedule(model, sched):
            assert model._lib.syn_backbone_launch_count(model._h) == LAUNCHES[arch][min(sched, 1)]
            got[sched] = model.forward_crops_u8(cd, return_pool=True) + model.forward_test(xd, return_pool=True)
    assert all(torch.isfinite(t).all() for t in got[0])
    for sched in (1, 2):
        for a, b in zip(got[0], got[sched]):
            assert torch.equal(a, b), f'schedule {sched} differs from the per-layer one by {rel_max(a.cpu().numpy(), b.cpu().numpy()):.3g}'
    assert float(got[0][0].abs().max()) > 1e-2


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_environment_knob_selects_the_schedule(arch):
    """SYNERGY_HIP_FUSION, the documented way: 0 = per-layer, 1 = LDS-tiled."""
    from synergynet_amd.synergy3DMM import SynergyNet
    a = bc.ARCH_ID[arch]
    for knob in (0, 1):
        os.environ['SYNERGY_HIP_FUSION'] = str(knob)
        try:
            m = SynergyNet(device='cuda:0', load_constants=False, arch=arch)
            flat = np.zeros(m._lib.syn_resnet_basic_flat_count(a), np.float32)
            assert m._lib.syn_load_backbone_resnet_basic(m._h, a, flat.ctypes.data, flat.size) == 0
            assert m._lib.syn_backbone_launch_count(m._h) == LAUNCHES[arch][knob]
        finally:
            os.environ.pop('SYNERGY_HIP_FUSION', None)


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_a_face_does_not_depend_on_its_batch(models, arch):
    """One face alone, first, in the middle and last in a batch of 33: the same bits, in both schedules (no tile and no band shares
    anything between faces)."""
    import torch
    from synergynet_amd import synth
    model = models(arch)
    seq = synth.make_crops(33, seed=5200)
    want, _ = _want(arch, 'sequence', bc.normalize_u8(seq), [0])
    for sched in (0, 1):
        with _schedule(model, sched):
            alone, alone_pool = model.forward_crops_u8(torch.from_numpy(seq[:1]).cuda(), return_pool=True)
            assert rel_max(alone.cpu().numpy(), want) < TOL
            for pos in (0, 16, 32):
                batch = seq.copy()
                batch[[0, pos]] = batch[[pos, 0]]
                got, got_pool = model.forward_crops_u8(torch.from_numpy(batch).cuda(), return_pool=True)
                assert torch.equal(got[pos], alone[0]) and torch.equal(got_pool[pos], alone_pool[0]), f'schedule {sched} position {pos}'


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_numerics_entry_points_have_nothing_to_report(models, arch):
    from synergynet_amd import synth
    model = models(arch)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        n, text = model.numerics_report()
        assert n == 0 and text.count('\n') == 1 and arch in text and 'exact fp32' in text
        model.forward_crops_u8(synth.make_crops(3, seed=5))
        assert model.range_status(fallback=True)[0] == 0
        assert model.calibrate(synth.make_crops(3, seed=5)) == 0


def test_constants_export_import(models, pack, backbone_sd):
    import torch
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    crops = torch.from_numpy(synth.make_crops(5, seed=91)).cuda()
    bare = SynergyNet(device='cuda:0', load_constants=False)
    v2 = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    for src in (models('resnet18'), v2, models('resnet34'), models('resnet18')):      # one bare handle across four loads
        bare.import_constants(src.export_constants())
        assert bare.arch == src.arch and bare.pool_dim == src.pool_dim
        (a, ap), (b, bp) = src.forward_crops_u8(crops, return_pool=True), bare.forward_crops_u8(crops, return_pool=True)
        assert torch.equal(a, b) and torch.equal(ap, bp)
    assert bare.arch == 'resnet18' and bare.pool_dim == 512


@pytest.mark.parametrize('arch', bc.ARCHS)
def test_checkpoint_with_prefixed_keys_loads_and_runs(models, pack, arch, tmp_path):
    """A main_train.py checkpoint ({'state_dict': I2P.backbone.* keys}) of either depth goes through load_weights and gives the bits of
    the model built from the state directly; get_all_outputs runs on it."""
    import torch
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    fp = str(tmp_path / 'ckpt.pth.tar')
    torch.save({'state_dict': {'module.I2P.backbone.' + k: torch.from_numpy(np.asarray(v)) for k, v in _state(arch).items()}}, fp)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = SynergyNet(device='cuda:0', pack=pack, checkpoint_fp=fp, arch=arch)
    crops = torch.from_numpy(synth.make_crops(3, seed=33)).cuda()
    assert torch.equal(m.forward_crops_u8(crops), models(arch).forward_crops_u8(crops))
    one = m.get_all_outputs(synth.make_frame(180, 180, seed=4), [[-10.0, 15.0, 120.0, 150.0, 0.95]])
    assert one[0][0].shape == (3, 68) and np.isfinite(one[0][0]).all() and np.isfinite(np.asarray(one[1][0])).all()


def test_refinement_is_refused(models):
    import torch
    from synergynet_amd import abi, synth
    model = models('resnet18')
    model.load_synergy_state(synth.make_synergy_state(1))
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(2, seed=17))).cuda()
    param, pool = model.forward_test(x, return_pool=True)
    with pytest.raises(RuntimeError, match='1280-d pooled feature'):
        model.refine_landmarks(param, pool)
    out = torch.full((2, 3, 68), 7.0, device='cuda')
    rc_ = model._lib.syn_refine_landmarks(model._h, param.data_ptr(), pool.data_ptr(), 2, 1, None, None, out.data_ptr(), None, model._stream())
    assert rc_ == abi.SYN_ERR_INVALID and b'1280-d' in model._lib.syn_last_error() and b'resnet18' in model._lib.syn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_whole_path_on_frames(models):
    """get_all_outputs_frames (FaceBoxes on the device, detections kept there) on two small synthetic frames equals get_all_outputs_batch
    on the same frames array for array: the front end and the geometry stage do not depend on the backbone."""
    from synergynet_amd import synth
    from synergynet_amd.faceboxes import FaceBoxes
    m = models('resnet34')
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
