"""The BasicBlock ResNet kernels one block at a time (syn_resnet_basic_block: the launches of the forward itself, on activations the test
supplies), every element judged.  tests/test_gpu_resnet_basic.py holds a block to rel_max < 1e-4 of the tensor's largest element and, in
its grid cases, to the other schedule; here
  * an integer probe (resnet_basic_cases.make_integer_state / integer_faces: every partial sum of every stage is an fp32 number in any
    order of summation -- conditions asserted on the CPU in tests/test_resnet_basic_cpu.py) has to come out EQUAL to the float64
    reference, on both schedules, on every face of every launcher grid;
  * the gaussian checkpoint has to stay within the elementwise fp32 bound of resnet_basic_cases.block_bound (small integers would also
    be exact on a reduced-precision matrix path; this pins fp32);
  * the blocks chained through the hook equal the production forward bit for bit.
All outputs land in NaN-filled regions between NaN sentinels, which have to survive."""
import numpy as np
import pytest

import exact_probe as ep
import resnet_basic_cases as bc

pytestmark = pytest.mark.gpu
PAD = 1024                                       # floats of NaN sentinel before and after the output region
SHAPES = {a: bc.block_shapes(a) for a in bc.ARCHS}


@pytest.fixture(scope='module')
def handles(pack):
    """(arch, 'integer' | 'gaussian') -> (model, state_dict), built on first use"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    made = {}

    def get(arch, kind):
        if (arch, kind) not in made:
            sd = bc.make_integer_state(arch) if kind == 'integer' else synth.make_resnet_basic_state(arch, bc.SEED)
            made[arch, kind] = (SynergyNet(device='cuda:0', pack=pack, backbone_state=sd, arch=arch), sd)
        return made[arch, kind]
    return get


def _out_shape(arch, block, B):
    s = SHAPES[arch][block]
    return (B, 62) if block == bc.last_block(arch) else (B, s['hout'], s['hout'], s['cout'])


def call_block(m, block, fused, x):
    """One block through the hook into a NaN-filled buffer with NaN sentinels on both sides; asserts the sentinels untouched and the region
    free of NaN.  x: numpy or device tensor in the block's layout.  Returns the output as a device tensor."""
    import torch
    from synergynet_amd import abi
    x = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(m.device).contiguous()
    B = x.shape[0]
    shape = _out_shape(m.arch, block, B)
    assert x.dtype == torch.float32
    buf = torch.full((2 * PAD + int(np.prod(shape)),), float('nan'), dtype=torch.float32, device=m.device)
    out = buf[PAD:buf.numel() - PAD]
    abi.check(m._lib.syn_resnet_basic_block(m._h, block, int(fused), x.data_ptr(), B, x.numel(), out.data_ptr(), out.numel(), m._stream()))
    torch.cuda.synchronize()
    what = f'{m.arch} block {block} B={B} fused={fused}'
    assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all()), what + ': sentinel overwritten'
    assert not bool(torch.isnan(out).any()), what + ': output not fully written'
    return out.view(shape)


def _assert_equal(got, want64, what):
    got, want = got.cpu().numpy(), want64.astype(np.float32)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at (face, y, x, channel) = {i}: got {got[i]!r}, want {want[i]!r}')


_PROBE_REF = {}


def _probe_faces(arch, block):
    """(the 8 distinct faces, their float64 reference), computed once per block; a batch of any size indexes them"""
    if (arch, block) not in _PROBE_REF:
        x = bc.integer_faces(arch, block)
        _PROBE_REF[arch, block] = (x, bc.block_reference(ep.reference_state(bc.make_integer_state(arch)), arch, block, x))
    return _PROBE_REF[arch, block]


def _probe(arch, block, B):
    x, ref = _probe_faces(arch, block)
    idx = ep.batch_index(B)
    return np.ascontiguousarray(x[idx]), ref[idx]


@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('arch', bc.ARCHS)
def test_integer_probe_matches_bit_for_bit(handles, arch, fused):
    """Every block (0 = stem + max pool, the BasicBlocks, pool + heads) at B = 1 (900 / 225 / 64 / 16 pixels: every partly empty tile, and on
    30^2 the last band of 2 rows) and B = 3 (tiles and bands next to another face): np.array_equal with the float64 reference cast to
    fp32."""
    m, _ = handles(arch, 'integer')
    for block in range(len(SHAPES[arch])):
        for B in (1, 3):
            x, ref = _probe(arch, block, B)
            _assert_equal(call_block(m, block, fused, x), ref, f'{arch} block {block} ({SHAPES[arch][block]["key"]}) B={B} fused={fused}')


@pytest.mark.parametrize('name,B,what', bc.GRID_CASES, ids=[f'{n}-B{b}' for n, b, _ in bc.GRID_CASES])
def test_integer_probe_on_every_launcher_grid(handles, name, B, what):
    """Every grid-shape branch of the LDS kernel's launcher at its own batch size: the LDS-tiled output equals the float64 reference on
    EVERY face, and so does the per-layer output -- an independent reference where test_launcher_grids has the other schedule."""
    arch = 'resnet18'
    m, _ = handles(arch, 'integer')
    block = [s['key'] for s in SHAPES[arch]].index(name)
    x, ref = _probe(arch, block, B)
    import torch
    xd = torch.from_numpy(x).cuda()
    for fused in (1, 0):
        _assert_equal(call_block(m, block, fused, xd), ref, f'{name} B={B} fused={fused} ({what})')


_GAUSS = {}


def _gaussian_cases(arch, sd):
    """per block [(kind, x [3,...] fp32, float64 reference, bound)]: the fp32 cast of the float64 reference's previous block output on real
    crops, and a sign-mixed N(0,1) tensor of the same shape -- computed once for 3 faces; B = 1 takes the first"""
    if arch not in _GAUSS:
        from synergynet_amd import synth
        rng = np.random.default_rng([77, bc.ARCH_ID[arch]])
        prev, cases = synth.normalize_crops(synth.make_crops(3, seed=903)), []
        for block in range(len(SHAPES[arch])):
            chain = np.ascontiguousarray(prev.astype(np.float32))
            noise = rng.standard_normal(chain.shape).astype(np.float32)
            assert (noise < 0).any() and (noise > 0).any()
            both = []
            for kind, x in (('chain', chain), ('gauss', noise)):
                both.append((kind, x, bc.block_reference(sd, arch, block, x), bc.block_bound(sd, arch, block, x)))
            prev = both[0][2]
            cases.append(both)
        _GAUSS[arch] = cases
    return _GAUSS[arch]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('arch', bc.ARCHS)
def test_gaussian_checkpoint_within_the_fp32_bound(handles, arch, B):
    """The ordinary checkpoint, every block on two inputs, on both schedules: |got - ref64| <= block_bound elementwise.  The block has no
    intermediate output, so the bound carries conv1's through conv2 and adds the downsample's own; the last block carries the 16-term
    mean's through the heads.  Measured on an MI355X: DESIGN 5.16."""
    m, sd = handles(arch, 'gaussian')
    worst = {}
    for block, both in enumerate(_gaussian_cases(arch, sd)):
        for kind, x, ref, bound in both:
            for fused in (1, 0):
                got = call_block(m, block, fused, x[:B]).cpu().numpy()
                worst[block, fused] = max(worst.get((block, fused), 0.0), ep.bound_ratio(got, ref[:B], bound[:B]))
    for fused in (1, 0):
        print(f'{arch} B={B} fused={fused} max(err / bound): ' + ', '.join(f'{b}:{r:.3g}' for (b, f), r in sorted(worst.items()) if f == fused))
    bad = {k: r for k, r in worst.items() if not r < 1.0}
    assert not bad, f'{arch} B={B}: (block, fused) -> err / bound {bad}'


@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('arch', bc.ARCHS)
def test_chained_blocks_equal_the_production_forward(handles, arch, fused):
    """Blocks 0 .. last through the hook at B = 3, each output fed to the next, against forward_test on the same fp32 crops: the per-layer
    launches against schedule 0, the LDS-tiled ones against the default schedule.  torch.equal on the 62 parameters."""
    import torch
    from synergynet_amd import synth
    m, _ = handles(arch, 'gaussian')
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(3, seed=934))).cuda()
    if fused:
        want = m.forward_test(x)
    else:
        prev = m._lib.syn_set_schedule(m._h, 0)
        try:
            want = m.forward_test(x)
        finally:
            m._lib.syn_set_schedule(m._h, prev)
    y = x
    for block in range(len(SHAPES[arch])):
        y = call_block(m, block, fused, y)
    assert tuple(want.shape) == (3, 62) and torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(y, want)
