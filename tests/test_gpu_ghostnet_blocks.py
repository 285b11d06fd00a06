"""The GhostNet kernels one block at a time (syn_ghostnet_block: the launches of the forward itself, on activations the test supplies),
every element judged.  tests/test_gpu_ghostnet.py holds a block to rel_max < 1e-4 of the tensor's largest element; here
  * an integer probe (ghostnet_cases.make_integer_state / integer_faces: every partial sum of every stage is an fp32 number in any order
    of summation, and every squeeze-and-excite gate is saturated to an exact 0 or 1 that depends on the face -- conditions asserted on
    the CPU in tests/test_ghostnet_cpu.py) has to come out EQUAL to the float64 reference, output and gate / pool, on both schedules
    and on both sides of the fused kernel's batch threshold;
  * the gaussian checkpoint has to stay within the elementwise fp32 bound of ghostnet_cases.block_bound (small integers would also be
    exact on a reduced-precision matrix path; this pins fp32);
  * the blocks chained through the hook, the stem (block 18) first, equal the production forward bit for bit, and the hook refuses what
    it cannot run.
All outputs, aux included, land in NaN-filled regions between NaN sentinels, which have to survive."""
import numpy as np
import pytest

import exact_probe as ep
import ghostnet_cases as gc

pytestmark = pytest.mark.gpu
PAD = 1024                                       # floats of NaN sentinel before and after every output region
ORDER = [gc.STEM] + list(range(18))              # the forward's order
SHAPES = gc.block_shapes()


@pytest.fixture(scope='module')
def handles(pack):
    """'integer' | 'gaussian' -> (model, state_dict), built on first use"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    made = {}

    def get(kind):
        if kind not in made:
            sd = gc.make_integer_state() if kind == 'integer' else synth.make_ghostnet_state(gc.SEED)
            made[kind] = (SynergyNet(device='cuda:0', pack=pack, backbone_state=sd, arch='ghostnet'), sd)
        return made[kind]
    return get


def call_block(m, block, fused, x):
    """One block through the hook into NaN-filled buffers with NaN sentinels on both sides (aux wherever the block has one); asserts the
    sentinels untouched and the regions free of NaN.  x: numpy or device tensor in the block's layout.  Returns (out, aux | None) as
    device tensors."""
    import torch
    from synergynet_amd import abi
    x = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(m.device).contiguous()
    B = x.shape[0]
    f_in, f_out, f_aux = gc.hook_counts(block)
    assert x.dtype == torch.float32 and tuple(x.shape[1:]) == f_in
    bufs = [None if shape is None else torch.full((2 * PAD + B * int(np.prod(shape)),), float('nan'), dtype=torch.float32, device=m.device)
            for shape in (f_out, f_aux)]
    out, aux = bufs
    region = lambda b: b[PAD:b.numel() - PAD]
    abi.check(m._lib.syn_ghostnet_block(m._h, block, int(fused), x.data_ptr(), B, x.numel(), region(out).data_ptr(), region(out).numel(),
                                        region(aux).data_ptr() if aux is not None else None, region(aux).numel() if aux is not None else 0,
                                        m._stream()))
    torch.cuda.synchronize()
    for name, b in (('out', out), ('aux', aux)):
        if b is None:
            continue
        assert bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[-PAD:]).all()), f'block {block} B={B} fused={fused}: {name} sentinel overwritten'
        assert not bool(torch.isnan(region(b)).any()), f'block {block} B={B} fused={fused}: {name} not fully written'
    return region(out).view((B,) + f_out), (region(aux).view((B,) + f_aux) if aux is not None else None)


def _assert_equal(got, want64, what):
    got, want = got.cpu().numpy(), want64.astype(np.float32)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at (face, ...) = {i}: got {got[i]!r}, want {want[i]!r}')


_PROBE_REF = {}


def _probe(block, B):
    """(input, float64 out, float64 aux | None) of a probe batch: the reference is computed once on the 8 distinct faces and indexed"""
    if block not in _PROBE_REF:
        x = gc.integer_faces(block)
        _PROBE_REF[block] = (x,) + gc.probe_reference(ep.reference_state(gc.make_integer_state()), block, x)
    x, out, aux = _PROBE_REF[block]
    idx = ep.batch_index(B)
    return np.ascontiguousarray(x[idx]), out[idx], None if aux is None else aux[idx]


THRESHOLD_BLOCKS = (7, 9)          # 6.1 (ragged 92 / 40 channel tiles) and 6.3 (SE gate, shortcut), both on 8^2 maps


def probe_batches(block, fused):
    """B = 1 everywhere (3600, 900, 225, 64 and 16 pixels: every partly empty tile), B = 3 everywhere (tiles straddling faces; at 4^2 a
    partly filled 4-face workgroup), B = 5 on every 8^2 and 4^2 block and the tail, and on blocks 7 and 9 the two sides of the fused
    kernel's kGnTwoFacesMinBatch = 1024 and the odd last workgroup: 1023, 1024, 1025 (per-layer: 1025 only)."""
    small = block != gc.STEM and (block >= 16 or SHAPES[block]['hout'] <= 8)
    big = ([1023, 1024, 1025] if fused else [1025]) if block in THRESHOLD_BLOCKS else []
    return [1, 3] + ([5] if small else []) + big


def test_probe_batches_are_the_ones_the_conditions_were_checked_on():
    """tests/test_ghostnet_cpu.py checks the conditions on the 8 distinct faces and on B = 1, 3, 5; the large batches hold the same faces"""
    for fused in (0, 1):
        assert {B for b in ORDER for B in probe_batches(b, fused) if B < 8} == {1, 3, 5}
        assert [b for b in ORDER if 5 in probe_batches(b, fused)] == list(range(5, 18))
    assert set(ep.batch_index(1023)) == set(range(8))


@pytest.mark.parametrize('fused', [1, 0])
def test_integer_probe_matches_bit_for_bit(handles, fused):
    """Blocks 0..18 at every batch of probe_batches: np.array_equal with the float64 reference cast to fp32, the output and the aux (SE
    gate, pool)."""
    import torch
    m, _ = handles('integer')
    for block in ORDER:
        for B in probe_batches(block, fused):
            x, ref, ref_aux = _probe(block, B)
            out, aux = call_block(m, block, fused, torch.from_numpy(x).cuda())
            what = f'block {block} B={B} fused={fused}'
            assert (aux is None) == (ref_aux is None), what
            if aux is not None:
                _assert_equal(aux, ref_aux, what + (' pool' if block == 17 else ' gate'))
            _assert_equal(out, ref, what)


_GAUSS = {}


def _gaussian_inputs(sd):
    """block -> [(kind, x [3,...] fp32)]: the fp32 cast of the float64 reference's previous block output on real crops, and a sign-mixed
    N(0,1) tensor of the same shape -- computed once for 3 faces; B = 1 takes the first"""
    if not _GAUSS:
        from synergynet_amd import synth
        rng = np.random.default_rng(77)
        prev = synth.normalize_crops(synth.make_crops(3, seed=905))
        for block in ORDER:
            chain = np.ascontiguousarray(prev.astype(np.float32))
            noise = rng.standard_normal(chain.shape).astype(np.float32)
            assert (noise < 0).any() and (noise > 0).any()
            _GAUSS[block] = [('chain', chain), ('gauss', noise)]
            prev = gc.probe_reference(sd, block, chain)[0]
    return _GAUSS


@pytest.mark.parametrize('B', [1, 3])
def test_gaussian_checkpoint_within_the_fp32_bound(handles, B):
    """The ordinary checkpoint, every block on two inputs, on both schedules: |got - ref64| <= ghostnet_cases.block_bound elementwise
    (ghostnet_cases.judge).  SE blocks: the returned gate under its own bound, the output against a float64 block that uses the RETURNED
    gate, which isolates squeeze-and-excite from the two ghost modules.  Block 17: the pool under its bound, the heads on the returned
    pool.  Measured on an MI355X: DESIGN 5.14."""
    m, sd = handles('gaussian')
    worst = {}
    for block in ORDER:
        for kind, x in _gaussian_inputs(sd)[block]:
            for fused in (1, 0):
                out, aux = call_block(m, block, fused, x[:B])
                for name, r in gc.judge(sd, block, x[:B], out.cpu().numpy(), None if aux is None else aux.cpu().numpy()):
                    worst[block, fused, name] = max(worst.get((block, fused, name), 0.0), r)
    for fused in (1, 0):
        print(f'B={B} fused={fused} max(err / bound): ' + ', '.join(f'{b}:{n} {r:.3g}' for (b, f, n), r in worst.items() if f == fused))
    bad = {k: r for k, r in worst.items() if not r < 1.0}
    assert not bad, f'B={B}: (block, fused, part) -> err / bound {bad}'


@pytest.mark.parametrize('fused', [0, 1])
def test_chained_blocks_equal_the_production_forward(handles, fused):
    """Block 18, then 0..17 through the hook at B = 3, each output fed to the next, against forward_test on the same fp32 crops: fused = 0
    against schedule 0, fused = 1 against the default schedule.  torch.equal on param and pool."""
    import torch
    from synergynet_amd import synth
    m, _ = handles('gaussian')
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(3, seed=935))).cuda()
    if fused:
        want, want_pool = m.forward_test(x, return_pool=True)
    else:
        prev = m._lib.syn_set_schedule(m._h, 0)
        try:
            want, want_pool = m.forward_test(x, return_pool=True)
        finally:
            m._lib.syn_set_schedule(m._h, prev)
    y = x
    for block in ORDER:
        y, aux = call_block(m, block, fused, y)
    assert tuple(want.shape) == (3, 62) and torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(y, want) and torch.equal(aux, want_pool)


def test_stem_refusals_leave_buffers_and_handle_alone(handles):
    """The refusals of block 18 and of the block past it: SYN_ERR_INVALID with a message that names what was expected, before any launch
    (the NaN output stays NaN), and the handle still runs afterwards."""
    import torch
    from synergynet_amd import abi
    m, _ = handles('integer')
    lib = m._lib
    x, ref, _ = _probe(gc.STEM, 1)
    xd = torch.from_numpy(x).cuda()
    n_in, n_out = 3 * 120 * 120, 3600 * 16
    out = torch.full((n_out + 64,), float('nan'), device='cuda')
    aux = torch.full((64,), float('nan'), device='cuda')
    cases = [  # (block, fused, B, n_in, n_out, aux?, n_aux, what the message says)
        (18, 0, 1, n_in, n_out, True, 16, b'aux on block 18'), (18, 0, 1, n_in - 3, n_out, False, 0, b'n_in='),
        (18, 0, 1, n_in, n_out + 64, False, 0, b'n_out='), (18, 1, 2, n_in, n_out, False, 0, b'B=2'), (18, 0, 1, n_in, n_out, False, 16, b'n_aux='),
        (18, 0, 1, 3600 * 16, n_out, False, 0, b'n_in='), (19, 0, 1, n_in, n_out, False, 0, b'block=19'), (18, 2, 1, n_in, n_out, False, 0, b'fused=2'),
    ]
    for block, fused, B, ni, no, with_aux, na, word in cases:
        rc = lib.syn_ghostnet_block(m._h, block, fused, xd.data_ptr(), B, ni, out.data_ptr(), no, aux.data_ptr() if with_aux else None, na, m._stream())
        err = lib.syn_last_error()
        assert rc == abi.SYN_ERR_INVALID, (block, fused, B, ni, no, with_aux, na)
        assert b'syn_ghostnet_block' in err and b'expected' in err and word in err, err
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(aux).all())
    for fused in (0, 1):                                                     # `fused` selects nothing on the stem
        _assert_equal(call_block(m, gc.STEM, fused, xd)[0], ref, f'after the refusals, fused={fused}')
