"""The ResNeSt-50 kernels one block at a time (syn_resnest50_block: the launches of the forward itself, on activations the test supplies),
every element judged.  tests/test_gpu_resnest.py holds a block to rel_max < 1e-4 of the tensor's largest element; here
  * an integer probe (resnest_cases.make_integer_state / integer_faces: every partial sum of every stage is an fp32 number in any order
    of summation, the avd pool's product with fl(1 / 9) is exact, and every attention is an exact 0, 0.5 or 1 that depends on the face --
    conditions asserted on the CPU in tests/test_resnest_cpu.py) has to come out EQUAL to the float64 reference, output and attention /
    pool, on both schedules, and at every grid the fused tail takes (resnest_cases.TAIL_CASES), every face of every batch;
  * the gaussian checkpoint has to stay within the elementwise fp32 bound of resnest_cases.block_bound (small integers would also be
    exact on a reduced-precision matrix path; this pins fp32), and the gate state -- the probe's exact U in front of an ordinary gate --
    within the gate's own bound, which is the one a wrong gate input cannot hide under;
  * the blocks chained through the hook equal both production entry points bit for bit.
All outputs, aux included, land in NaN-filled regions between NaN sentinels, which have to survive."""
import numpy as np
import pytest

import exact_probe as ep
import resnest_cases as rc

pytestmark = pytest.mark.gpu
PAD = 1024                                       # floats of NaN sentinel before and after every output region
SHAPES = rc.block_shapes()
NAMES = [s['key'] for s in SHAPES]


@pytest.fixture(scope='module')
def handles(pack):
    """'integer' | 'gaussian' | 'gate' -> (model, state_dict), built on first use"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    made = {}
    states = {'integer': rc.make_integer_state, 'gate': rc.make_gate_state, 'gaussian': lambda: synth.make_resnest50_state(rc.SEED)}

    def get(kind):
        if kind not in made:
            sd = states[kind]()
            made[kind] = (SynergyNet(device='cuda:0', pack=pack, backbone_state=sd, arch='resnest50'), sd)
        return made[kind]
    return get


def call_block(m, block, fused, x):
    """One block through the hook into NaN-filled buffers with NaN sentinels on both sides (aux wherever the block has one); asserts the
    sentinels untouched and the regions free of NaN.  x: numpy or device tensor, NHWC.  Returns (out, aux | None) as device tensors."""
    import torch
    from synergynet_amd import abi
    x = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(m.device).contiguous()
    B = x.shape[0]
    f_in, f_out, f_aux = rc.hook_counts(block)
    assert x.dtype == torch.float32 and tuple(x.shape[1:]) == f_in
    bufs = [None if shape is None else torch.full((2 * PAD + B * int(np.prod(shape)),), float('nan'), dtype=torch.float32, device=m.device)
            for shape in (f_out, f_aux)]
    out, aux = bufs
    region = lambda b: b[PAD:b.numel() - PAD]
    abi.check(m._lib.syn_resnest50_block(m._h, block, int(fused), x.data_ptr(), B, x.numel(), region(out).data_ptr(), region(out).numel(),
                                         region(aux).data_ptr() if aux is not None else None, region(aux).numel() if aux is not None else 0,
                                         m._stream()))
    torch.cuda.synchronize()
    for name, b in (('out', out), ('aux', aux)):
        if b is None:
            continue
        assert bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[-PAD:]).all()), f'block {block} B={B} fused={fused}: {name} sentinel overwritten'
        assert not bool(torch.isnan(region(b)).any()), f'block {block} B={B} fused={fused}: {name} not fully written'
    return region(out).view((B,) + f_out), (region(aux).view((B,) + f_aux) if aux is not None else None)


def _assert_equal(got, want, what):
    """device tensors; the message names the first differing element and both values"""
    import torch
    assert got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {len(bad)} of {got.numel()} elements differ, first at (face, ...) = {i}: got {got[i].item()!r}, want {want[i].item()!r}')


_PROBE_REF = {}


def _probe_faces(block):
    """(input, float64 out cast to fp32, float64 aux cast to fp32 | None) of the 8 distinct faces on the device, computed once per block"""
    import torch
    if block not in _PROBE_REF:
        x = rc.integer_faces(block)
        out, aux = rc.probe_reference(ep.reference_state(rc.make_integer_state()), block, x)
        _PROBE_REF[block] = tuple(None if t is None else torch.from_numpy(np.ascontiguousarray(t.astype(np.float32))).cuda() for t in (x, out, aux))
    return _PROBE_REF[block]


def _run_probe(m, block, B, fused):
    """a probe batch built on the device by indexing the 8 faces, every face compared with the float64 reference there"""
    import torch
    x, ref, ref_aux = _probe_faces(block)
    idx = torch.from_numpy(ep.batch_index(B)).cuda()
    out, aux = call_block(m, block, fused, x[idx])
    what = f'block {block} ({NAMES[block]}) B={B} fused={fused}'
    assert (aux is None) == (ref_aux is None), what
    if aux is not None:
        _assert_equal(aux, ref_aux[idx], what + (' pool' if block == rc.TAIL else ' attention'))
    _assert_equal(out, ref[idx], what)


def probe_batches(block):
    """B = 1 everywhere (900, 225, 64 and 16 pixels: every partly empty tile), B = 3 everywhere (tiles straddling faces, three different
    attentions), B = 5 where a face has at most 64 output pixels and on the tail"""
    return [1, 3] + ([5] if block == rc.TAIL or (block > 0 and SHAPES[block]['hout'] <= 8) else [])


def test_probe_batches_are_the_ones_the_conditions_were_checked_on():
    """tests/test_resnest_cpu.py checks the conditions on the 8 distinct faces and on B = 1, 3, 5; the large batches hold the same faces"""
    assert {B for b in range(18) for B in probe_batches(b)} == {1, 3, 5}
    assert [b for b in range(18) if 5 in probe_batches(b)] == list(range(NAMES.index('layer3.0'), 18))
    assert all(set(ep.batch_index(B)) == set(range(8)) for _, B, _ in rc.TAIL_CASES if B >= 8)


@pytest.mark.parametrize('fused', [1, 0])
def test_integer_probe_matches_bit_for_bit(handles, fused):
    """Blocks 0..17 at every batch of probe_batches: equal to the float64 reference cast to fp32, the output and the aux (attention,
    pool).  A device whose expf(0) is not 1 or whose expf(-104 and below) is not 0 fails here, on the attention, and the message says so."""
    m, _ = handles('integer')
    for block in range(18):
        for B in probe_batches(block):
            _run_probe(m, block, B, fused)


@pytest.mark.parametrize('key,B,what', rc.TAIL_CASES, ids=[f'{k}-{B}' for k, B, _ in rc.TAIL_CASES])
def test_integer_probe_at_every_grid_of_the_fused_tail(handles, key, B, what):
    """resnest_cases.TAIL_CASES (tests/test_resnest_cpu.py holds the table against the launcher's rule): the fused schedule at every
    batch, the per-layer schedule at the largest batch of the block; every face of the batch against float64."""
    m, _ = handles('integer')
    block = NAMES.index(key)
    _run_probe(m, block, B, 1)
    if B == max(b for k, b, _ in rc.TAIL_CASES if k == key):
        _run_probe(m, block, B, 0)


_GAUSS, _PARTS = {}, {}


def _gaussian_inputs(sd):
    """block -> [(kind, x [3,...] fp32)]: the fp32 cast of the float64 reference's previous block output on real crops, and a sign-mixed
    N(0,1) tensor of the same shape -- computed once for 3 faces; B = 1 takes the first"""
    if not _GAUSS:
        from synergynet_amd import synth
        rng = np.random.default_rng(77)
        prev = synth.normalize_crops(synth.make_crops(3, seed=905)).transpose(0, 2, 3, 1)
        for block in range(18):
            chain = np.ascontiguousarray(prev.astype(np.float32))
            noise = rng.standard_normal(chain.shape).astype(np.float32)
            assert (noise < 0).any() and (noise > 0).any()
            _GAUSS[block] = [('chain', chain), ('gauss', noise)]
            prev = rc.probe_reference(sd, block, chain)[0]
    return _GAUSS


def _parts(sd, block, kind, x, aux):
    """resnest_cases.judge_parts, computed once per returned aux (the two schedules run the same gate kernel)"""
    key = (block, kind, x.shape[0], None if aux is None else aux.tobytes())
    if key not in _PARTS:
        _PARTS[key] = rc.judge_parts(sd, block, x, aux)
    return _PARTS[key]


@pytest.mark.parametrize('B', [1, 3])
def test_gaussian_checkpoint_within_the_fp32_bound(handles, B):
    """The ordinary checkpoint, every block on two inputs, on both schedules: |got - ref64| <= resnest_cases.block_bound elementwise.
    Bottlenecks: the returned attention under its own bound, the output against a float64 tail that uses the RETURNED attention, which
    isolates the gate from the convolutions.  Block 17: the pool under its bound, the heads on the returned pool.  Measured on an
    MI355X: DESIGN 5.15."""
    m, sd = handles('gaussian')
    worst = {}
    for block in range(18):
        for kind, x in _gaussian_inputs(sd)[block]:
            for fused in (1, 0):
                out, aux = call_block(m, block, fused, x[:B])
                results = {'out': out.cpu().numpy(), 'aux': None if aux is None else aux.cpu().numpy()}
                for name, which, ref, bound in _parts(sd, block, kind, x[:B], results['aux']):
                    worst[block, fused, name] = max(worst.get((block, fused, name), 0.0), ep.bound_ratio(results[which], ref, bound))
    for fused in (1, 0):
        print(f'B={B} fused={fused} max(err / bound): ' + ', '.join(f'{b}:{n} {r:.3g}' for (b, f, n), r in worst.items() if f == fused))
    bad = {k: r for k, r in worst.items() if not r < 1.0}
    assert not bad, f'B={B}: (block, fused, part) -> err / bound {bad}'


def test_gate_state_attention_within_the_gate_bound(handles):
    """resnest_cases.make_gate_state on the probe's faces at B = 1, 3 and 5, both schedules: the attention of every bottleneck within the
    gate's own fp32 bound, which starts from an exact U (resnest_cases.gate_reference).  A gap from one radix half, a gap divided by the
    wrong pixel count or a dropped fc1 bias is more than 100 x that bound on every block, a gap that misses a pixel more than 4 x
    (tests/test_resnest_cpu.py::test_every_variant_bites)."""
    m, sd = handles('gate')
    ref_sd, worst = rc.gate_reference_state(sd), {}
    for block in range(1, 17):
        for B in (1, 3, 5):
            x = rc.integer_input(block, B)
            att, bound = rc.gate_reference(ref_sd, block, x)
            for fused in (1, 0):
                _, aux = call_block(m, block, fused, x)
                worst[block, fused] = max(worst.get((block, fused), 0.0), ep.bound_ratio(aux.cpu().numpy(), att, bound))
    print('max(err / bound) of the attention: ' + ', '.join(f'{b}/{f} {r:.3g}' for (b, f), r in worst.items()))
    bad = {k: r for k, r in worst.items() if not r < 1.0}
    assert not bad, f'(block, fused) -> err / bound {bad}'


@pytest.mark.parametrize('fused', [0, 1])
def test_chained_blocks_equal_the_production_forward(handles, fused):
    """Blocks 0..17 through the hook at B = 3, each output fed to the next, against forward_test on the same fp32 crops and against
    forward_crops_u8 on the uint8 crops they were normalised from: fused = 0 against schedule 0, fused = 1 against the default schedule.
    torch.equal on param and pool (the stem's three ingest paths add the same 27 terms in the same order)."""
    import torch
    from synergynet_amd import synth
    m, _ = handles('gaussian')
    crops = synth.make_crops(3, seed=935)
    x = torch.from_numpy(synth.normalize_crops(crops)).cuda()
    prev = m._lib.syn_set_schedule(m._h, 0) if not fused else None
    try:
        want, want_pool = m.forward_test(x, return_pool=True)
        want8, want8_pool = m.forward_crops_u8(torch.from_numpy(crops).cuda(), return_pool=True)
    finally:
        if not fused:
            m._lib.syn_set_schedule(m._h, prev)
    y = x.permute(0, 2, 3, 1).contiguous()
    for block in range(18):
        y, aux = call_block(m, block, fused, y)
    assert tuple(want.shape) == (3, 62) and torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(y, want) and torch.equal(aux, want_pool)
    assert torch.equal(y, want8) and torch.equal(aux, want8_pool)
