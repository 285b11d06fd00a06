"""ResNet-50 one span at a time (syn_resnet50_span: run_resnet50 itself, entered at block `first` and left behind block `last`, on activations
the test supplies), every element judged, at every batch size where a launcher picks another kernel variant.  The end-to-end tests
(tests/test_gpu_parity.py, test_gpu_fullsize.py, test_gpu_numerics.py) see the 62 parameters behind 16 bottlenecks and compare schedules
with each other; here
  * an integer probe per block (resnet50_cases.make_integer_state / integer_faces: every partial sum is an fp32 number in any order, every
    weight one fp16 piece, every split activation inside the guard's window and within 22 bits, two channels NEEDING the low piece --
    conditions asserted on the CPU in tests/test_resnet50_cpu.py) has to come out EQUAL to the float64 reference, on six handles (resnet50_cases.SCHEDULES), with
    the launch tags resnet50_cases.expected_tags reads off the launchers and the guard maxima equal to max |reference tensor|;
  * the spans chained in the forward's own partition equal the production forward bit for bit, and the hook refuses what it cannot run.
A batch is eight distinct faces, slot i holding face (5 i + 3) % 8; references are computed for the eight faces once and gathered on the
device; a block's batches run largest first, the smaller ones over a workspace left dirty."""
import ctypes
import os

import numpy as np
import pytest

import resnet50_cases as rc

pytestmark = pytest.mark.gpu
PAD = 1024                                       # floats of NaN sentinel before and after every output region
AUX_WRITTEN = 0x10000                            # include/synergy_hip.h SYN_SPAN_AUX_WRITTEN
SCHEDS = list(rc.SCHEDULES)
TWO_BLOCK = [(1, 2), (3, 4), (4, 5), (7, 8), (16, 17)]


@pytest.fixture(scope='module')
def handles(pack):
    """(schedule, 'integer' | 'gaussian') -> (model, state_dict), built on first use; the schedule variables are read at syn_create"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    made = {}

    def get(sched, kind):
        if (sched, kind) not in made:
            sd = rc.make_integer_state() if kind == 'integer' else synth.make_resnet50_state()
            os.environ.update(rc.SCHEDULES[sched])
            try:
                m = SynergyNet(device='cuda:0', pack=pack, backbone_state=sd, arch='resnet50')
            finally:
                for k in rc.SCHEDULES[sched]:
                    os.environ.pop(k, None)
            assert m.numerics_report()[0] == 0, m.numerics_report()[1]        # no convolution fell back: the probes judge the kernels they name
            m._range_checked = True                                           # (the spans are judged here, not by the first-forward host check)
            made[sched, kind] = (m, sd)
        return made[sched, kind]
    return get


def call_span(m, first, last, x, want_aux=False):
    """Runs one span through the hook into NaN-filled buffers with NaN sentinels on both sides; asserts the sentinels untouched and the
    written regions free of NaN; an aux the hook reports as not written has to be untouched.  x: device tensor in the span's input layout
    (uint8 -> in_u8).  Returns (out, aux | None, launch tags)."""
    import torch
    from synergynet_amd import abi
    x = x.contiguous()
    B = x.shape[0]
    n_in, out_shape, aux_shape = rc.span_counts(first, last, B, want_aux)
    assert x.numel() == n_in and x.dtype in (torch.uint8, torch.float32) and x.is_cuda
    bufs = [None if shape is None else torch.full((2 * PAD + int(np.prod(shape)),), float('nan'), dtype=torch.float32, device=m.device)
            for shape in (out_shape, aux_shape)]
    out, aux = bufs
    region = lambda b: b[PAD:b.numel() - PAD]
    tags = (ctypes.c_int * 160)()
    n = m._lib.syn_resnet50_span(m._h, first, last, x.data_ptr(), int(x.dtype == torch.uint8), B, n_in, region(out).data_ptr(), region(out).numel(),
                                 region(aux).data_ptr() if aux is not None else None, region(aux).numel() if aux is not None else 0, tags, 160,
                                 m._stream())
    if n < 0:
        abi.check(n)
    torch.cuda.synchronize()
    aux_written = bool(n & AUX_WRITTEN) or (aux is not None and last == 17)
    n &= AUX_WRITTEN - 1
    what = f'blocks {first}-{last} B={B}'
    for name, b, written in (('out', out, True), ('aux', aux, aux_written)):
        if b is None:
            continue
        assert bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[-PAD:]).all()), f'{what}: {name} sentinel overwritten'
        if written:
            assert not bool(torch.isnan(region(b)).any()), f'{what}: {name} not fully written'
        else:
            assert bool(torch.isnan(region(b)).all()), f'{what}: {name} reported as not written, but touched'
    return region(out).view(out_shape), (region(aux).view(aux_shape) if aux_written and aux is not None else None), list(tags[:n])


def _first_difference(got, want):
    bad = (got != want).nonzero()
    i = tuple(int(v) for v in bad[0])
    return f'{len(bad)} of {got.numel()} elements differ, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}'


def _assert_equal(got, want, what):
    import torch
    assert got.shape == want.shape, what
    assert torch.equal(got, want), f'{what}: {_first_difference(got, want)}'


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _index(B):
    import torch
    return torch.from_numpy(rc.batch_index(B)).cuda()


def _integer_probe(first, last, u8=True):
    """(device faces in the span's input layout, float64 reference of the eight faces cast to fp32 on the device: (out, aux | None), the
    guard maxima per face)"""
    import torch

    def make():
        faces, x = rc.integer_faces(first), rc.probe_input(first)
        sd_ref = rc.reference_state(rc.make_integer_state())
        refs = tuple(None if r is None else torch.from_numpy(np.ascontiguousarray(r).astype(np.float32)).cuda() for r in rc.span_reference(sd_ref, first, last, x))
        return torch.from_numpy(faces if (u8 or first) else x).cuda(), refs, rc.guard_maxima(sd_ref, first, last, x)
    return _cached(('int', first, last, u8), make)


def _run_probe(m, sched, first, last, batches, u8=True, check_aux=True):
    """the integer probe of one span on one handle at the given batches: out (and aux where a fused launch wrote it) equal to the reference,
    the tags equal to expected_tags, the guard maxima equal to max |reference tensor| on an fp16 x2 handle and all 1 on an fp32 one"""
    fusion, fuse, gemm = rc.schedule_args(sched)
    faces, refs, maxima = _integer_probe(first, last, u8)
    seen = set()
    for B in batches:
        idx = _index(B)
        out, aux, tags = call_span(m, first, last, faces[idx], want_aux=check_aux and (last == 17 or 1 <= last <= 15))
        want_tags, fused = rc.expected_tags(first, last, B, fusion, fuse, gemm, in_u8=u8)
        what = f'{sched} blocks {first}-{last} B={B} launches {tags}'
        assert tags == want_tags, what + f', expected {want_tags}'
        seen |= {t % 1000 for t in tags}
        _assert_equal(out, refs[0][idx], what + (' param' if last == 17 else ''))
        if check_aux and (last == 17 or 1 <= last <= 15):
            assert (aux is not None) == (fused or last == 17), what + ': aux written <=> a fused launch ended the span'
            if aux is not None:
                _assert_equal(aux, refs[1][idx], what + (' pool' if last == 17 else ' fused conv1'))
        if first != last and fused:           # (the third block's conv1 behind a two-block span is not exact and may leave the window)
            continue
        n_bad, mx = m.range_status()
        want_mx = rc.guard_expected(maxima, last, rc.batch_index(B), fused) if fusion >= 2 else np.ones(54, np.float32)
        assert n_bad == 0 and np.array_equal(mx, want_mx), what + f': guard maxima differ in slots {np.flatnonzero(mx != want_mx).tolist()}: ' \
            f'got {mx[mx != want_mx].tolist()}, want {want_mx[mx != want_mx].tolist()}'
    return seen


@pytest.mark.parametrize('block', range(18))
@pytest.mark.parametrize('sched', SCHEDS)
def test_integer_probe_matches_bit_for_bit(handles, sched, block):
    """Every block 0..17 alone at every batch of resnet50_cases.probe_batches (both sides of every threshold of the launchers, 1, 3 and an odd
    batch above the last threshold; largest first), on the default schedule, SYNERGY_HIP_RESNET_FUSE=0 (conv3 and conv1 as launches of their
    own) and =1 (fused, without conv2 in front), SYNERGY_HIP_RESNET_GEMM=0 and =2, and SYNERGY_HIP_FUSION=1 (the exact conv_kernel throughout): torch.equal with the float64
    reference cast to fp32 for `out` and, where a fused launch ended the block, for the next block's conv1 it also produced; tags equal to
    expected_tags; guard maxima equal to max |reference tensor| in the slots the span produced and 1 in every other."""
    m, _ = handles(sched, 'integer')
    _run_probe(m, sched, block, block, rc.probe_batches(block, sched))


@pytest.mark.parametrize('sched', SCHEDS)
def test_integer_probe_on_the_stem_from_fp32_crops(handles, sched):
    """fp32 CHW crops never take the matrix-pipe stem: the direct kernel and the max-pool at 1, 3 and 129 faces"""
    m, _ = handles(sched, 'integer')
    seen = _run_probe(m, sched, 0, 0, [129, 3, 1], u8=False)
    assert seen == {rc.TAG_STEM, rc.TAG_MAXPOOL}


@pytest.mark.parametrize('first,last', TWO_BLOCK, ids=[f'{a}-{b}' for a, b in TWO_BLOCK])
@pytest.mark.parametrize('sched', SCHEDS)
def test_integer_probe_on_two_block_spans(handles, sched, first, last):
    """Two blocks in one span: the second takes its conv1 from the fused launch of the first where the schedule fuses (1-2: the DS form of
    layer1.0; 4-5: layer2.0 with its separately computed fp32 identity), as in production.  The probe stays exact through the second block
    (tests/test_resnet50_cpu.py); the conv1 of a third block that a fused launch at the end also produces is not exact any more and is not
    asked for.  16-17: the last bottleneck's fp32 output into pool and heads."""
    m, _ = handles(sched, 'integer')
    _run_probe(m, sched, first, last, [21, 3], check_aux=last == 17)


def _ratio(got, ref, bound):
    """max |got - ref| / bound on the device, float64; an element whose bound is 0 has to match exactly"""
    import torch
    err = (got.double() - ref).abs()
    assert err.shape == bound.shape
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(r.max())


def _gaussian_case(sd, block, sched, B):
    """(device input faces, float64 references (out, aux) on the device, bounds (out, aux) on the device) of one block of the gaussian
    checkpoint; the bound depends on the batch only through the kernels that change the arithmetic (matrix-pipe stem, DUAL GEMM)"""
    import torch
    fusion, fuse, gemm = rc.schedule_args(sched)
    codes = tuple(t for t in rc.block_tags(block, B, fusion, fuse, gemm)[0] if t in (rc.TAG_STEM, rc.TAG_DUAL))
    xs = _cached('gin', lambda: rc.gaussian_inputs(sd))

    def make():
        x = xs[block]
        xr = rc.normalize_u8(x) if block == 0 else x
        dev = lambda r: None if r is None else torch.from_numpy(np.ascontiguousarray(r)).cuda()
        return tuple(dev(r) for r in rc.span_reference(sd, block, block, xr)), tuple(dev(b) for b in rc.span_bound(sd, block, block, xr, fusion, fuse, gemm, B))
    refs, bounds = _cached(('gref', block, fusion >= 2, codes), make)
    return _cached(('gdev', block), lambda: torch.from_numpy(xs[block]).cuda()), refs, bounds


@pytest.mark.parametrize('block', range(18))
@pytest.mark.parametrize('sched', SCHEDS)
def test_gaussian_checkpoint_within_the_bound(handles, sched, block):
    """The ordinary checkpoint (synth.make_resnet50_state), every block alone at one batch per kernel variant (resnet50_cases.variant_batches),
    on the fp32 cast of the float64 reference's previous activation on real crops: |got - ref64| <= resnet50_cases.span_bound elementwise --
    exact_probe.conv_bn_pair on the fp32 handle, the split terms, 3 n summands and floors on the fp16 x2 handles -- for `out` and for the conv1
    a fused launch also produces.  Block 17: the pool by its bound, the 62 outputs against a float64 head on the RETURNED pool.  Measured on
    an MI355X: DESIGN 5.11a.  No other tolerance."""
    import torch
    m, sd = handles(sched, 'gaussian')
    worst = {}
    for B in rc.variant_batches(block, sched):
        x, refs, bounds = _gaussian_case(sd, block, sched, B)
        idx = torch.from_numpy(rc.batch_index(B, rc.N_GAUSS)).cuda()
        out, aux, tags = call_span(m, block, block, x[idx], want_aux=block == 17 or 1 <= block <= 15)
        key = (B, tuple(t % 1000 for t in tags))
        if block == 17:
            worst[key + ('pool',)] = _ratio(aux, refs[1][idx], bounds[1][idx])
            pool = aux.cpu().numpy()
            worst[key + ('heads',)] = rc.bound_ratio(out.cpu().numpy(), rc.heads_reference(sd, pool).numpy(), rc.heads_bound(sd, pool))
        else:
            worst[key] = _ratio(out, refs[0][idx], bounds[0][idx])
            if aux is not None:
                worst[key + ('fused conv1',)] = _ratio(aux, refs[1][idx], bounds[1][idx])
    print(f'{sched} block {block} max(err / bound): ' + ', '.join(f'{k} {r:.3g}' for k, r in worst.items()))
    bad = {k: r for k, r in worst.items() if not r <= 1.0}
    assert not bad, f'{sched} block {block}: err / bound {bad}'


def test_integer_probe_past_the_32bit_window(handles):
    """One middle block of layer 1 at the smallest batch whose input reaches 2 GiB (2331 faces x 30 x 30 x 256 x 4 bytes): conv1 has to leave
    the buffer-load kernels for conv_f16x2_kernel (64-bit addressing), conv2 + conv3 + the next conv1 stay one fused launch (its T1 is below
    2 GiB).  Equal to the reference, compared on the device only.  Runs once."""
    B = 2331
    assert B * 900 * 256 * 4 >= 2 ** 31 > (B - 1) * 900 * 256 * 4
    m, _ = handles('default', 'integer')
    tags, fused = rc.expected_tags(2, 2, B)
    assert tags == [2000 + 22, 2000 + 100 + 2 + 1] and fused
    _run_probe(m, 'default', 2, 2, [B])


# The lt_glds / lt_stage knobs are read once per process (SYNERGY_HIP_TEST_KNOBS): one fresh child per knob set, each under its own time limit,
# runs the integer probe (this module's helpers) of blocks with LDS-tiled GEMMs at two batches and prints the tags; a mismatch is its non-zero
# exit.  Layer 1's blocks launch no LDS-tiled GEMM under the default fusion (conv1 has 64 output channels, the rest is one fused launch).
KNOB_BLOCKS = [(7, (293, 21)), (8, (511, 125)), (9, (511, 65)), (15, (1011, 257))]
KNOB_CHILD = r'''
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import torch
import resnet50_cases as rc
import test_gpu_resnet50_spans as t
from synergynet_amd import synth
from synergynet_amd.synergy3DMM import SynergyNet
m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(n_vert=640), backbone_state=rc.make_integer_state(), arch='resnet50')
assert m.numerics_report()[0] == 0
m._range_checked = True
tags = {}
for block, batches in t.KNOB_BLOCKS:
    faces, refs, _ = t._integer_probe(block, block)
    for B in batches:
        idx = t._index(B)
        out, aux, tags[f'{block}:{B}'] = t.call_span(m, block, block, faces[idx])
        t._assert_equal(out, refs[0][idx], f'block {block} B={B} launches {tags[f"{block}:{B}"]}')
print('TAGS ' + json.dumps(tags))
'''
_KNOB_FAILED = []


@pytest.mark.parametrize('knobs', [{'lt_glds': 0}, {'lt_glds': 2}, {'lt_stage': 0}, {'lt_stage': 1}], ids=lambda k: ','.join(f'{a}={b}' for a, b in k.items()))
def test_integer_probe_under_the_lt_knobs(knobs):
    """lt_glds = 0: conv_lt_kernel everywhere and no DUAL GEMM; lt_glds = 2: conv_lp_kernel for the 128-pixel tiles too; lt_stage = 0 / 1: the
    row- / plane-shaped staging loads forced on every convolution.  Bit for bit on the integer probe, with the tags the knobs imply.  Once a
    child has failed no further child is started."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    assert not _KNOB_FAILED, f'not started: the child under {_KNOB_FAILED[0]} failed'
    env = dict(os.environ, SYNERGY_HIP_TEST_KNOBS=','.join(f'{k}={v}' for k, v in knobs.items()))
    r = subprocess.run([sys.executable, '-c', KNOB_CHILD, ROOT, os.path.join(ROOT, 'tests')], env=env, capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        _KNOB_FAILED.append(knobs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tags = json.loads([l for l in r.stdout.splitlines() if l.startswith('TAGS ')][-1][5:])
    changed = False
    for block, batches in KNOB_BLOCKS:
        for B in batches:
            want = rc.expected_tags(block, block, B, **knobs)[0]
            assert tags[f'{block}:{B}'] == want, (block, B, tags[f'{block}:{B}'], want)
            changed |= want != rc.expected_tags(block, block, B)[0]
    assert changed                                   # the knob set selects another kernel somewhere in these cases


def _partition(B, fusion, fuse, gemm):
    """the forward's own partition into spans: a cut behind block k only where no fused launch hands conv1 of block k + 1 over"""
    spans, start = [], 0
    for k in range(18):
        if k == 17 or not rc.block_tags(k, B, fusion, fuse, gemm)[1]:
            spans.append((start, k))
            start = k + 1
    return spans


@pytest.mark.parametrize('B', [3, 136, 512])
def test_chained_spans_equal_the_production_forward(handles, B):
    """The spans of the forward's own partition, each output fed to the next, against forward_crops_u8 on the same handle and against the
    single 0..17 call: torch.equal, param and pool, and the same launch tags.  The hook runs the forward's launches, and the conversions
    between the caller's fp32 and the pair format at the cuts lose nothing."""
    import torch
    from synergynet_amd import synth
    m, _ = handles('default', 'gaussian')
    crops = torch.from_numpy(synth.make_crops(rc.N_FACES, seed=933)).cuda()[_index(B)].contiguous()
    want, want_pool = m.forward_crops_u8(crops, return_pool=True)
    want, want_pool = want[:, :62].contiguous(), want_pool.contiguous()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    whole, whole_pool, tags = call_span(m, 0, 17, crops, want_aux=True)
    assert tags == rc.expected_tags(0, 17, B)[0], tags
    assert torch.equal(whole, want) and torch.equal(whole_pool, want_pool)
    spans = _partition(B, 2, 4, 1)
    assert spans[0] == (0, 0) and (1, 7) in spans and spans[-1] == (17, 17), spans
    y, issued = crops, []
    for first, last in spans[:-1]:
        y, _, t = call_span(m, first, last, y)
        issued += t
    got, got_pool, t = call_span(m, 17, 17, y, want_aux=True)
    assert issued + t == tags, (issued + t, tags)
    assert torch.equal(got, want) and torch.equal(got_pool, want_pool)


def test_converters_alone(handles):
    """The two converters of the hook: the pair layout of one [M,64] tensor against the numpy restatement of the header comment of
    csrc/resnet_kernels.hip, and a round trip of values that use all 22 bits (both signs, binades from 2^-3 to 2^15), bitwise."""
    import torch
    m, _ = handles('default', 'integer')
    rng = np.random.default_rng(22)
    M = 37
    mant = rng.integers(2 ** 21, 2 ** 22, size=(M, 64)).astype(np.float64)                     # 22 significant bits, the lowest often set
    x = (mant * 2.0 ** rng.integers(-24, -6, size=(M, 64)) * rng.choice([-1.0, 1.0], size=(M, 64))).astype(np.float32)
    x[0, :8] = [0.0, 1.0, -1.0, 2047.0, 2049.0, -4095.0, 60000.0, 2.0 ** -10]
    hi, lo = rc.f16_pieces(x.astype(np.float64))
    assert np.array_equal(hi + lo, x.astype(np.float64)) and (lo != 0).mean() > 0.9            # the values fit the two pieces and need both
    xd = torch.from_numpy(x).cuda()
    pairs, back = torch.full_like(xd, float('nan')), torch.full_like(xd, float('nan'))
    assert m._lib.syn_debug_resnet_pairs(xd.data_ptr(), pairs.data_ptr(), M, 64, 1, m._stream()) == 0
    assert m._lib.syn_debug_resnet_pairs(pairs.data_ptr(), back.data_ptr(), M, 64, 0, m._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pairs.cpu().numpy().view(np.uint32), rc.pair_layout(x))
    assert np.array_equal(back.cpu().numpy().view(np.uint32), x.view(np.uint32))


def test_hook_refusals_leave_buffers_and_handle_alone(handles, pack):
    """Every refusal of include/synergy_hip.h: SYN_ERR_INVALID with a message that names what was expected, before any launch (the NaN
    outputs stay NaN), and the handle still passes a probe afterwards."""
    import torch
    from synergynet_amd import abi, synth
    from synergynet_amd.synergy3DMM import SynergyNet
    m, _ = handles('default', 'integer')
    lib = m._lib
    faces, refs, _ = _integer_probe(9, 9)                                  # layer3.1: [B,8,8,1024] -> [B,8,8,1024], next conv1 [B,8,8,256]
    n, na = 8 * 8 * 1024, 8 * 8 * 256
    xd = faces[:1].contiguous()
    out = torch.full((n + 64,), float('nan'), device='cuda')
    aux = torch.full((na + 64,), float('nan'), device='cuda')
    tags = (ctypes.c_int * 160)()
    other = SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_mobilenet1_state(1357, 0.5), arch='mobilenet_05')
    cases = [  # (handle, first, last, in_u8, B, n_in, n_out, aux?, n_aux, max_tags, what the message says)
        (m._h, 9, 9, 0, 1, n + 1, n, False, 0, 160, b'n_in='), (m._h, 9, 9, 0, 1, n, n - 1, False, 0, 160, b'n_out='),
        (m._h, 9, 9, 0, 1, n, n + 64, False, 0, 160, b'n_out='), (m._h, 9, 9, 0, 1, n, n, False, na, 160, b'n_aux='),
        (m._h, 9, 9, 0, 1, n, n, True, na + 64, 160, b'n_aux='), (m._h, 9, 9, 0, 1, n, n, True, 0, 160, b'n_aux='),
        (m._h, 17, 17, 0, 1, 16 * 2048, 62, True, 2048 + 64, 160, b'n_aux='),
        (m._h, 9, 9, 0, 2, n, n, False, 0, 160, b'B=2'),                    # counts of one face offered for two
        (other._h, 9, 9, 0, 1, n, n, False, 0, 160, b'mobilenet_05'),
        (m._h, 10, 9, 0, 1, n, n, False, 0, 160, b'first=10'), (m._h, -1, 9, 0, 1, n, n, False, 0, 160, b'first=-1'),
        (m._h, 9, 18, 0, 1, n, n, False, 0, 160, b'last=18'), (m._h, 18, 18, 0, 1, n, n, False, 0, 160, b'first=18'),
        (m._h, 9, 9, 1, 1, n, n, False, 0, 160, b'in_u8'), (m._h, 16, 16, 0, 1, 16 * 2048, 16 * 2048, True, na, 160, b'aux'),
        (m._h, 0, 0, 1, 1, 3 * 120 * 120, 900 * 64, True, na, 160, b'aux'),
        (m._h, 9, 9, 0, 0, 0, 0, False, 0, 160, b'B=0'), (m._h, 9, 9, 0, -1, n, n, False, 0, 160, b'B=-1'), (m._h, 9, 9, 0, 65537, n, n, False, 0, 160, b'B=65537'),
        (m._h, 9, 9, 0, 1, n, n, False, 0, 2, b'max_tags=2'), (m._h, 17, 17, 0, 1, 16 * 2048, 62, False, 0, 0, b'max_tags=0'),
        (m._h, 9, 9, 0, 1, n, n, False, 0, -1, b'max_tags=-1'),
    ]
    for h, first, last, u8, B, ni, no, with_aux, n_aux, mt, word in cases:
        rc_ = lib.syn_resnet50_span(h, first, last, xd.data_ptr(), u8, B, ni, out.data_ptr(), no, aux.data_ptr() if with_aux else None, n_aux, tags, mt,
                                    m._stream())
        err = lib.syn_last_error()
        assert rc_ == abi.SYN_ERR_INVALID, (first, last, u8, B, ni, no, with_aux, n_aux, mt)
        assert b'syn_resnet50_span' in err and b'expected' in err and word in err, err
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(aux).all())
    got, _, t = call_span(m, 9, 9, xd)
    assert t == rc.expected_tags(9, 9, 1)[0]
    _assert_equal(got, refs[0][:1], 'after the refusals')
