"""The MobileNetV1 kernels one layer at a time (syn_mobilenet1_layer: the launches of the forward itself, on activations the test
supplies), every element judged.  tests/test_gpu_mobilenet1.py looks at the end of the network with rel_max < 1e-4, which a wrong tap,
a wrong k slot or a wrong tail pixel of one tile passes; here
  * an integer probe (mobilenet1_cases.make_integer_state / integer_input: every partial sum of every layer is an fp32 number in any
    order of summation -- conditions asserted on the CPU in tests/test_mobilenet1_cpu.py) has to come out EQUAL to the float64 reference;
  * the gaussian checkpoint has to stay within the elementwise fp32 bound of mobilenet1_cases.layer_bound (small integers would also be
    exact on a reduced-precision matrix path; this pins fp32);
  * the layers chained through the hook equal the production forward bit for bit, and the hook refuses what it cannot run."""
import numpy as np
import pytest

import mobilenet1_cases as mc

pytestmark = pytest.mark.gpu
ARCHS = ['mobilenet_1', 'mobilenet_05', 'mobilenet_2']
PAD = 1024                                       # floats of NaN sentinel before and after every output region


@pytest.fixture(scope='module')
def handles(pack):
    """(arch, 'integer' | 'gaussian') -> model, built on first use"""
    import torch
    assert torch.cuda.is_available()
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    made = {}

    def get(arch, kind):
        if (arch, kind) not in made:
            w = mc.WIDTHS[arch]
            sd = mc.make_integer_state(mc.PROBE_SEED, w) if kind == 'integer' else synth.make_mobilenet1_state(mc.SEEDS[w], w)
            made[arch, kind] = (SynergyNet(device='cuda:0', pack=pack, backbone_state=sd, arch=arch), sd)
        return made[arch, kind]
    return get


def _counts(width, layer, B):
    hin, cin, hout, cout = mc.layer_shapes(width)[layer]
    n_in = B * hin * hin * cin
    if layer == 14:
        return n_in, (B, 62), (B, cin)
    return n_in, (B, hout, hout, cout), (B, hout, hout, cin) if layer else None


def call_layer(m, width, layer, fused, x, want_aux=False):
    """Runs one layer through the hook into NaN-filled buffers with NaN sentinels on both sides; asserts the sentinels untouched and the
    regions free of NaN.  x: numpy or device tensor in the layer's layout (uint8 -> in_u8).  Returns (out, aux | None) as device tensors."""
    import torch
    from synergynet_amd import abi
    x = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(m.device).contiguous()
    B = x.shape[0]
    n_in, out_shape, aux_shape = _counts(width, layer, B)
    assert x.numel() == n_in and x.dtype in (torch.uint8, torch.float32)
    bufs = []
    for shape in (out_shape, aux_shape if want_aux else None):
        bufs.append(None if shape is None else torch.full((2 * PAD + int(np.prod(shape)),), float('nan'), dtype=torch.float32, device=m.device))
    out, aux = bufs
    region = lambda b: b[PAD:b.numel() - PAD]
    abi.check(m._lib.syn_mobilenet1_layer(m._h, layer, int(fused), x.data_ptr(), int(x.dtype == torch.uint8), B, n_in,
                                          region(out).data_ptr(), region(out).numel(), region(aux).data_ptr() if aux is not None else None,
                                          region(aux).numel() if aux is not None else 0, m._stream()))
    torch.cuda.synchronize()
    for name, b in (('out', out), ('aux', aux)):
        if b is None:
            continue
        assert bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[-PAD:]).all()), f'layer {layer} B={B} fused={fused}: {name} sentinel overwritten'
        assert not bool(torch.isnan(region(b)).any()), f'layer {layer} B={B} fused={fused}: {name} not fully written'
    return region(out).view(out_shape), (region(aux).view(aux_shape) if aux is not None else None)


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    i = tuple(bad[0])
    return f'{len(bad)} of {got.size} elements differ, first at {i}: got {got[i]!r}, want {want[i]!r}'


def _assert_equal(got, want64, what):
    got, want = got.cpu().numpy(), want64.astype(np.float32)
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f'{what}: {_first_difference(got, want)}'


_PROBE_REF = {}


def _probe(arch, layer, B):
    """(input, float64 reference) of the integer probe, computed once and shared by the two schedules"""
    if (arch, layer, B) not in _PROBE_REF:
        w = mc.WIDTHS[arch]
        x = mc.integer_input(layer, w, B)
        sd = mc.reference_state(mc.make_integer_state(mc.PROBE_SEED, w))
        _PROBE_REF[arch, layer, B] = (x, mc.layer_reference(sd, w, layer, mc.normalize_u8(x) if layer == 0 else x))
    return _PROBE_REF[arch, layer, B]


@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('arch', ARCHS)
def test_integer_probe_matches_bit_for_bit(handles, arch, fused):
    """Every layer 0..14 at every batch of mobilenet1_cases.probe_batches: np.array_equal with the float64 reference cast to fp32 -- the
    layer output, at fused = 0 the depthwise output, the stem from uint8 and from its normalised fp32 form, the pool and the 62 outputs."""
    m, _ = handles(arch, 'integer')
    w = mc.WIDTHS[arch]
    for layer in range(15):
        for B in mc.probe_batches(w, layer):
            x, ref = _probe(arch, layer, B)
            what = f'{arch} layer {layer} B={B} fused={fused}'
            if layer == 0:
                _assert_equal(call_layer(m, w, 0, fused, x)[0], ref, what + ' uint8')
                _assert_equal(call_layer(m, w, 0, fused, mc.normalize_u8(x))[0], ref, what + ' fp32')
            elif layer == 14:
                out, pool = call_layer(m, w, 14, fused, x, want_aux=True)
                _assert_equal(pool, ref[0], what + ' pool')
                _assert_equal(out, ref[1], what + ' param')
            else:
                out, aux = call_layer(m, w, layer, fused, x, want_aux=not fused)
                if not fused:
                    _assert_equal(aux, ref[0], what + ' depthwise')
                _assert_equal(out, ref[1], what)


def _judge(sd, layer, fused, ref, bound, out, aux):
    """[(name, max err / bound)] of one layer's results against the float64 reference `ref` and the bound `bound` of the same fp32 input"""
    out = out.cpu().numpy()
    if layer == 0:
        return [('out', mc.bound_ratio(out, ref, bound))]
    if layer == 14:
        pool = aux.cpu().numpy()
        return [('pool', mc.bound_ratio(pool, ref[0], bound[0])), ('heads', mc.bound_ratio(out, mc.heads_reference(sd, pool), mc.heads_bound(sd, pool)))]
    if fused:
        return [('block', mc.bound_ratio(out, ref[1], bound[1]))]
    dw = aux.cpu().numpy()
    return [('depthwise', mc.bound_ratio(dw, ref[0], bound[0])),
            ('pointwise', mc.bound_ratio(out, mc.pointwise_reference(sd, layer, dw), mc.pointwise_bound(sd, layer, dw)))]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('arch', ARCHS)
def test_gaussian_checkpoint_within_the_fp32_bound(handles, arch, B):
    """The ordinary checkpoint, every layer on two inputs -- the fp32 cast of the float64 reference's previous activation on real crops,
    and a sign-mixed gaussian tensor of the same shape -- on both schedules: |got - ref64| <= (n + 8) u (|s| sum |a||w| + |beta| + |mean s|)
    elementwise (mobilenet1_cases.layer_bound; torch's own fp32 layers reach 0.26 of it).  At fused = 0 the depthwise output is judged
    with the depthwise bound and the layer output against a float64 pointwise of the RETURNED depthwise output, which isolates the two
    kernels; the heads are judged on the returned pool.  Measured on an MI355X: DESIGN 5.13."""
    from synergynet_amd import synth
    m, sd = handles(arch, 'gaussian')
    w = mc.WIDTHS[arch]
    crops = synth.make_crops(B, seed=900 + B)
    rng = np.random.default_rng([77, B, int(w * 10)])
    prev, worst = None, {}
    for layer in range(15):
        chain = mc.normalize_u8(crops) if layer == 0 else prev.astype(np.float32)
        noise = rng.standard_normal(chain.shape).astype(np.float32)
        assert (noise < 0).any() and (noise > 0).any()
        for kind, x in (('chain', chain), ('gauss', noise)):
            ref, bound = mc.layer_reference(sd, w, layer, x), mc.layer_bound(sd, w, layer, x)
            if kind == 'chain':
                prev = ref if layer == 0 else ref[1]
            for fused in (1, 0):
                feed = crops if (layer == 0 and kind == 'chain') else x                  # the chain's stem takes the uint8 crops themselves
                out, aux = call_layer(m, w, layer, fused, feed, want_aux=(layer == 14 or (layer > 0 and not fused)))
                for name, r in _judge(sd, layer, fused, ref, bound, out, aux):
                    worst[layer, fused, name] = max(worst.get((layer, fused, name), 0.0), r)
    for fused in (1, 0):
        print(f'{arch} B={B} fused={fused} max(err / bound): ' +
              ', '.join(f'{l}:{n} {r:.3f}' for (l, f, n), r in sorted(worst.items()) if f == fused))
    bad = {k: r for k, r in worst.items() if not r < 1.0}
    assert not bad, f'{arch} B={B}: (layer, fused, part) -> err / bound {bad}'


@pytest.mark.parametrize('sched', [0, 1])
@pytest.mark.parametrize('arch', ARCHS)
def test_chained_layers_equal_the_production_forward(handles, arch, sched):
    """Layers 0..14 through the hook, each output fed to the next (blocks without aux: the per-layer depthwise output then lives in the
    handle's workspace, as in the forward), against forward_crops_u8 on the same handle under syn_set_schedule: torch.equal."""
    import torch
    from synergynet_amd import synth
    m, _ = handles(arch, 'gaussian')
    w = mc.WIDTHS[arch]
    crops = torch.from_numpy(synth.make_crops(3, seed=933)).cuda()
    prev = m._lib.syn_set_schedule(m._h, sched)
    try:
        want, want_pool = m.forward_crops_u8(crops, return_pool=True)
    finally:
        m._lib.syn_set_schedule(m._h, prev)
    y = crops
    for layer in range(14):
        y, _ = call_layer(m, w, layer, sched, y)
    got, got_pool = call_layer(m, w, 14, sched, y, want_aux=True)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want) and torch.equal(got_pool, want_pool)


def test_hook_refusals_leave_buffers_and_handle_alone(handles):
    """Every refusal of include/synergy_hip.h: SYN_ERR_INVALID with a message that names what was expected, before any launch (the NaN
    output stays NaN), and the handle still runs afterwards."""
    import torch
    from synergynet_amd import abi
    from synergynet_amd.synergy3DMM import SynergyNet
    m, _ = handles('mobilenet_05', 'integer')
    lib, w = m._lib, 0.5
    x, ref = _probe('mobilenet_05', 6, 1)                                  # dw4_2: [1,15,15,128] -> [1,8,8,256], depthwise [1,8,8,128]
    n_in, n_out, n_aux = 15 * 15 * 128, 8 * 8 * 256, 8 * 8 * 128
    xd = torch.from_numpy(x).cuda()
    out = torch.full((n_out + 64,), float('nan'), device='cuda')
    aux = torch.full((n_aux + 64,), float('nan'), device='cuda')
    bare = SynergyNet(device='cuda:0', load_constants=False)               # arch mobilenet_v2
    cases = [  # (handle, layer, fused, in_u8, B, n_in, n_out, aux?, n_aux, what the message says)
        (m._h, 6, 0, 0, 1, n_in + 1, n_out, True, n_aux, b'n_in='), (m._h, 6, 0, 0, 1, n_in, n_out - 1, True, n_aux, b'n_out='),
        (m._h, 6, 0, 0, 1, n_in, n_out + 64, True, n_aux, b'n_out='), (m._h, 6, 0, 0, 1, n_in, n_out, True, n_aux + 64, b'n_aux='),
        (m._h, 6, 0, 0, 1, n_in, n_out, True, 0, b'n_aux='), (m._h, 6, 0, 0, 1, n_in, n_out, False, n_aux, b'n_aux='),
        (m._h, 6, 1, 0, 2, n_in, n_out, False, 0, b'B=2'),                  # counts of one face offered for two
        (bare._h, 6, 0, 0, 1, n_in, n_out, False, 0, b'mobilenet_v2'),
        (m._h, -1, 0, 0, 1, n_in, n_out, False, 0, b'layer=-1'), (m._h, 15, 0, 0, 1, n_in, n_out, False, 0, b'layer=15'),
        (m._h, 6, 0, 0, 0, 0, 0, False, 0, b'B=0'), (m._h, 6, 0, 0, -1, n_in, n_out, False, 0, b'B=-1'), (m._h, 6, 0, 0, 65537, n_in, n_out, False, 0, b'B=65537'),
        (m._h, 6, 1, 0, 1, n_in, n_out, True, n_aux, b'fused=1'), (m._h, 6, 0, 1, 1, n_in, n_out, False, 0, b'in_u8'),
        (m._h, 14, 0, 1, 1, n_in, n_out, False, 0, b'in_u8'), (m._h, 6, 2, 0, 1, n_in, n_out, False, 0, b'fused=2'),
    ]
    for h, layer, fused, u8, B, ni, no, with_aux, na, word in cases:
        rc = lib.syn_mobilenet1_layer(h, layer, fused, xd.data_ptr(), u8, B, ni, out.data_ptr(), no, aux.data_ptr() if with_aux else None, na,
                                      m._stream())
        err = lib.syn_last_error()
        assert rc == abi.SYN_ERR_INVALID, (layer, fused, u8, B, ni, no, with_aux, na)
        assert b'syn_mobilenet1_layer' in err and b'expected' in err and word in err, err
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(aux).all())
    got, dw = call_layer(m, w, 6, 0, x, want_aux=True)
    _assert_equal(dw, ref[0], 'after the refusals: depthwise')
    _assert_equal(got, ref[1], 'after the refusals')
