"""Test infrastructure of the MobileNetV2 span tests (syn_mobilenet2_span, tests/test_gpu_mobilenet2_spans.py): a float64 restatement of
.features[first] .. [last] written against the state_dict alone (it shares nothing with the library's packing code), an integer probe on
which every kernel of every schedule has to be EXACT, the elementwise bound the gaussian checkpoint is judged with, six wrong variants of a
block restated in numpy (the evidence that the probes bite, tests/test_mobilenet2_cpu.py), and the table of launches the forward is expected
to issue per batch size (written from the launchers' thresholds: csrc/fused_block_rm.hip, fused_block_lb.hip, fused_block_lb4.hip,
fused_block_f16.hip, stem_rm.hip, head_kernel.hip, and run_backbone in csrc/synergy_abi.hip).

Layouts: crops are uint8 HWC [B,120,120,3] or normalised fp32 CHW [B,3,120,120]; every other activation is NHWC, as the library keeps it."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from synergynet_amd import synth

U = 2.0 ** -24                                   # unit roundoff of fp32
V_STAR = np.float32(1) - np.float32(1e-5)        # running_var with fl32(v + 1e-5f) == 1: the folded scale is gamma exactly (asserted on the CPU)
V_STAR64 = np.float64(1) - np.float64(1e-5)      # its float64 counterpart
PROBE_SEED = 20250
N_FACES = 8                                      # distinct faces of a probe batch; slot i holds face (5 i + 3) % 8
LAYERS = synth.mbv2_layers()
HEADS = [n for n, _ in synth.HEADS]
TOL_END = 1e-4                                   # the end-of-network tolerance of tests/test_gpu_parity.py, for the dilution figures only


def _shapes():
    """feature -> (hin, cin, hout, cout) of .features[0..18]"""
    out, h = {}, 120
    for f in range(19):
        ls = [L for L in LAYERS if L['feature'] == f]
        ho = h
        for L in ls:
            if L['stride'] == 2:
                ho = (ho - 1) // 2 + 1
        out[f] = (h, ls[0]['cin'], ho, ls[-1]['cout'])
        h = ho
    return out


SHAPES = _shapes()
RESIDUAL = {f for f in range(19) if any(L['residual'] for L in LAYERS if L['feature'] == f)}
STRIDE2 = {f for f in range(1, 18) if any(L['stride'] == 2 for L in LAYERS if L['feature'] == f)}


def feature_layers(f):
    return [L for L in LAYERS if L['feature'] == f]


def span_counts(first, last, B):
    """(n_in, out shape, pool shape | None) of a span, as syn_mobilenet2_span wants them"""
    n_in = B * (3 * 120 * 120 if first == 0 else SHAPES[first][0] ** 2 * SHAPES[first][1])
    if last == 19:
        return n_in, (B, 62), (B, 1280)
    return n_in, (B, SHAPES[last][2], SHAPES[last][2], SHAPES[last][3]), None


def batch_index(B, n=N_FACES):
    """slot i of a probe batch holds face (5 i + 3) % n: 5 is coprime to 8, so neighbouring slots of a unit, band or pair differ"""
    return (np.arange(B) * 5 + 3) % n


def normalize_u8(crops_u8):
    return ((np.asarray(crops_u8).astype(np.float32) - 127.5) / 128.0).transpose(0, 3, 1, 2).copy()


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def bound_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound; an element whose bound is 0 has to match exactly"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert err.shape == bound.shape and (bound >= 0).all()
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------
def _t(sd, key, dtype=torch.float64):
    v = sd[key]
    v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    return v.to(dtype)


def _fold(sd, L, dtype=torch.float64):
    """(scale, shift) of the layer's eval-mode BatchNorm: scale = gamma / sqrt(var + 1e-5), shift = beta - mean scale"""
    bn = L['bn']
    s = _t(sd, bn + '.weight', dtype) / torch.sqrt(_t(sd, bn + '.running_var', dtype) + 1e-5)
    return s, _t(sd, bn + '.bias', dtype) - _t(sd, bn + '.running_mean', dtype) * s


def _conv(L, a, w):
    if L['kind'] == 'dw':
        return F.conv2d(a, w, None, L['stride'], 1, 1, L['cout'])
    if L['kind'] == 'stem':
        return F.conv2d(a, w, None, 2, 1)
    return F.conv2d(a, w)


def _layer(sd, L, a, dtype=torch.float64):
    s, b = _fold(sd, L, dtype)
    y = _conv(L, a, _t(sd, L['key'] + '.weight', dtype)) * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    return torch.clamp(y, 0.0, 6.0) if L['relu6'] else y


def _nchw(x, dtype=torch.float64):
    return torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# The wrong variants of tests/test_mobilenet2_cpu.py: {'kind': ..., 'feature': f} changes ONE thing in .features[f]
#   'tap'       depthwise tap (0, 0) of channel 0 applied one pixel to the right (its weight moved to tap (0, 1))
#   'tail'      stride-2 block: the last output row of the depthwise taken one input row too high
#   'halo'      the hidden row above the image (a row band's upper halo at the border) = the expand of a zero input row, relu6(shift),
#               instead of the depthwise's padding zeros
#   'kswap'     hidden channels 0 and 1 swapped in front of the project GEMM (two k slots of one group)
#   'nores'     the residual add left out
#   'stempad'   the stem's padding is PIXEL 0, (0 - 127.5) / 128, instead of normalised 0
#   'lowdrop'   the block input of the expand GEMM (or of features.18) without its low fp16 piece: rtz16(x) in place of x
VARIANTS = ('tap', 'tail', 'halo', 'kswap', 'nores', 'stempad', 'lowdrop')      # + 'pixel': True -> the mistake in one pixel of that layer's output only


def _feature(sd, f, a, dtype, variant, trace):
    """one .features[f] on NCHW `a`; trace (a list) receives (layer, input, output) per layer"""
    v = variant['kind'] if variant and variant['feature'] == f else None
    block_in = a
    for L in feature_layers(f):
        x_in = a
        if L['kind'] == 'stem' and v == 'stempad':
            s, b = _fold(sd, L, dtype)
            padded = F.pad(a, (1, 1, 1, 1), value=-127.5 / 128.0)
            a = torch.clamp(F.conv2d(padded, _t(sd, L['key'] + '.weight', dtype), None, 2, 0) * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1), 0.0, 6.0)
        elif L['kind'] == 'dw' and v in ('tap', 'tail', 'halo'):
            s, b = _fold(sd, L, dtype)
            w = _t(sd, L['key'] + '.weight', dtype).clone()
            epi = lambda y: torch.clamp(y * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1), 0.0, 6.0)
            if v == 'tap':
                w[0, 0, 0, 1] += w[0, 0, 0, 0]
                w[0, 0, 0, 0] = 0
                a = epi(_conv(L, a, w))
            elif v == 'tail':
                assert L['stride'] == 2
                good = epi(_conv(L, a, w))
                high = epi(_conv(L, F.pad(a, (0, 0, 1, 0))[:, :, :-1], w))       # every row reads one input row too high
                a = torch.cat([good[:, :, :-1], high[:, :, -1:]], dim=2)
            else:
                E = feature_layers(f)[0]
                assert E['kind'] == 'pw' and E['relu6']
                row = torch.clamp(_fold(sd, E, dtype)[1], 0.0, 6.0).view(1, -1, 1, 1).expand(a.shape[0], -1, 1, a.shape[3])
                padded = F.pad(torch.cat([row, a], dim=2), (1, 1, 0, 1))
                a = epi(F.conv2d(padded, w, None, L['stride'], 0, 1, L['cout']))
        else:
            if L['kind'] == 'pw' and L['relu6'] and v == 'lowdrop':
                a = torch.from_numpy(f16_rtz(a.numpy())).to(dtype)
            if L['kind'] == 'pw' and not L['relu6'] and v == 'kswap':
                a = torch.cat([a[:, 1:2], a[:, 0:1], a[:, 2:]], dim=1)
            a = _layer(sd, L, a, dtype)
            if L['residual'] and v != 'nores':
                a = a + block_in
        if v and variant.get('pixel') and ((L['kind'] == 'stem' and v == 'stempad') or (L['kind'] == 'dw' and v in ('tap', 'tail', 'halo')) or
                                           (L['kind'] == 'pw' and not L['relu6'] and v in ('kswap', 'nores'))):
            # the same mistake in ONE pixel of the layer's output: the first of the map where the upper border is at fault, else the last
            good = _layer(sd, L, x_in, dtype) + (block_in if L['residual'] else 0.0)
            p = 0 if v in ('halo', 'stempad') else good.shape[2] - 1
            good[:, :, p, p] = a[:, :, p, p]
            a = good
        if trace is not None:
            trace.append((L, x_in, a))
    return a


def heads_reference(sd, pool, dtype=torch.float64):
    p = torch.as_tensor(np.asarray(pool)).to(dtype)
    return torch.cat([p @ _t(sd, n + '.weight', dtype).t() + _t(sd, n + '.bias', dtype) for n in HEADS], dim=1).numpy()


def span_reference(sd, first, last, x, dtype=torch.float64, variant=None, trace=None):
    """.features[first] .. [last] from the state_dict.  x: the normalised CHW crops for first = 0, the NHWC block input otherwise.
    Returns the NHWC output of .features[last] as numpy, or (pool [B,1280], param [B,62]) for last = 19."""
    assert 0 <= first <= last <= 19 and first not in (1, 19) and (first, last) != (0, 0)
    with torch.no_grad():
        a = torch.as_tensor(np.asarray(x)).to(dtype) if first == 0 else _nchw(x, dtype)
        for f in range(first, min(last, 18) + 1):
            a = _feature(sd, f, a, dtype, variant, trace)
        if last < 19:
            return _nhwc(a)
        pool = a.mean(dim=(2, 3))
        return pool.numpy(), heads_reference(sd, pool, dtype)


# ---- the elementwise bound ---------------------------------------------------------------------------------------------------------------
# fp32 schedules (SYNERGY_HIP_FUSION = 1, 0), per layer, the form of mobilenet1_cases.layer_bound: a length-n dot product summed in fp32 in
# ANY order, with or without FMA, is within n u sum |a_k||w_k| of the exact one; the fold adds 3 roundings in scale and 2 in shift, the
# epilogue 2, one to spare: (n + 8) u (|s| sum |a||w| + |beta| + |mean s|).
# fp16 x2 schedule (SYNERGY_HIP_FUSION = 2), stem and every 1x1 convolution: each operand x is carried as a = rtz16(x),
# b = rtz16(x - a).  rtz keeps 11 significant bits: for x in [2^e, 2^e+1) a ends at bit e - 10, so |b| <= |x - a| < 2^(e-10) <= 2^-10 |x|;
# the leading bit of x - a is at most e - 11, so b ends at bit e - 21 or below and |r| = |x - a - b| < 2^(e-21) <= 2^-21 |x|.
# The kernels form a1 a2 + a1 b2 + b1 a2 of x1 x2 = (a1 + b1 + r1)(a2 + b2 + r2); what is missing is b1 b2 + r1 x2 + x1 r2 (+ second order):
#   |b1 b2| < 2^-10 |x1| 2^-10 |x2| = 2 x 2^-21 |x1 x2|,  |r1 x2| < 2^-21 |x1 x2|,  |x1 r2| < 2^-21 |x1 x2|   ->   C_SPLIT = 4
# per product, relative, in units of 2^-21 (first order, as the fp32 term; the second-order terms are below 2^-30).  The three partial
# products are exact fp32 numbers and are summed in fp32: the (n + 8) u term with 3 n summands.  The row-marching and register-resident
# kernels carry relu6(x) / 6 (the `clamp` modifier): the rounded constant 1 / (6 S), the multiply by it, shift / 6 and the multiply that
# undoes it are four more roundings of relative size u on quantities the bound already holds: (3 n + 12) u.
# 5.3a, the absolute floor: a low piece below 2^-14 is an fp16 subnormal, spacing 2^-24, so an activation (split at scale 1; scale 16 errs
# less) errs by up to 2^-24 whatever its size -- |s| sum |w| 2^-24 per output -- and a weight (scaled to max |w s| S in [2^13, 2^14)) by up
# to 2^-24 / S <= 2^-37 max |w s| -- sum |a| 2^-37 max |w s| per output.
C_SPLIT = 4.0


def _layer_bound(sd, L, a, f16):
    """(elementwise local bound of the layer on the exact input `a`, |s|, |w|) in float64, NCHW"""
    s, _ = _fold(sd, L)
    bn = L['bn']
    sa = s.abs()
    w = _t(sd, L['key'] + '.weight').abs()
    n = 27 if L['kind'] == 'stem' else 9 if L['kind'] == 'dw' else L['cin']
    mag = _conv(L, a.abs(), w) * sa.view(1, -1, 1, 1)
    const = (_t(sd, bn + '.bias').abs() + _t(sd, bn + '.running_mean').abs() * sa).view(1, -1, 1, 1)
    split = f16 and L['kind'] != 'dw'
    b = ((3 * n if split else n) + (12 if f16 else 8)) * U * (mag + const)
    if split:
        wmax = float((w.flatten(1) * sa.view(-1, 1)).max())
        b = b + C_SPLIT * 2.0 ** -21 * mag + 2.0 ** -24 * _conv(L, torch.ones_like(a), w) * sa.view(1, -1, 1, 1) \
            + 2.0 ** -37 * wmax * _conv(L, a.abs(), torch.ones_like(w))
    return b, sa, w


def heads_bound(sd, pool):
    """(C + 2) u (sum |W||pool| + |b|) of the 62 outputs on a GIVEN pool [B,C] (fp32 on every schedule)"""
    p = torch.as_tensor(np.asarray(pool)).to(torch.float64).abs()
    mag = torch.cat([p @ _t(sd, n + '.weight').abs().t() + _t(sd, n + '.bias').abs() for n in HEADS], dim=1)
    return ((p.shape[1] + 2) * U * mag).numpy()


def span_bound(sd, first, last, x, schedule):
    """Elementwise bound of |got - span_reference(float64)| for the same fp32 input x, schedule 'fp32' or 'f16x2'.  Spans of several layers
    PROPAGATE: the bound of a layer's input is carried through the float64 Jacobian bound |s| sum_k |w_nk| bound_in,k (ReLU6 is 1-Lipschitz,
    the residual adds the block input's bound), and the layer's own bound on the reference's activations is added.  Returns the NHWC bound
    of .features[last], or for last = 19 (bound of the pool, None): the 62 outputs are judged on the pool the library returned
    (heads_reference / heads_bound), which isolates the heads."""
    assert schedule in ('fp32', 'f16x2')
    trace = []
    span_reference(sd, first, last, x, trace=trace)
    with torch.no_grad():
        bnd, block_bnd = None, None
        for L, a, y in trace:
            if L is feature_layers(L['feature'])[0]:
                block_bnd = bnd
            local, sa, w = _layer_bound(sd, L, a, schedule == 'f16x2')
            if bnd is not None:
                local = local + _conv(L, bnd, w) * sa.view(1, -1, 1, 1)
            if L['residual']:
                local = local + (block_bnd if block_bnd is not None else 0.0) + U * y.abs()      # (the add itself rounds once)
            bnd = local
        if last < 19:
            return _nhwc(bnd)
        y = trace[-1][2]
        return (bnd.mean(dim=(2, 3)) + 17 * U * y.abs().mean(dim=(2, 3))).numpy(), None


# ---- fp16 pieces, restated (csrc/synergy_abi.hip f16_rtz / pow2_scale; v_cvt_pkrtz_f16_f32) -------------------------------------------------
def f16_rtz(x):
    """the fp16 number nearest to x toward zero, as float64 (11 significant bits, subnormals spaced 2^-24, saturating at 65504)"""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    _, e = np.frexp(ax)                                          # ax = m 2^e, m in [0.5, 1)
    q = np.maximum(np.ldexp(1.0, e - 11), 2.0 ** -24)
    return np.sign(x) * np.minimum(np.floor(ax / q) * q, 65504.0)


def f16_pieces(x):
    a = f16_rtz(x)
    return a, f16_rtz(np.asarray(x, np.float64) - a)


def pow2_scale(mx):
    """the packers' scale of a layer: max |w s| S in [2^13, 2^14)"""
    _, e = np.frexp(float(mx))
    return 2.0 ** (14 - int(e))


# ---- the integer probe ---------------------------------------------------------------------------------------------------------------------
def integer_faces(first, n=N_FACES, seed=PROBE_SEED):
    """The n distinct faces of the probe input of a span that starts at `first`.  first = 0: uint8 HWC crops over the full 0..255
    ((x - 127.5) / 128 is exact in fp32, 8 fractional bits).  Otherwise integer-valued fp32 in [-4, 4], NHWC: block inputs are linear
    project outputs, so both signs are legitimate; two channels carry 12-bit values (pair_channels).  Every face draws its own values."""
    rng = np.random.default_rng([seed, first, n])
    if first == 0:
        return rng.integers(0, 256, size=(n, 120, 120, 3), dtype=np.uint8)
    hin, cin, _, _ = SHAPES[first]
    x = rng.integers(-4, 5, size=(n, hin, hin, cin)).astype(np.float32)
    k1, k2 = pair_channels(cin)                   # the 12-bit pair: a common large value per pixel plus the channel's own small integer
    big = rng.integers(BIG_LO, BIG_HI, size=(n, hin, hin)).astype(np.float32)
    x[..., k1] += big
    x[..., k2] += big
    return x


# The pair channels.  Small integers fit ONE fp16 piece, so a probe made of them alone never runs the a1 b2 / b1 a2 products of the two-piece
# path.  Two channels of every block input therefore carry values above 2^11 -- 12 significant bits, the low piece is the value's parity
# (x 16 at input scale 16) -- and every expand row (and features.18 row) takes the two with OPPOSITE weights or not at all, so that the
# large parts cancel and the pre-activation stays near [0, 6], where a lost or mis-slotted low piece (+-1 in x, +-3 in the pre-activation)
# is not hidden by the clamp.  Inside a span the pair is kept alive by the projects: a block without residual gives both channels the odd
# bias BIG_BIAS, a residual block hands the block input's large part on; the two project rows differ in two entries only, so the
# difference of the pair stays a small integer.  16 x the largest value stays below 65504 (input scale 16), the range verdict at "fp16 x2".
BIG_LO, BIG_HI, BIG_BIAS = 2304, 3300, 2561


def pair_channels(c):
    return 2, c - 3


def integer_input(first, B, n_distinct=N_FACES):
    return integer_faces(first, n_distinct)[batch_index(B, n_distinct)]


_INT_STATE = {}


def make_integer_state(seed=PROBE_SEED):
    """A mobilenet_v2 state_dict on which every layer is exact in fp32 AND on the two-piece fp16 path, on integer_input, whatever the order
    of summation.  running_mean 0, running_var V_STAR (the folded scale is then gamma itself), gamma a power of two from {1, 2, -1} (ReLU6
    layers) or {1, -1} (linear projects), integer BN and head biases.  Convolution weights are small integers:
      * stem (+-3), depthwise, features.1's project (+-1) and the heads ({-2, -1, 1, 2}): dense (no zero: a zero weight hides its term);
      * expand convolutions (+-3) and features.18 (+-1): eight non-zeros per output row, every input channel used;
      * projects of features.2-17: every hidden channel feeds ceil(16 cout / K) rows (+-1, one in five +-2), about 16 non-zeros per row.
    MULTIPLES OF 3: the row-marching and register-resident kernels (stem_rm.hip, fused_block_rm.hip, fused_block_lb.hip, fused_block_lb4.hip)
    carry a hidden activation as relu6(x) / 6 in [0, 1], what the `clamp` output modifier leaves, and 1 / 6 is no fp32 number.  With stem and
    expand weights +-3 and the biases of the ReLU6 layers (and of features.1's project, which stem_rm.hip also divides by 6) multiples of 3,
    every hidden activation of features.0-17 is a multiple of 3 x 2^-q -- {0, 3, 6} in the blocks -- so x / 6 is a short binary fraction,
    and (3 k) x fl(1 / 6) rounds to k / 2 exactly (fl(1 / 6) = (1 / 6)(1 + 2^-25): below half an ulp of k / 2; asserted on the CPU).
    The sparse rows are what keeps the probe INSIDE the network's own operating range: with dense rows a project output would reach
    6 x 960 x 2, the load-time range verdict (analyze_mbv2_ranges) would take the blocks off the fp16 x2 kernels the probe is there to
    judge, and the next expand would see nothing but saturated inputs.  Every row differs from every other, so two swapped k slots still
    change the result.  The integer bias of a ReLU6 channel centres its median on 3 over two canonical faces -- integer_faces(f, 1) and the
    face the previous blocks hand on from integer_faces(0, 1) -- so that a channel holds 0, 6 and values in between both when a block is
    probed alone and inside a chain; projects get a bias from [-3, 3].  Two channels of every block input carry 12-bit values: see
    pair_channels."""
    if seed in _INT_STATE:
        return _INT_STATE[seed]
    rng = np.random.default_rng([seed, 2])
    f64 = torch.float64
    sd = {}

    def put_bn(L, gammas):
        c = L['cout']
        sd[L['bn'] + '.weight'] = rng.choice(np.array(gammas, np.float32), size=c)
        sd[L['bn'] + '.running_mean'] = np.zeros(c, np.float32)
        sd[L['bn'] + '.running_var'] = np.full(c, V_STAR, np.float32)
        sd[L['bn'] + '.num_batches_tracked'] = np.array(1000, dtype=np.int64)
        sd[L['bn'] + '.bias'] = np.zeros(c, np.float32)

    def weights(L):
        cin, cout = L['cin'], L['cout']
        if L['kind'] == 'stem':
            return rng.choice(np.array([-3, 3], np.float32), size=(cout, cin, 3, 3))
        if L['kind'] == 'dw':
            return rng.choice(np.array([-2, -1, 1, 2], np.float32), size=(cout, 1, 3, 3), p=[0.1, 0.4, 0.4, 0.1])
        w = np.zeros((cout, cin), np.float32)
        if L['feature'] == 1:
            w[:] = rng.choice(np.array([-1, 1], np.float32), size=w.shape)
        elif L['relu6']:                                  # expand (+-3) / features.18 (+-1): eight per row, then every column at least once
            one = 1 if L['feature'] == 18 else 3
            for r in range(cout):
                w[r, rng.choice(cin, 8, replace=False)] = rng.choice(np.array([-one, one], np.float32), size=8)
            for k in np.flatnonzero(~w.any(axis=0)):
                w[rng.integers(cout), k] = one
            k1, k2 = pair_channels(cin)                   # the pair: opposite weights in half of the rows, absent from the others
            sign = rng.choice(np.array([-one, 0, 0, one], np.float32), size=cout)
            w[:, k1], w[:, k2] = sign, -sign
            for r in np.flatnonzero(~w.any(axis=1)):
                w[r, k1], w[r, k2] = one, -one
        else:                                             # project
            m = -(-16 * cout // cin)
            for k in range(cin):
                w[rng.choice(cout, m, replace=False), k] = rng.choice(np.array([-2, -1, 1, 2], np.float32), size=m, p=[0.1, 0.4, 0.4, 0.1])
            for r in np.flatnonzero(~w.any(axis=1)):
                w[r, rng.integers(cin)] = 1
            p1, p2 = pair_channels(cout)                  # the next block's pair: the same row but for two entries
            w[p2] = w[p1]
            w[p2, rng.choice(np.flatnonzero(w[p1] == 0), 2, replace=False)] = np.array([1, -1], np.float32)
        return w.reshape(cout, cin, 1, 1)

    with torch.no_grad():
        chain = torch.from_numpy(normalize_u8(integer_faces(0, 1))).to(f64)          # the face the previous blocks hand on
        for f in range(19):
            own = None if f < 2 else _nchw(integer_faces(f, 1), f64)
            a = chain if own is None else torch.cat([own, chain], dim=0)
            block_in = a
            for L in feature_layers(f):
                sd[L['key'] + '.weight'] = weights(L)
                put_bn(L, [1, 1, 2, -1] if L['relu6'] else [1, -1])
                pre = _layer(sd, dict(L, relu6=False), a)
                if L['relu6']:
                    med = pre.permute(1, 0, 2, 3).reshape(L['cout'], -1).median(dim=1).values.numpy()
                    bias = np.rint(3.0 - med) if f == 18 else 3.0 * np.rint((3.0 - med) / 3.0)
                else:
                    bias = rng.integers(-3, 4, size=L['cout']).astype(np.float64) * (3.0 if f == 1 else 1.0)
                    if f >= 2:
                        p1, p2 = pair_channels(L['cout'])
                        sd[L['bn'] + '.weight'][p2] = sd[L['bn'] + '.weight'][p1]
                        if not L['residual']:
                            bias[p1] = bias[p2] = BIG_BIAS
                sd[L['bn'] + '.bias'] = bias.astype(np.float32)
                a = _layer(sd, L, a)
                if L['residual']:
                    a = a + block_in
            chain = a[-1:]
    for name in HEADS:
        n = dict(synth.HEADS)[name]
        sd[name + '.weight'] = rng.choice(np.array([-2, -1, 1, 2], np.float32), size=(n, 1280))
        sd[name + '.bias'] = rng.integers(-8, 9, size=n).astype(np.float32)
    _INT_STATE[seed] = sd
    return sd


def reference_state(sd):
    """The integer state as the float64 reference has to see it: the library folds in fp32, where V_STAR + 1e-5f rounds to 1; in float64
    the same number plus 1e-5 is 1 - 1.4e-8.  The reference gets the float64 number with the same property and nothing else changes."""
    assert all(np.all(v == V_STAR) for k, v in sd.items() if k.endswith('running_var'))
    return {k: (np.full(v.shape, V_STAR64, np.float64) if k.endswith('running_var') else v) for k, v in sd.items()}


def q_of(feature):
    """every intermediate of .features[feature] on the probe is a multiple of 2^-q: 8 behind the normalised pixels (the stem and
    features.1, which only exist in the span from the crops), 0 elsewhere; the pool is a mean of 16 (q + 4)"""
    return 8 if feature <= 1 else 0


def exactness_violations(sd_ref, first, last, x):
    """The conditions under which the probe is exact on every kernel, checked on the float64 trace of one span; returns a list of
    violations (empty = all hold).  Per layer: the output is a multiple of 2^-q; 2^q (|s| sum |a||w| + |shift|) < 2^24, so every partial
    sum in any order is an fp32 number; for the GEMM layers (stem, 1x1): the folded weight x the packer's scale S is ONE fp16 piece (zero low
    piece, hence b1 b2 = 0 for every product) and every activation that is split fits two fp16 pieces that are zero or normal, at input
    scale 1 and 16, and at more than half of the pixels an operand of every expand layer and of features.18 NEEDS its low piece (pair_channels); the
    output is not constant; a block's two hidden tensors hit 0, the open interval (0, 6) and 6; the hidden tensors of
    features.0-17 are multiples of 3 x 2^-q, so that the kernels that carry relu6(x) / 6 hold them exactly."""
    trace, bad = [], []
    out = span_reference(sd_ref, first, last, x, trace=trace)
    block_in = None
    for L, a, y in trace:
        f, q = L['feature'], q_of(L['feature'])
        name = f"features.{f} {L['key']}"
        if L is feature_layers(f)[0]:
            block_in = a
        s, b = _fold(sd_ref, L)
        w = _t(sd_ref, L['key'] + '.weight')
        if not torch.equal(y * 2.0 ** q, torch.round(y * 2.0 ** q)):
            bad.append(f'{name}: output is no multiple of 2^-{q}')
        mag = float((_conv(L, a.abs(), w.abs()) * s.abs().view(1, -1, 1, 1) + b.abs().view(1, -1, 1, 1)).max())
        if L['residual']:
            mag += float(block_in.abs().max())
        if not mag * 2.0 ** q < 2.0 ** 24:
            bad.append(f'{name}: 2^{q} (sum |a||w||s| + |shift|) = {mag * 2.0 ** q:.4g} >= 2^24')
        if float(y.min()) == float(y.max()):
            bad.append(f'{name}: constant output')
        if L['relu6'] and f <= 17 and not torch.equal(y * 2.0 ** q / 3.0, torch.round(y * 2.0 ** q / 3.0)):
            bad.append(f'{name}: a hidden activation is no multiple of 3 x 2^-{q}')
        if L['relu6'] and 2 <= f <= 17:
            if not (bool((y == 0).any()) and bool((y == 6).any()) and bool(((y > 0) & (y < 6)).any())):
                bad.append(f'{name}: hidden activations miss one of 0, (0, 6), 6')
        if L['kind'] != 'dw':
            ws = (w.flatten(1) * s.view(-1, 1)).numpy()
            for pre in ((1.0 / 128.0, 1.0) if L['kind'] == 'stem' else (1.0,)):      # (the uint8 stem divides its filter by 128)
                S = pow2_scale(np.abs(ws * pre).max())
                hi, lo = f16_pieces(ws * pre * S)
                if np.any(lo != 0) or np.any(hi != ws * pre * S):
                    bad.append(f'{name}: a folded weight x S = {S:g} needs a low fp16 piece')
            act = a.numpy()
            for scale in (1.0, 16.0):
                hi, lo = f16_pieces(act * scale)
                if L['relu6'] and f >= 2 and not float((lo != 0).any(axis=1).mean()) > 0.5:
                    bad.append(f'{name}: fewer than half of the pixels hold an operand that needs its low fp16 piece at input scale {scale:g}')
                ok = (hi + lo == act * scale) & (np.abs(act * scale) <= 65504.0)
                for p in (hi, lo):
                    ok &= (p == 0) | (np.abs(p) >= 2.0 ** -14)
                if not ok.all():
                    bad.append(f'{name}: an activation does not fit two normal fp16 pieces at input scale {scale:g}')
    if last == 19:
        pool, param = out
        wmax = max(float(np.abs(sd_ref[n + '.weight']).max()) for n in HEADS)
        bmax = max(float(np.abs(sd_ref[n + '.bias']).max()) for n in HEADS)
        if not np.array_equal(pool * 16, np.rint(pool * 16)) or not np.array_equal(param * 16, np.rint(param * 16)):
            bad.append('pool / heads: no multiple of 2^-4')
        if not (16 * float(np.abs(pool).max()) * 16 < 2.0 ** 24 and 16 * (1280 * float(np.abs(pool).max()) * wmax + bmax) < 2.0 ** 24):
            bad.append('pool / heads: partial sums reach 2^24')
        if np.ptp(param) == 0 or np.ptp(pool) == 0:
            bad.append('pool / heads: constant output')
    return bad


def range_verdict(sd):
    """(unsafe1 mask, unsafe16 mask, input bound per feature) of the load-time range analysis -- what syn_numerics_report prints -- from
    the device-free packer, so the CPU tests see the verdict the handle will apply"""
    from synergynet_amd.build import LIB
    from synergynet_amd.synergy3DMM import flatten_backbone
    lib = C.CDLL(LIB)
    lib.syn_pack_constants_host_bytes.restype = C.c_size_t
    lib.syn_pack_constants_host_bytes.argtypes = [C.c_int] * 4
    lib.syn_pack_constants_host.argtypes = [C.c_int, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    flat = flatten_backbone(sd)
    n = lib.syn_pack_constants_host_bytes(0, 1, 0, 0)
    buf = np.zeros(n, dtype=np.uint8)
    assert lib.syn_pack_constants_host(0, flat.ctypes.data, flat.size, None, None, None, None, None, None, 0, 0, buf.ctypes.data, n) == 0
    tail = buf[-256:]
    return int(tail.view(np.uint32)[0]), int(tail.view(np.uint32)[1]), tail.view(np.float32)[2:22].copy()


def gaussian_faces(first, bound, n=N_FACES, seed=77):
    """sign-mixed gaussian block inputs scaled to the block input's bound of the range analysis: sigma = bound / 4, clipped at the bound"""
    rng = np.random.default_rng([seed, first, n])
    if first == 0:
        return np.clip(rng.standard_normal((n, 3, 120, 120)) * 0.25, -255.0 / 256.0, 255.0 / 256.0).astype(np.float32)
    hin, cin, _, _ = SHAPES[first]
    return np.clip(rng.standard_normal((n, hin, hin, cin)) * (bound / 4.0), -bound, bound).astype(np.float32)


# ---- the schedule table ----------------------------------------------------------------------------------------------------------------------
# Written from the launchers, not from the library's answers.  SCHEDULES: name -> (SYNERGY_HIP_FUSION, SYNERGY_HIP_EARLY_RM).
SCHEDULES = {'default': (2, 2047), 'tiled': (2, 0), 'fused-fp32': (1, 2047), 'per-layer': (0, 2047)}
CHAIN_MIN, SMALL_CHAIN_MAX = 384, 256            # fused_block_lb.hip kChainMin, kSmallChainMax
LB4_MIN = 576                                    # fused_block_lb4.hip lb4_min_batch()
PAIR_RM_MIN, PAIR34_MAX = 513, 1024              # fused_block_rm.hip launch_fused_pair_rm: B >= 513, features.3 + 4 while (B + 3) / 4 <= 256
PAIR_F16_MAX = 256                               # fused_block_f16.hip launch_fused_pair_f16: one workgroup per face, grid <= B5::SLOTS


def expected_tags(first, last, B, fusion=2, early_rm=2047, lb_chain=3, small_f7=1):
    """The launch codes run_backbone issues for .features[first] .. [last] at batch B (a checkpoint inside the fp16 window; test knobs at
    their defaults but for lb_chain and small_f7, fused_block_lb.hip lb_chain_mode: 3 = features.7-14, 2 = 8-14, 1 = 8-13 from 384 faces;
    up to 256 faces 7-14, or 8-14 with small_f7 = 0): 1 = stem + features.1, f = .features[f] (per layer: once per layer), 100 a + b =
    .features[a] .. [b] in one launch, 19 = pool + heads (with features.18 in front of it on the fused schedules).  A pair or chain is
    only taken when the span reaches its end."""
    stop = -1 if last == 19 else last
    top = min(last, 18)
    if fusion == 0:
        tags = []
        for f in range(first, top + 1):
            tags += [f] * len(feature_layers(f))
        return tags + ([19] if last == 19 else [])
    reaches = lambda end: stop < 0 or stop >= end
    rm_bit = lambda f: (early_rm >> (f - 2 if f <= 4 else f)) & 1
    tags, f = [], first
    while f <= top:
        if f == 0:
            tags.append(1)
            f = 2
            continue
        if fusion >= 2:
            if f in (7, 8) and (early_rm & 128) and (early_rm & 512):
                mode = 0 if lb_chain <= 0 else min(lb_chain, 3) if B >= CHAIN_MIN else \
                    (3 if small_f7 else 2) if ((early_rm & 1024) and B <= SMALL_CHAIN_MAX) else 0
                cf, cl = (7 if mode == 3 else 8), (13 if mode == 1 else 14)
                if mode and f == cf and reaches(cl):
                    tags.append(100 * cf + cl)
                    f = cl + 1
                    continue
            if f == 15 and (early_rm & 256) and (early_rm & 512) and reaches(17) and B >= LB4_MIN:
                tags.append(1517)
                f = 18
                continue
            if f in (3, 5) and reaches(f + 1):
                rm = rm_bit(f) and rm_bit(f + 1) and B >= PAIR_RM_MIN and (f == 5 or B <= PAIR34_MAX)
                f16 = f == 5 and B < 513 and B <= PAIR_F16_MAX
                if rm or f16:
                    tags.append(100 * f + f + 1)
                    f += 2
                    continue
        if f == 18:
            tags.append(18 if stop == 18 else 19)
            return tags
        tags.append(f)
        f += 1
    return tags


# Thresholds of the kernel SELECTION inside a launch code (the code does not tell the row-marching kernel from the tiled one): span key ->
# batch sizes t at which the launch of B = t differs from that of B = t - 1 under the default schedule.  From the launchers:
#   stem_rm.hip kStemBandMin 112, kStemMin2 480, kStemMin4 513 (fp32 crops: no band configuration);
#   fused_block_rm.hip features.2: kBand2Min 40, 352, 513; features.3: kBand3Min 96, 200, 448; features.4: 480, 513; features.5/6: 513, and
#     below it fused_block_f16.hip's persistent grid from 257 workgroups; pairs: 513, and features.3 + 4 only up to 1024;
#   fused_block_lb.hip: hidden-sliced from 32 faces (features.8-11 up to 192 only), the register-resident kernels from kLbMinBatch 768
#     (features.7 runs fused_block_f16.hip's persistent grid from 257 below that); chain 7-14 up to 256 and from 384;
#   fused_block_lb4.hip: hidden-sliced below lb4_min_batch() 576, where the 15-17 chain starts -- S slices of the 30 hidden groups, the fewest
#     of {2, 3, 5, 6, 10, 15, 30} that give 192 workgroups of four faces: 30 up to 48 faces, then 15, 10 (77), 6 (125), 5 (153), 3 (253),
#     2 (381); features.17 deferred to the tail with three or two slices (from 253 faces) below 513;
#   head_kernel.hip: five workgroups per face pair up to 192 faces, the wide tail from 513.
LB4_SLICES = [49, 77, 125, 153, 253, 381]
THRESHOLDS = {
    'stem_u8': [112, 480, 513], 'stem_f32': [480, 513],
    2: [40, 352, 513], 3: [96, 200, 448], 4: [480, 513], 5: [257, 513], 6: [257, 513], 7: [257, 768],
    8: [32, 193, 768], 9: [32, 193, 768], 10: [32, 193, 768], 11: [32, 193, 768], 12: [32, 768], 13: [32, 768], 14: [32, 768],
    15: LB4_SLICES + [576], 16: LB4_SLICES + [576], 17: LB4_SLICES + [576],
    (3, 4): [513, 1025], (5, 6): [257, 513], (7, 14): [257, 384], (8, 14): [257, 384], (8, 13): [257, 384], (15, 17): [576],
    (17, 19): [193, 253, 381, 513, 576], (18, 19): [193, 513],
}
# an odd batch where a unit holds two or four faces, or a workgroup two or four one-face units (a half-empty last unit or workgroup), per span key
ODD = {'stem_u8': [113, 481, 515], 'stem_f32': [481, 515], 2: [41, 353, 515], 3: [97, 201, 449], 4: [481, 515], 5: [515], 6: [515], 7: [769], 8: [33, 769], 9: [33, 769], 10: [33, 769],
       11: [33, 769], 12: [33, 769], 13: [33, 769], 14: [33, 769], 15: [3, 577], 16: [3, 577], 17: [3, 577], (3, 4): [515], (5, 6): [3, 515],
       (7, 14): [3, 385], (8, 14): [3, 385], (8, 13): [3, 385], (15, 17): [3, 577], (17, 19): [3, 577], (18, 19): [3, 515]}
SPANS = [(3, 4), (5, 6), (7, 14), (8, 14), (8, 13), (15, 17), (17, 19), (18, 19)]
BIG = 2307                                       # more faces than resident workgroups x units: features.2 only


def span_key(first, last, in_u8=True):
    if first == 0:
        return 'stem_u8' if in_u8 else 'stem_f32'
    return first if first == last else (first, last)


def probe_batches(key, schedule='default'):
    """The batches of the integer probe for a span key: B = 1, the smallest batch on each side of every threshold, the odd sizes, and BIG
    for features.2.  The fp32 schedules have no batch thresholds in these kernels: {1, 3, 33}.  The tiled schedule (SYNERGY_HIP_EARLY_RM =
    0) keeps fused_block_f16.hip's own thresholds: 192 / 193 (output-channel slices of features.15-17, the head's five workgroups per face
    pair) and 256 / 257 (persistent grids, the features.5 + 6 pair)."""
    if schedule in ('fused-fp32', 'per-layer'):
        return [1, 3, 33]
    if schedule == 'tiled':
        return [1, 3, 192, 193, 256, 257]
    bs = {1}
    for t in THRESHOLDS[key]:
        bs |= {t - 1, t}
    bs |= set(ODD.get(key, []))
    if key == 2:
        bs.add(BIG)
    return sorted(bs)
