"""Test infrastructure of the ResNet-50 span tests (syn_resnet50_span, tests/test_gpu_resnet50_spans.py, tests/test_resnet50_cpu.py): a float64
restatement of blocks first .. last written against the state_dict alone (it shares nothing with the library's packing code), an integer
probe per block on which every kernel of every schedule has to be EXACT, the maxima the run-time range guard has to report for it, and the
table of kernel variants the forward is expected to launch per batch size (written from the launchers' conditions: launch_conv,
launch_conv_f16x2, launch_conv_lt_t, launch_conv_dual, launch_conv_c3f[_ds] in csrc/resnet_kernels.hip and run_resnet50 in
csrc/synergy_abi.hip).

Blocks: 0 = stem + max-pool, 1..16 = the bottlenecks layer1.0 .. layer4.2, 17 = pool + heads.  Layouts: crops are uint8 HWC [B,120,120,3] or
normalised fp32 CHW [B,3,120,120]; every other activation is NHWC fp32, as the hook takes and returns it."""
import numpy as np
import torch
import torch.nn.functional as F

import exact_probe as ep
from exact_probe import N_FACES, V_STAR, batch_index, bound_ratio, reference_state          # noqa: F401  (same meanings, one definition)
from mobilenet2_cases import f16_pieces, pow2_scale, normalize_u8                          # noqa: F401  (the fp16 pieces, restated there)
from synergynet_amd import synth

PROBE_SEED = 50500
F64 = torch.float64
CONVS = synth.resnet50_convs()                   # state_dict order: stem, then conv1, conv2, conv3, (downsample) per bottleneck
HEADS = ['fc_ori', 'fc_shape', 'fc_exp']         # the cat order of the 62 parameters (the module appends fc_tex behind them)
RANGE_LO, RANGE_HI = 2.0 ** -10, 6.0e4           # csrc/syn_internal.h kRangeLo, kRangeHi


def _geometry():
    """BLOCKS[k - 1] of bottleneck k: conv indices c1, c2, c3, ds (None without a downsample branch) and hin, hout, cin, c, cout, stride;
    GEO[ci] = (hin, hout) of convolution ci"""
    blocks, geo, h = [], {0: (120, 60)}, 30
    ci = 1
    while ci < len(CONVS):
        c1, c2, c3 = ci, ci + 1, ci + 2
        ds = ci + 3 if ci + 3 < len(CONVS) and CONVS[ci + 3]['role'] == 'ds' else None
        stride = CONVS[c2]['stride']
        ho = (h + 2 - 3) // stride + 1
        geo[c1], geo[c2], geo[c3] = (h, h), (h, ho), (ho, ho)
        if ds is not None:
            geo[ds] = (h, ho)
        blocks.append(dict(key=CONVS[c1]['block'], c1=c1, c2=c2, c3=c3, ds=ds, hin=h, hout=ho, cin=CONVS[c1]['cin'], c=CONVS[c1]['cout'],
                           cout=CONVS[c3]['cout'], stride=stride))
        ci += 3 if ds is None else 4
        h = ho
    return blocks, geo


BLOCKS, GEO = _geometry()
assert len(BLOCKS) == 16 and len(CONVS) == 53


def span_counts(first, last, B, want_aux=False):
    """(n_in, out shape, aux shape | None) of a span, as syn_resnet50_span wants them"""
    if first == 0:
        n_in = B * 3 * 120 * 120
    elif first == 17:
        n_in = B * 16 * 2048
    else:
        b = BLOCKS[first - 1]
        n_in = B * b['hin'] ** 2 * b['cin']
    if last == 17:
        return n_in, (B, 62), ((B, 2048) if want_aux else None)
    if last == 0:
        return n_in, (B, 30, 30, 64), None
    b = BLOCKS[last - 1]
    aux = (B, b['hout'], b['hout'], BLOCKS[last]['c']) if want_aux and last <= 15 else None
    return n_in, (B, b['hout'], b['hout'], b['cout']), aux


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------
def _nchw(x, dtype=F64):
    return torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def _fold(sd, ci, dtype=F64):
    bn = CONVS[ci]['bn']
    g, b, m, v = (ep.t64(sd, bn + k).to(dtype) for k in ('.weight', '.bias', '.running_mean', '.running_var'))
    s = g / torch.sqrt(v + 1e-5)
    return s, b - m * s


def _conv(sd, ci, a, dtype=F64, w=None, stride=None):
    c = CONVS[ci]
    w = ep.t64(sd, c['key'] + '.weight').to(dtype) if w is None else w
    return F.conv2d(a, w, None, c['stride'] if stride is None else stride, c['k'] // 2)


def _cbn(sd, ci, a, dtype=F64, relu=True, add=None, **kw):
    s, b = _fold(sd, ci, dtype)
    y = _conv(sd, ci, a, dtype, **kw) * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    if add is not None:
        y = y + add
    return torch.relu(y) if relu else y


def heads_reference(sd, pool, dtype=F64):
    p = torch.as_tensor(np.asarray(pool)).to(dtype)
    return torch.cat([p @ ep.t64(sd, n + '.weight').to(dtype).t() + ep.t64(sd, n + '.bias').to(dtype) for n in HEADS], dim=1)


def span_trace(sd, first, last, x, dtype=F64):
    """Every tensor of blocks first .. last, in the order the forward produces them: [(name, guard slot | None, NCHW tensor)].  x: the normalised
    CHW crops for first = 0, the NHWC block input otherwise.  Names: 'maxpool', '<k>.t1' / '.t2' / '.ds' / '.out' of bottleneck k, 'pool',
    'param'; behind the last bottleneck of a span that ends at last <= 15 comes '<last + 1>.t1', the conv1 the fused launch also produces.
    The guard slot (csrc/synergy_abi.hip resnet_stat_used): 0 = the max-pool output, 1 + ci = the output of convolution ci, for the tensors a
    later fp16 x2 convolution splits -- not the downsample branches, not the last block's output."""
    assert 0 <= first <= last <= 17
    tr = []
    with torch.no_grad():
        a = torch.as_tensor(np.asarray(x)).to(dtype) if first == 0 else _nchw(x, dtype)
        if first == 0:
            a = F.max_pool2d(_cbn(sd, 0, a, dtype), 3, 2, 1)
            tr.append(('maxpool', 0, a))
        for k in range(max(first, 1), min(last, 16) + 1):
            b = BLOCKS[k - 1]
            t1 = _cbn(sd, b['c1'], a, dtype)
            t2 = _cbn(sd, b['c2'], t1, dtype)
            tr += [(f'{k}.t1', 1 + b['c1'], t1), (f'{k}.t2', 1 + b['c2'], t2)]
            idn = a
            if b['ds'] is not None:
                idn = _cbn(sd, b['ds'], a, dtype, relu=False)
                tr.append((f'{k}.ds', None, idn))
            a = _cbn(sd, b['c3'], t2, dtype, add=idn)
            tr.append((f'{k}.out', 1 + b['c3'] if k < 16 else None, a))
        if 1 <= last <= 15:
            nb = BLOCKS[last]
            tr.append((f'{last + 1}.t1', 1 + nb['c1'], _cbn(sd, nb['c1'], a, dtype)))
        if last == 17:
            pool = a.mean(dim=(2, 3))
            tr += [('pool', None, pool), ('param', None, heads_reference(sd, pool, dtype))]
    return tr


def span_reference(sd, first, last, x, dtype=F64):
    """(out, aux) as the hook returns them, numpy: last <= 16: the NHWC output of block `last` and (last = 1..15) the NHWC conv1 output of block
    last + 1, else None; last = 17: (param [B,62], pool [B,2048])"""
    tr = {n: t for n, _, t in span_trace(sd, first, last, x, dtype)}
    if last == 17:
        return tr['param'].numpy(), tr['pool'].numpy()
    if last == 0:
        return _nhwc(tr['maxpool']), None
    return _nhwc(tr[f'{last}.out']), (_nhwc(tr[f'{last + 1}.t1']) if last <= 15 else None)


# ---- the integer probe ---------------------------------------------------------------------------------------------------------------------
# Every block gets a fresh small-integer input and weights on which every partial sum of every convolution, in any order and with or without
# FMA, is an fp32 number, so every kernel has to EQUAL the float64 reference.  On top of that the fp16 x2 kernels take every operand as two
# fp16 pieces and drop lo x lo: every weight times its packer scale has to be ONE piece (small integers, gamma a signed power of two), and
# every activation a convolution splits has to fit 22 bits inside the guard's window.  What bounds the probe is therefore the number of BITS
# a tensor needs, and a dense +-1 row of K terms adds log2(3 sqrt(K / 2)) of them per convolution -- 7 for conv1 of layer 4 -- where four
# convolutions in a row (conv1, conv2, conv3 and the next block's conv1, which the fused launch computes from the block output) have 22
# between them.  So the rows are SPARSE: NNZ non-zeros per row from {-2, -1, 1, 2}, every row different, every input channel and every tap
# used (asserted in tests/test_resnet50_cpu.py); rows differ, so two swapped K slots still change the result.
# Small integers fit one fp16 piece and would never run the hi x lo products.  Two channels of every block input, BIG(cin), therefore carry
# a common value in [2048, 4090) per pixel plus their own small integer (12 significant bits: the low piece is the value's parity).  Half of
# the rows of every convolution take the two with OPPOSITE weights in one tap, so the large parts cancel and a lost or mis-slotted low piece
# (+-1) is not hidden behind a large result; the others take neither.  The two rows BIG(cout) take one of them each with weight +1, gamma +1
# and a bias from [-3, 3], so the pair is handed on with its common part: through conv1, conv2 (centre tap), conv3 (+ the identity's own pair)
# and, since the next block's conv1 treats BIG of ITS input the same way, through the fused conv1.
NNZ = {'c1': 8, 'c2': 16, 'c3': 8, 'ds': 8}
GSET = {'c1': (1, -1, 2), 'c2': (1, -1, 2), 'c3': (1, -1), 'ds': (1, -1, 2)}
SMALL_MAX = 3
BIG_LO, BIG_HI = 2048, 4090


def BIG(c):
    return 2, c - 3


def integer_faces(block, n=N_FACES, seed=PROBE_SEED):
    """The n distinct faces of the probe input of `block`.  0: uint8 HWC crops over the full 0..255.  17: integers in [0, 7], NHWC
    [n,4,4,2048].  Bottlenecks: integers in [0, SMALL_MAX], the two channels BIG(cin) in [BIG_LO, BIG_HI); every face draws its own values."""
    rng = np.random.default_rng([seed, block, n])
    if block == 0:
        return rng.integers(0, 256, size=(n, 120, 120, 3), dtype=np.uint8)
    if block == 17:
        return rng.integers(0, 8, size=(n, 4, 4, 2048)).astype(np.float32)
    b = BLOCKS[block - 1]
    x = rng.integers(0, SMALL_MAX + 1, size=(n, b['hin'], b['hin'], b['cin'])).astype(np.float32)
    big = rng.integers(BIG_LO, BIG_HI, size=x.shape[:3]).astype(np.float32)      # a common large value per pixel plus the channel's own small integer
    for ch in BIG(b['cin']):
        x[..., ch] += big
    return x


def probe_input(block, dtype=F64):
    """the reference's view of integer_faces(block): normalised CHW crops for block 0, NHWC otherwise"""
    f = integer_faces(block)
    return normalize_u8(f) if block == 0 else f


def _sparse_rows(rng, cout, cin, k, nnz, big_in, big_out):
    """[cout, cin, k, k]: nnz non-zeros per row from {-2, -1, 1, 2}; every input channel and every tap used.  The two big input channels:
    half of the rows take BOTH, with opposite weights +-1 in one tap (the common large part cancels, the low pieces do not), the others
    neither; row big_out[i] takes big_in[i] alone (centre tap, weight +1) and hands it on."""
    w = np.zeros((cout, cin * k * k), np.float32)
    slots = cin * k * k
    for r in range(cout):
        w[r, rng.choice(slots, nnz, replace=False)] = rng.choice(np.array([-2, -1, 1, 2], np.float32), size=nnz, p=[0.1, 0.4, 0.4, 0.1])
    w = w.reshape(cout, cin, k * k)
    for ch in np.flatnonzero(~w.any(axis=(0, 2))):                 # an unused input channel: one more entry in some row
        w[rng.integers(cout), ch, rng.integers(k * k)] = 1
    w[:, list(big_in), :] = 0
    for r in np.flatnonzero(rng.integers(0, 2, size=cout)):
        tap, sign = rng.integers(k * k), rng.choice(np.array([-1, 1], np.float32))
        w[r, big_in[0], tap], w[r, big_in[1], tap] = sign, -sign
    for i, r in enumerate(big_out):
        w[r, list(big_in), :] = 0
        w[r, big_in[i], (k * k) // 2] = 1
    assert w.any(axis=(0, 1)).all() and w.any(axis=(0, 2)).all() and w.any(axis=(1, 2)).all()
    return w.reshape(cout, cin, k, k)


_INT_STATE = {}


def make_integer_state(seed=PROBE_SEED):
    """The resnet50 state_dict of the probe (see above): running_mean 0, running_var V_STAR (the packer's fold gamma * (1 / sqrtf(var + 1e-5f))
    is then gamma itself), gamma a signed power of two from GSET, integer biases by exact_probe.relu_bias on the block's own probe input with
    every channel clamped by 30 .. 70 % and no channel dead on any face (conv3's on conv3 + identity), from [-3, 3] on the downsample branch
    and on the rows that carry the big channels.  Stem: dense weights from {-3 .. 3} without 0, gamma from {1, -1, 2}.  Heads: dense weights
    {-2, -1, 1, 2}, integer biases in [-8, 8]."""
    if seed in _INT_STATE:
        return _INT_STATE[seed]
    rng = np.random.default_rng([seed, 1])
    sd = {}

    def put(ci, w, gset, a, relu=True, add=None, big_out=()):
        c = CONVS[ci]
        cout = c['cout']
        g = rng.choice(np.asarray(gset, np.float32), size=cout)
        g[list(big_out)] = 1
        sd[c['key'] + '.weight'] = w
        sd[c['bn'] + '.weight'] = g
        sd[c['bn'] + '.running_mean'] = np.zeros(cout, np.float32)
        sd[c['bn'] + '.running_var'] = np.full(cout, V_STAR, np.float32)
        sd[c['bn'] + '.num_batches_tracked'] = np.array(1000, dtype=np.int64)
        pre = F.conv2d(a, torch.from_numpy(w).to(F64), None, c['stride'], c['k'] // 2) * torch.from_numpy(g).to(F64).view(1, -1, 1, 1)
        if add is not None:
            pre = pre + add
        bias = ep.relu_bias(rng, pre, clamp_all=True) if relu else rng.integers(-3, 4, size=cout).astype(np.float64)
        bias[list(big_out)] = rng.integers(-3, 4, size=len(big_out))
        sd[c['bn'] + '.bias'] = bias.astype(np.float32)
        y = pre + torch.from_numpy(bias).view(1, -1, 1, 1)
        return torch.relu(y) if relu else y

    with torch.no_grad():
        x0 = torch.from_numpy(probe_input(0)).to(F64)
        put(0, rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), size=(64, 3, 7, 7)), (1, -1, 2), x0)
        for k, b in enumerate(BLOCKS, start=1):
            x = _nchw(integer_faces(k))
            cin, c, cout = b['cin'], b['c'], b['cout']
            t1 = put(b['c1'], _sparse_rows(rng, c, cin, 1, NNZ['c1'], BIG(cin), BIG(c)), GSET['c1'], x, big_out=BIG(c))
            t2 = put(b['c2'], _sparse_rows(rng, c, c, 3, NNZ['c2'], BIG(c), BIG(c)), GSET['c2'], t1, big_out=BIG(c))
            idn = x
            if b['ds'] is not None:
                idn = put(b['ds'], _sparse_rows(rng, cout, cin, 1, NNZ['ds'], BIG(cin), ()), GSET['ds'], x, relu=False)
            put(b['c3'], _sparse_rows(rng, cout, c, 1, NNZ['c3'], BIG(c), BIG(cout)), GSET['c3'], t2, add=idn, big_out=BIG(cout))
    for name, n in synth.RESNET_HEADS:
        sd[name + '.weight'] = rng.choice(np.array([-2, -1, 1, 2], np.float32), size=(n, 2048))
        sd[name + '.bias'] = rng.integers(-8, 9, size=n).astype(np.float32)
    _INT_STATE[seed] = sd
    return sd


def _ulp_bits(t):
    """(q, bits): the tensor is a multiple of 2^-q (smallest such q >= 0, None if none up to 30) and its largest element needs `bits`
    significant bits at that quantum"""
    t = np.abs(np.asarray(t, np.float64))
    for q in range(31):
        s = t * 2.0 ** q
        if np.array_equal(s, np.rint(s)):
            return q, int(np.ceil(np.log2(max(float(s.max()), 1.0) + 1.0)))
    return None, None


def needs_low_piece(t):
    """per channel of an NCHW tensor: some element has a non-zero low fp16 piece"""
    _, lo = f16_pieces(np.asarray(t, np.float64))
    return (lo != 0).any(axis=(0, 2, 3))


def exactness_violations(sd_ref, first, last, x, f16=True):
    """The conditions under which the probe is exact on every kernel, checked on the float64 trace of one span; returns a list of violations
    (empty = all hold).  Per convolution: 2^q (|s| sum |a||w| + |shift| + |identity|) < 2^24 with 2^-q the quantum of its output, so every
    partial sum in any order is an fp32 number; the folded weight x the packer's scale S is ONE fp16 piece (also the rows of the DUAL matrix
    w x scale, conv3 | downsample under one S, and the stem's w x scale / 128).  Per tensor a later convolution splits (those with a guard
    slot): max |x| inside [RANGE_LO, RANGE_HI], at most 22 significant bits, both pieces zero or normal (>= 2^-14), hi + lo == x, and at
    least two channels NEED the low piece.  Pool and heads: multiples of 2^-4 (2^-12 behind the stem) below 2^24."""
    bad = []
    tr = span_trace(sd_ref, first, last, x)
    by = {n: t for n, _, t in tr}

    def one_piece(name, ws):
        S = pow2_scale(np.abs(ws).max())
        hi, lo = f16_pieces(ws * S)
        if np.any(lo != 0) or np.any(hi != ws * S):
            bad.append(f'{name}: a folded weight x S = {S:g} needs a low fp16 piece')

    def conv_check(name, ci, a, y, add=None):
        s, sh = _fold(sd_ref, ci)
        w = ep.t64(sd_ref, CONVS[ci]['key'] + '.weight')
        q, _ = _ulp_bits(y)
        mag = _conv(sd_ref, ci, a.abs(), w=w.abs()) * s.abs().view(1, -1, 1, 1) + sh.abs().view(1, -1, 1, 1)
        if add is not None:
            mag = mag + add.abs()
        if q is None or not float(mag.max()) * 2.0 ** q < 2.0 ** 24:
            bad.append(f'{name}: quantum 2^-{q}, 2^q (sum |a||w||s| + |shift|) = {float(mag.max()) * 2.0 ** (q or 0):.4g} >= 2^24')
        if float(y.min()) == float(y.max()):
            bad.append(f'{name}: constant output')
        ws = w.flatten(1).numpy()
        one_piece(name, ws)
        if ci == 0:
            one_piece(name + ' (uint8 stem)', ws * s.view(-1, 1).numpy() / 128.0)
        return ws * s.view(-1, 1).numpy()

    a = torch.as_tensor(np.asarray(x)).to(F64) if first == 0 else _nchw(x)
    if first == 0:
        conv_check('stem', 0, a, torch.relu(_cbn(sd_ref, 0, a, relu=False)))
        a = by['maxpool']
    for k in range(max(first, 1), min(last, 16) + 1):
        b = BLOCKS[k - 1]
        conv_check(f'{k}.conv1', b['c1'], a, by[f'{k}.t1'])
        conv_check(f'{k}.conv2', b['c2'], by[f'{k}.t1'], by[f'{k}.t2'])
        idn = a
        if b['ds'] is not None:
            idn = by[f'{k}.ds']
            wd = conv_check(f'{k}.downsample', b['ds'], a, idn)
        w3 = conv_check(f'{k}.conv3', b['c3'], by[f'{k}.t2'], by[f'{k}.out'], add=idn)
        if b['ds'] is not None and b['stride'] == 2:
            one_piece(f'{k} DUAL matrix', np.concatenate([w3, wd], axis=1))
        a = by[f'{k}.out']
    if 1 <= last <= 15:
        conv_check(f'{last + 1}.conv1 (fused)', BLOCKS[last]['c1'], a, by[f'{last + 1}.t1'])
    if f16:
        split = [(n, t) for n, slot, t in tr if slot is not None]
        if first >= 1 and first <= 16:
            split.insert(0, (f'{first}.in', _nchw(x)))
        for name, t in split:
            v = t.numpy()
            q, bits = _ulp_bits(v)
            hi, lo = f16_pieces(v)
            mx = float(np.abs(v).max())
            if not RANGE_LO <= mx <= RANGE_HI:
                bad.append(f'{name}: max |x| = {mx:g} outside the guard window')
            if q is None or bits > 22:
                bad.append(f'{name}: needs {bits} significant bits at quantum 2^-{q}')
            ok = (hi + lo == v)
            for p in (hi, lo):
                ok &= (p == 0) | (np.abs(p) >= 2.0 ** -14)
            if not ok.all():
                bad.append(f'{name}: an activation does not fit two normal fp16 pieces')
            if int(needs_low_piece(v).sum()) < 2:
                bad.append(f'{name}: fewer than two channels need the low fp16 piece')
    if last == 17:
        pool, param = by['pool'].numpy(), by['param'].numpy()
        q = 12 if first == 0 else 4
        wmax = max(float(np.abs(sd_ref[n + '.weight']).max()) for n in HEADS)
        bmax = max(float(np.abs(sd_ref[n + '.bias']).max()) for n in HEADS)
        if not np.array_equal(pool * 2.0 ** q, np.rint(pool * 2.0 ** q)):
            bad.append(f'pool: no multiple of 2^-{q}')
        feat = float((by['16.out'] if '16.out' in by else _nchw(x)).abs().max())
        if not (2.0 ** q * 16 * feat < 2.0 ** 24 and 2.0 ** q * (float(np.abs(pool).sum(axis=1).max()) * wmax + bmax) < 2.0 ** 24):
            bad.append('pool / heads: partial sums reach 2^24')
        if np.ptp(param) == 0 or np.ptp(pool) == 0:
            bad.append('pool / heads: constant output')
    return bad


def relu_shares(sd_ref, block):
    """{tensor name: per-channel share of clamped elements [C]} of the ReLU outputs of a block's own probe, and per name whether some channel is
    dead on one of the faces"""
    out = {}
    for name, _, t in span_trace(sd_ref, block, block, probe_input(block)):
        if name.endswith(('.t1', '.t2', '.out')) and name.split('.')[0] == str(block):
            out[name] = ((t == 0).double().mean(dim=(0, 2, 3)).numpy(), bool((t.amax(dim=(2, 3)) <= 0).any()))
    return out


def pair_layout(x):
    """The pair format of an fp32 tensor [M,C] (C % 32 == 0) as uint32 dwords [M,C], restated from the header comment of
    csrc/resnet_kernels.hip: per pixel and 32-channel chunk 128 bytes = the 32 high halves (16 dwords, channel 2 d in the low half of dword
    d, channel 2 d + 1 in the high half) and then the 32 low halves; hi = rtz_f16(x), lo = rtz_f16(x - hi)."""
    x = np.asarray(x, np.float32)
    M, C = x.shape
    hi, lo = f16_pieces(x.astype(np.float64))
    out = np.zeros((M, C // 32, 2, 16), np.uint32)
    for p, piece in enumerate((hi, lo)):
        h = piece.astype(np.float16).view(np.uint16).astype(np.uint32).reshape(M, C // 32, 16, 2)
        out[:, :, p, :] = h[..., 0] | (h[..., 1] << 16)
    return out.reshape(M, C)


def guard_maxima(sd_ref, first, last, x):
    """[(name, guard slot, max |t| per distinct face [N_FACES])] of the guarded tensors of a span's float64 trace"""
    return [(name, slot, t.abs().flatten(1).amax(dim=1).numpy()) for name, slot, t in span_trace(sd_ref, first, last, x) if slot is not None]


def guard_expected(maxima, last, idx, fused_ran):
    """The 54 maxima syn_backbone_range_status has to return after a span on the batch of faces `idx` of an fp16 x2 handle with the guard
    armed: max |t| over the batch for every guarded tensor the span produced (the next block's conv1 only where the fused launch ran), 1
    everywhere else"""
    want = np.ones(54, np.float32)
    faces = np.unique(np.asarray(idx))
    for name, slot, per_face in maxima:
        if 1 <= last <= 15 and name == f'{last + 1}.t1' and not fused_ran:
            continue
        want[slot] = np.float32(per_face[faces].max())
    return want


# ---- the elementwise bound of the gaussian checkpoint ------------------------------------------------------------------------------------------
# Every rule takes and returns (exact float64 activation, elementwise bound of |device - exact|), NCHW.  fp32 handles (SYNERGY_HIP_FUSION=1,
# conv_kernel throughout, the direct stem): exact_probe.conv_bn_pair as it stands, (n + 8) u (|s| sum |a||w| + |beta| + |mean s|) + |s| sum |w| e_in.
# fp16 x2 handles, per convolution (the derivation of mobilenet2_cases._layer_bound in this file's conventions):
#   * every operand is carried as hi = rtz16(x), lo = rtz16(x - hi); hi ends at bit e - 10 of x in [2^e, 2^e+1), lo at bit e - 21 or below, so
#     |x - hi - lo| < 2^(e-21) <= 2^-21 |x| and |lo| < 2^-10 |x|.  The kernels form hi hi + hi lo + lo hi; missing from x1 x2 are lo lo
#     (< 2^-20 |x1 x2| = 2 x 2^-21) and the two remainders (2^-21 each): C_SPLIT = 4, in units of 2^-21 |x1 x2|.  (An fp32 number has 24 bits, so
#     the remainder is at most bits e - 22 and e - 23: 1.5 x 2^-22 |x|; 2^-21 covers it, 2^-22 would not.)
#   * the three partial products are fp32 numbers and are summed in fp32 in any order: 3 n summands; the BN scale is applied in the epilogue
#     (scale x 1/S, S a power of two: exact), the fold rounds 3 times in scale and 2 in shift, the epilogue 2, one to spare: (3 n + 8) u.
#   * floors: a low piece below 2^-14 is an fp16 subnormal, spacing 2^-24.  Activations are split at scale 1: 2^-24 |s| sum |w| per output.
#     Weights are scaled to max |w| S in [2^13, 2^14), WITHOUT the BN scale: 2^-24 / S <= 2^-37 max |w|, so 2^-37 max |w| |s| sum |a| per output.
#   * DUAL (conv3 + stride-2 downsample branch as one GEMM): the BN scales are folded into the rows (one more rounding per weight: 4), the
#     epilogue multiplies by `ones`, the shift is the sum of the two folded shifts (2 + 2 roundings and the add: each part off by at most 3 u
#     of the sum of the absolute parts): 3 (n3 + nd) summands + 4 + 3 + 2 epilogue + 1 to spare = (3 n + 10) u on the sum of the magnitudes;
#     split terms and floors as above with the folded rows (max |w s| over the combined matrix); the add of the identity does not round.
#   * a tensor that travels in the pair format is read as hi + lo by whoever does not feed it to a matrix instruction -- the identity of a
#     bottleneck, and the hook on its way out (out, and aux behind a fused launch): 2^-21 |x| + 2^-24.  On the way in the hook splits the
#     caller's fp32 block input; conv1's share of that is inside C_SPLIT, the identity's is this term.
#   * the fused conv1 consumes the split block output: the conv rule on (block output, its bound).
#   * the matrix-pipe stem (uint8 crops, 128 faces and more) takes the RAW bytes as exact fp16 numbers against the filter w s / 128 in two
#     pieces: 2 x 154 summands (22 K slots per kernel row, padding 127.5), 4 roundings in the folded weight, 3 in the shift (beta - mean s in
#     fp32, the sum in double, the cast), 1 in the epilogue, 1 to spare: (2 x 154 + 9) u on sum p |w s| / 128 + |beta| + |mean s| + 255 / 256
#     sum |w s| -- the raw sum and the folded shift cancel, and both round before they do -- plus the weight's remainder 2^-21 sum p |w s| / 128
#     and its floor 2^-37 max |w s / 128| sum p.  The max-pool takes the largest bound of its window.
U = ep.U
C_SPLIT = 4.0
PAIR_READ = 2.0 ** -21


def _pair_read(y, e):
    """a pair-format tensor read back as hi + lo"""
    return e + PAIR_READ * y.abs() + 2.0 ** -24


def _parts(sd, ci, a):
    """(y, |s| sum |a||w|, |beta| + |mean s|, |s| sum |w| (a map), |s| max |w| sum |a|, w abs, s abs) of one convolution on the exact input a"""
    c = CONVS[ci]
    w = ep.t64(sd, c['key'] + '.weight')
    s, shift, shift_abs = ep.fold64(sd, c['bn'])
    sv = s.abs().view(1, -1, 1, 1)
    conv = lambda t, ww: F.conv2d(t, ww, None, c['stride'], c['k'] // 2)
    y = conv(a, w) * s.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    return y, conv(a.abs(), w.abs()) * sv, shift_abs.view(1, -1, 1, 1), conv(torch.ones_like(a), w.abs()) * sv, \
        conv(a.abs(), torch.ones_like(w)) * sv * float(w.abs().max()), conv, w.abs(), sv


def conv_pair(sd, ci, a, e, f16):
    """conv + folded BN, no activation: (y, bound)"""
    c = CONVS[ci]
    if not f16:
        return ep.conv_bn_pair(sd, c['key'], c['bn'], a, e, c['stride'], c['k'] // 2, 1)
    y, mag, const, wsum, asum, conv, wabs, sv = _parts(sd, ci, a)
    n = c['cin'] * c['k'] ** 2
    b = (3 * n + 8) * U * (mag + const) + C_SPLIT * 2.0 ** -21 * mag + 2.0 ** -24 * wsum + 2.0 ** -37 * asum
    if e is not None:
        b = b + conv(e, wabs) * sv
    return y, b


def dual_pair(sd, c3, ds, t2, e2, x, ex):
    """conv3 + stride-2 downsample branch as one GEMM with folded rows: (bn3(conv3) + bn_d(conv_d), bound)"""
    y3, mag3, const3, wsum3, _, conv3, wabs3, sv3 = _parts(sd, c3, t2)
    yd, magd, constd, wsumd, _, convd, wabsd, svd = _parts(sd, ds, x)
    n = CONVS[c3]['cin'] + CONVS[ds]['cin']
    wmax = max(float((wabs3.flatten(1) * sv3.view(-1, 1)).max()), float((wabsd.flatten(1) * svd.view(-1, 1)).max()))
    asum = conv3(t2.abs(), torch.ones_like(wabs3)) + convd(x.abs(), torch.ones_like(wabsd))
    b = (3 * n + 10) * U * (mag3 + magd + const3 + constd) + C_SPLIT * 2.0 ** -21 * (mag3 + magd) + 2.0 ** -24 * (wsum3 + wsumd) + 2.0 ** -37 * wmax * asum
    b = b + conv3(e2, wabs3) * sv3 + (convd(ex, wabsd) * svd if ex is not None else 0.0)
    return y3 + yd, b


def stem_pair(sd, x, mfma):
    """conv1 + bn1 + ReLU + max-pool on the normalised crops x [B,3,120,120]: (y, bound); mfma: the matrix-pipe stem on the raw bytes"""
    if not mfma:
        y, b = ep.conv_bn_pair(sd, 'conv1', 'bn1', x, None, 2, 3, 1)
    else:
        w = ep.t64(sd, 'conv1.weight')
        s, shift, shift_abs = ep.fold64(sd, 'bn1')
        sv = s.abs().view(1, -1, 1, 1)
        raw = F.pad(x * 128.0 + 127.5, (3, 3, 3, 3), value=127.5)                       # the bytes, padding 127.5
        y = F.conv2d(x, w, None, 2, 3) * s.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        mag = F.conv2d(raw, w.abs(), None, 2, 0) * sv / 128.0
        const = (shift_abs + 255.0 / 256.0 * w.abs().sum(dim=(1, 2, 3)) * s.abs()).view(1, -1, 1, 1)
        wmax = float((w.abs().flatten(1) * s.abs().view(-1, 1)).max()) / 128.0
        b = (2 * 154 + 9) * U * (mag + const) + 2.0 ** -21 * mag + 2.0 ** -37 * wmax * F.conv2d(raw, torch.ones_like(w[:1]), None, 2, 0)
    return ep.max_pool_pair(torch.relu(y), b, 3, 2, 1)


def span_bound(sd, first, last, x, fusion=2, fuse=4, gemm=1, B=1, in_u8=True):
    """(out, aux) bounds of |hook result - span_reference(float64)| for the same fp32 input x at batch size B (the batch decides where the
    matrix-pipe stem and the DUAL GEMM run), laid out like span_reference's results; last = 17: (None, bound of the pool) -- the 62 outputs
    are judged on the pool the library returned (heads_reference / heads_bound), which isolates the heads."""
    f16 = fusion >= 2
    with torch.no_grad():
        a = torch.as_tensor(np.asarray(x)).to(F64) if first == 0 else _nchw(x)
        e = None
        if first == 0:
            a, e = stem_pair(sd, a, TAG_STEM not in block_tags(0, B, fusion, fuse, gemm, in_u8=in_u8)[0])
        for k in range(max(first, 1), min(last, 16) + 1):
            b = BLOCKS[k - 1]
            tags = block_tags(k, B, fusion, fuse, gemm)[0]
            t1, e1 = conv_pair(sd, b['c1'], a, e, f16)
            t1 = torch.relu(t1)
            t2, e2 = conv_pair(sd, b['c2'], t1, e1, f16)
            t2 = torch.relu(t2)
            if TAG_DUAL in tags:
                z, ez = dual_pair(sd, b['c3'], b['ds'], t2, e2, a, e)
            else:
                if b['ds'] is not None:
                    idn, ei = conv_pair(sd, b['ds'], a, e, f16)
                else:
                    idn, ei = a, (_pair_read(a, e if e is not None else 0.0) if f16 else e)
                y3, e3 = conv_pair(sd, b['c3'], t2, e2, f16)
                z, ez = ep.add_pair(y3, e3, idn, ei)
            a, e = torch.relu(z), ez
        if last == 17:
            return None, (ep.mean_pair(a, e)[1]).numpy()
        out_pairs = f16 and last < 16
        aux_b = None
        if 1 <= last <= 15:
            _, en = conv_pair(sd, BLOCKS[last]['c1'], a, e, f16)
            y1 = torch.relu(_cbn(sd, BLOCKS[last]['c1'], a))
            aux_b = _nhwc(_pair_read(y1, en) if f16 else en)
        return _nhwc(_pair_read(a, e) if out_pairs else e), aux_b


# ---- wrong variants: the evidence that the probes bite (tests/test_resnet50_cpu.py) ------------------------------------------------------------
#   'lohi'        conv1 without the lo x hi term of its activations: rtz16(x) in place of x
#   'swap8'       two output channels swapped inside a pair-order group of 8 (channels 4 and 5 of the block output)
#   'padtap'      conv2, last output row of the last face: the padding row below the image reads the last image row instead of zeros
#   'dualstride'  the stride-2 downsample branch (DUAL's second K segment) sampled at stride 1
#   'tail'        the ragged tail tile (the last M mod 128 pixels of the batch) left unwritten: zeros
#   'idfp32'      the identity read as fp32 where it is in the pair format
#   'poolshift'   block 0: the max-pool window one pixel down and to the right (rows 2 oy .. 2 oy + 2)
VARIANTS = {'lohi': 2, 'swap8': 2, 'padtap': 2, 'dualstride': 8, 'tail': 2, 'idfp32': 2, 'poolshift': 0}      # kind -> the block it is shown on


def variant_output(sd, kind, x):
    """the NHWC output of block VARIANTS[kind] on x (block 0: the normalised crops) with ONE thing wrong, float64"""
    k = VARIANTS[kind]
    with torch.no_grad():
        if kind == 'poolshift':
            y = _cbn(sd, 0, torch.as_tensor(np.asarray(x)).to(F64))
            return _nhwc(F.max_pool2d(F.pad(y, (0, 1, 0, 1), value=float('-inf')), 3, 2, 0))
        b, a = BLOCKS[k - 1], _nchw(x)
        t1 = _cbn(sd, b['c1'], torch.from_numpy(f16_pieces(a.numpy())[0]) if kind == 'lohi' else a)
        t2 = _cbn(sd, b['c2'], t1)
        if kind == 'padtap':
            assert b['stride'] == 1
            padded = F.pad(t1, (1, 1, 1, 1))
            padded[-1, :, -1, :] = padded[-1, :, -2, :]
            s, sh = _fold(sd, b['c2'])
            wrong = torch.relu(F.conv2d(padded, ep.t64(sd, CONVS[b['c2']]['key'] + '.weight')) * s.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
            t2[-1, :, -1, :] = wrong[-1, :, -1, :]
        idn = a
        if kind == 'dualstride':
            assert b['stride'] == 2
            idn = _cbn(sd, b['ds'], a, relu=False, stride=1)[:, :, :b['hout'], :b['hout']]
        elif b['ds'] is not None:
            idn = _cbn(sd, b['ds'], a, relu=False)
        if kind == 'idfp32':
            nhwc = np.ascontiguousarray(_nhwc(a)).astype(np.float32)
            garbage = pair_layout(nhwc.reshape(-1, nhwc.shape[-1])).view(np.float32).reshape(nhwc.shape)
            idn = _nchw(garbage)
        out = _nhwc(_cbn(sd, b['c3'], t2, add=idn))
        if kind == 'swap8':
            out[..., [4, 5]] = out[..., [5, 4]]
        if kind == 'tail':
            flat = out.reshape(-1, out.shape[-1])
            assert flat.shape[0] % 128
            flat[flat.shape[0] - flat.shape[0] % 128:] = 0
        return out


N_GAUSS = 2                                      # distinct faces of a gaussian batch: slot i holds face (5 i + 3) % 2


def gaussian_inputs(sd, seed=907):
    """block -> the input the gaussian checkpoint's block is judged on: the uint8 crops for block 0, else the fp32 cast of the float64
    reference's previous block output on those crops (each block's reference starts from the fp32 tensor the device is given)"""
    crops = synth.make_crops(N_GAUSS, seed=seed)
    xs, y = {0: crops}, span_reference(sd, 0, 0, normalize_u8(crops))[0].astype(np.float32)
    for k in range(1, 18):
        xs[k] = y
        if k <= 16:
            y = span_reference(sd, k, k, y)[0].astype(np.float32)
    return xs


def variant_batches(block, sched, in_u8=True):
    """one batch (the largest) per distinct list of kernel variants among the probe batches of a block"""
    fusion, fuse, gemm = schedule_args(sched)
    seen, out = set(), []
    for B in probe_batches(block, sched, in_u8):
        t = tuple(block_tags(block, B, fusion, fuse, gemm, in_u8=in_u8)[0])
        if t not in seen:
            seen.add(t)
            out.append(B)
    return out


def heads_bound(sd, pool):
    """(C + 2) u (sum |W||pool| + |b|) of the 62 outputs on a GIVEN pool [B,2048] (fp32 on every schedule)"""
    return ep.heads_pair(sd, HEADS, pool)[1].numpy()


# ---- the table of launches ---------------------------------------------------------------------------------------------------------------------
# Written from the launchers, not from the library's answers.  A tag is 1000 x block + the code of the kernel variant (include/synergy_hip.h).
# SCHEDULES: name -> the environment the handle is created under.
SCHEDULES = {'default': {}, 'nofuse': {'SYNERGY_HIP_RESNET_FUSE': '0'}, 'fuse1': {'SYNERGY_HIP_RESNET_FUSE': '1'}, 'gemm0': {'SYNERGY_HIP_RESNET_GEMM': '0'},
             'gemm2': {'SYNERGY_HIP_RESNET_GEMM': '2'}, 'fp32': {'SYNERGY_HIP_FUSION': '1'}}


def schedule_args(sched):
    """(fusion, fuse, gemm) of a schedule name"""
    e = SCHEDULES[sched]
    return int(e.get('SYNERGY_HIP_FUSION', 2)), int(e.get('SYNERGY_HIP_RESNET_FUSE', 4)), int(e.get('SYNERGY_HIP_RESNET_GEMM', 1))


TAG_STEM, TAG_STEM_MFMA, TAG_STEM_MFMA_POOL, TAG_MAXPOOL, TAG_DUAL, TAG_POOL_FC = 1, 3, 4, 5, 60, 90
GIB2 = 1 << 31


def _cdiv(a, b):
    return -(-a // b)


def conv_code(ci, B, f16, gemm=1, lt_glds=1, lt_stage=-1):
    """launch_conv (fp32 handle: conv_kernel<MT,4> by the number of 256-pixel x 64-channel tiles) / launch_conv_f16x2: the LDS-tiled GEMM
    (conv_lt_kernel / conv_lp_kernel) where N % 128 == 0 and M >= 4096 (every M with SYNERGY_HIP_RESNET_GEMM=2), 256-pixel tiles (MTW 4) for
    more than 16 k32 steps when they still fill 256 workgroups, never with GEMM=2; conv_lp_kernel for MTW 4 (lt_glds >= 1) and for MTW 2
    from 32 steps on (lt_glds = 1) or always (2); plane-shaped staging (frag) for 3x3 unless lt_stage forces it; else conv_h2s_kernel, 32-pixel
    wave tiles from 2048 tiles of 128 x 64; an input of 2 GiB or more: conv_f16x2_kernel."""
    c, (hin, hout) = CONVS[ci], GEO[ci]
    M, N, taps = B * hout * hout, c['cout'], c['k'] ** 2
    if not f16:
        t64 = _cdiv(M, 256) * (N // 64)
        return 10 + (4 if t64 >= 2048 else 2 if t64 >= 512 else 1)
    steps, small = taps * (c['cin'] // 32), B * hin * hin * c['cin'] * 4 < GIB2
    tiles = _cdiv(M, 128) * (N // 64)
    if gemm and N % 128 == 0 and M >= (1 if gemm == 2 else 4096) and steps % 2 == 0 and small:
        mtw4 = gemm != 2 and steps > 16 and _cdiv(M, 256) * (N // 128) >= 256
        frag = taps > 1 if lt_stage < 0 else lt_stage != 0
        lp = lt_glds >= 1 if mtw4 else (lt_glds >= 2 or (lt_glds == 1 and steps >= 32))
        return (50 if lp else 40) + (2 if mtw4 else 0) + int(frag)
    if steps % 2 == 0 and small:
        return 30 + (2 if tiles >= 2048 else 1)
    return 20 + (2 if tiles >= 1024 else 1)


def c3f_possible(k):
    """conv_c3f_kernel ends bottleneck k: the next conv1 has at most 512 input channels (its step-major fragments exist) and (K, N3, N1) is
    one of the instantiated shapes (conv_c3f_supported)"""
    if k >= 16:
        return False
    b, nb = BLOCKS[k - 1], BLOCKS[k]
    K, N3, N1 = b['c'], b['cout'], nb['c']
    return nb['cin'] <= 512 and N3 % 64 == 0 and N3 <= 512 and ((K == 64 and N1 in (64, 128)) or (K == 128 and N1 == 128))


def dual_taken(k, B):
    """launch_conv_dual: conv3 + the stride-2 downsample branch as one GEMM once 256-pixel x 128-channel tiles fill 256 workgroups"""
    b = BLOCKS[k - 1]
    M, N = B * b['hout'] ** 2, b['cout']
    return ((b['c'] + b['cin']) // 32) % 2 == 0 and N % 128 == 0 and _cdiv(M, 256) * (N // 128) >= 256 and \
        B * b['hout'] ** 2 * b['c'] * 4 < GIB2 and B * b['hin'] ** 2 * b['cin'] * 4 < GIB2


def block_tags(k, B, fusion=2, fuse=4, gemm=1, have_t1=False, in_u8=True, lt_glds=1, lt_stage=-1):
    """(codes of block k at batch B, whether its last launch also produced conv1 of block k + 1)"""
    f16 = fusion >= 2
    code = lambda ci: conv_code(ci, B, f16, gemm, lt_glds, lt_stage)
    if k == 0:
        if fusion >= 2 and in_u8 and B >= 128:
            return ([TAG_STEM_MFMA_POOL] if fuse else [TAG_STEM_MFMA, TAG_MAXPOOL]), False
        return [TAG_STEM, TAG_MAXPOOL], False
    if k == 17:
        return [TAG_POOL_FC], False
    b = BLOCKS[k - 1]
    tags = [] if have_t1 else [code(b['c1'])]
    c3f = f16 and fuse >= 1 and c3f_possible(k)
    c2f = c3f and fuse >= 2 and b['c'] in (64, 128) and b['c'] <= (128 if fuse >= 3 else 64) and B * b['hin'] ** 2 * b['c'] * 4 < GIB2
    if not c2f:
        tags.append(code(b['c2']))
    if c3f:
        if b['ds'] is not None and b['stride'] == 1:
            tags.append(100 + 4 + 2 * int(c2f))                                   # layer1.0: the downsample branch inside the kernel
        else:
            if b['ds'] is not None:
                tags.append(code(b['ds']))                                        # layer2.0: a launch of its own, fp32 identity
            shape = 2 if b['c'] == 128 else 1 if BLOCKS[k]['c'] == 128 else 0
            tags.append(100 + 10 * shape + 2 * int(c2f) + int(b['ds'] is None))
        return tags, True
    if f16 and fuse >= 4 and b['ds'] is not None and b['stride'] == 2 and lt_glds >= 1 and gemm == 1 and dual_taken(k, B):
        return tags + [TAG_DUAL], False
    if b['ds'] is not None:
        tags.append(code(b['ds']))
    return tags + [code(b['c3'])], False


def expected_tags(first, last, B, fusion=2, fuse=4, gemm=1, in_u8=True, **knobs):
    """(launch_tags of the span, whether the last launch of a span that ends at last <= 15 produced the next conv1)"""
    tags, have_t1 = [], False
    for k in range(first, last + 1):
        t, have_t1 = block_tags(k, B, fusion, fuse, gemm, have_t1, in_u8, **knobs)
        tags += [1000 * k + c for c in t]
    return tags, have_t1


B_SCAN = 1100                                   # thresholds are looked for up to here (the largest, layer 4's 256-pixel tiles, is 1009)


def thresholds(block, sched, in_u8=True):
    """the batch sizes t <= B_SCAN at which block `block` alone is launched differently from t - 1 under a schedule"""
    fusion, fuse, gemm = schedule_args(sched)
    prev, out = None, []
    for B in range(1, B_SCAN + 1):
        cur = block_tags(block, B, fusion, fuse, gemm, in_u8=in_u8)[0]
        if prev is not None and cur != prev:
            out.append(B)
        prev = cur
    return out


def probe_batches(block, sched, in_u8=True):
    """The batches of the integer probe of one block under a schedule, LARGEST FIRST (the smaller ones then run over a workspace left dirty):
    1, 3, both sides of every threshold, and the smallest odd batch above the last threshold -- every map is 30^2, 15^2, 8^2 or 4^2, so an
    odd batch is ragged against the 64-, 128- and 256-pixel tiles, and 3 is ragged below one tile."""
    ts = thresholds(block, sched, in_u8)
    bs = {1, 3}
    for t in ts:
        bs |= {t - 1, t}
    top = max(ts + [3]) + 1
    bs.add(top if top % 2 else top + 1)
    return sorted(bs, reverse=True)
