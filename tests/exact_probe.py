"""What the block-level exact probes of GhostNet, of the BasicBlock ResNets and of ResNeSt-50 share (tests/ghostnet_cases.py,
tests/resnet_basic_cases.py, tests/resnest_cases.py):
the probe batch, the builder of a probe layer, and the propagation of the elementwise fp32 bound through the stages of a block.  The
constants and the two small helpers keep the meaning they have in tests/mobilenet1_cases.py and are imported from there.

The probe: integer weights and inputs, running_mean 0, running_var V_STAR (the library's fp32 fold then gives scale == gamma exactly), gamma a
signed power of two and integer biases make every partial sum of a layer, in any order and with or without FMA, an fp32 number -- so the
kernel has to EQUAL the float64 reference.  The bound: on an ordinary checkpoint every element has to stay within what fp32 arithmetic
allows for ITS operands, carried through the block as a pair (exact activation a, elementwise error bound e), all in float64."""
import numpy as np
import torch
import torch.nn.functional as F

from mobilenet1_cases import U, V_STAR, V_STAR64, bound_ratio, reference_state          # noqa: F401  (same meanings, one definition)

N_FACES = 8                                      # distinct faces of a probe batch
F64 = torch.float64


def batch_index(B, n=N_FACES):
    """slot i of a probe batch holds distinct face (5 i + 3) % n: 5 is coprime to 8, so neighbouring slots always differ, and a batch of
    any size costs the float64 reference of n faces"""
    return (np.arange(B) * 5 + 3) % n


def t64(sd, key):
    v = sd[key]
    v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    return v.to(F64)


def fold64(sd, bn):
    """(scale, shift, |beta| + |mean scale|) of a BatchNorm in float64"""
    g, b, m, v = (t64(sd, bn + k) for k in ('.weight', '.bias', '.running_mean', '.running_var'))
    s = g / torch.sqrt(v + 1e-5)
    return s, b - m * s, b.abs() + (m * s).abs()


# ---- the probe-layer builder ---------------------------------------------------------------------------------------------------------
def probe_conv_bn(rng, sd, conv, bn, shape, a, stride, pad, groups, wset, gset, relu=True, add=None, clamp_all=False):
    """Draws one conv + BN of the probe into sd and returns its output on `a` (NCHW float64: the N_FACES distinct faces).  Weights from wset
    (no zero: a zero weight hides its term), running_mean 0, running_var V_STAR, gamma from gset (signed powers of two), integer bias.
    relu = True: ReLU follows (after `add`, a residual, where given) and the bias keeps it from hiding the probe, by the rule of
    mobilenet1_cases.make_integer_state on all the distinct faces: three channels in four get the smallest integer that lifts the whole
    channel above 0, the fourth the integer that clamps a share of 30 .. 70 % of it, raised until one element of EVERY distinct face is positive
    (a batch of one face must not hold a dead channel either); clamp_all = True: every channel takes the fourth's rule, which keeps the
    outputs, and with them the partial sums of the next stage, about half as large.
    relu = False: a linear stage (a downsample), integer bias from [-3, 3]."""
    cout = shape[0]
    sd[conv + '.weight'] = rng.choice(np.asarray(wset, np.float32), size=shape)
    sd[bn + '.weight'] = rng.choice(np.asarray(gset, np.float32), size=cout)
    sd[bn + '.running_mean'] = np.zeros(cout, np.float32)
    sd[bn + '.running_var'] = np.full(cout, V_STAR, np.float32)
    sd[bn + '.num_batches_tracked'] = np.array(1000, dtype=np.int64)
    pre = F.conv2d(a, t64(sd, conv + '.weight'), None, stride, pad, 1, groups) * t64(sd, bn + '.weight').view(1, -1, 1, 1)
    if not relu:
        bias = rng.integers(-3, 4, size=cout).astype(np.float64)
        sd[bn + '.bias'] = bias.astype(np.float32)
        return pre + torch.from_numpy(bias).view(1, -1, 1, 1)
    if add is not None:
        pre = pre + add
    bias = relu_bias(rng, pre, clamp_all=clamp_all)
    sd[bn + '.bias'] = bias.astype(np.float32)
    return torch.relu(pre + torch.from_numpy(bias).view(1, -1, 1, 1))


def relu_bias(rng, pre, per_face=True, clamp_all=False):
    """integer bias [C] for a ReLU that follows pre [B,C,H,W] (see probe_conv_bn); per_face = False for a map of one pixel, where a
    channel that is positive on every face would never be clamped: one positive face is enough there"""
    cout = pre.shape[1]
    hi = pre.amax(dim=(2, 3))
    lo, hi = pre.amin(dim=(0, 2, 3)).numpy(), (hi.amin(dim=0) if per_face else hi.amax(dim=0)).numpy()      # per_face: the face whose largest element is smallest
    bias = np.floor(-lo) + 1                                                # smallest integer with lo + bias > 0
    fourth = rng.permutation(cout)[:cout if clamp_all else cout // 4]
    flat = np.sort(pre.permute(1, 0, 2, 3).reshape(cout, -1).numpy()[fourth], axis=1)
    cut = flat[np.arange(fourth.size), (rng.uniform(0.3, 0.7, fourth.size) * (flat.shape[1] - 1)).astype(int)]
    bias[fourth] = np.maximum(np.floor(-cut), np.floor(-hi[fourth]) + 1)
    return bias


def relu_is_partly_clamped(y):
    """a ReLU map [B,C,H,W] of the probe: something is clamped in the map and no channel is dead"""
    return bool((y == 0).any()) and bool((y.amax(dim=(0, 2, 3)) > 0).all())


def is_multiple(y, q):
    y = torch.as_tensor(y) * 2.0 ** q
    return bool(torch.equal(y, torch.round(y)))


def conv_magnitude(sd, conv, bn, a, stride, pad, groups):
    """|s| sum |a||w| + |shift| elementwise: no partial sum of the stage, in any order, exceeds its maximum"""
    s, shift, _ = fold64(sd, bn)
    mag = F.conv2d(a.abs(), t64(sd, conv + '.weight').abs(), None, stride, pad, 1, groups)
    return mag * s.abs().view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)


# ---- bound propagation: every rule takes and returns (exact activation, elementwise bound), NCHW float64 ---------------------------------
# A length-n dot product summed in fp32 in ANY order, with or without FMA, is within n u sum |a_k||w_k| of the exact one (first order); the
# fold adds 3 roundings in scale and 2 in shift, the epilogue 2, one to spare: n + 8.  The shift enters as |beta| + |mean s| because the
# fold rounds both terms before they cancel.  An input that is itself off by e_in moves the output by at most |s| sum |w| e_in.
def conv_bn_pair(sd, conv, bn, a, e, stride, pad, groups):
    """conv + folded BN: (n + 8) u (|s| sum |a||w| + |beta| + |mean s|) + |s| sum |w| e_in, n = taps x input channels of the group"""
    w = t64(sd, conv + '.weight')
    s, shift, shift_abs = fold64(sd, bn)
    n = w.shape[1] * w.shape[2] * w.shape[3]
    y = F.conv2d(a, w, None, stride, pad, 1, groups) * s.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    mag = F.conv2d(a.abs(), w.abs(), None, stride, pad, 1, groups) * s.abs().view(1, -1, 1, 1) + shift_abs.view(1, -1, 1, 1)
    b = (n + 8) * U * mag
    if e is not None:
        b = b + F.conv2d(e, w.abs(), None, stride, pad, 1, groups) * s.abs().view(1, -1, 1, 1)
    return y, b


def relu_pair(a, e):
    """1-Lipschitz: the bound is carried"""
    return torch.relu(a), e


def max_pool_pair(a, e, k, stride, pad):
    """1-Lipschitz in the maximum norm of the window: the largest bound of the window"""
    return F.max_pool2d(a, k, stride, pad), F.max_pool2d(e, k, stride, pad)


def add_pair(x, ex, y, ey):
    """e_x + e_y + u |x + y| (either bound may be None: an operand given exactly)"""
    z = x + y
    e = U * z.abs()
    for part in (ex, ey):
        if part is not None:
            e = e + part
    return z, e


def mean_pair(a, e):
    """mean over HW: (HW + 1) u mean|a| + mean(e)"""
    hw = a.shape[2] * a.shape[3]
    b = (hw + 1) * U * a.abs().mean(dim=(2, 3))
    if e is not None:
        b = b + e.mean(dim=(2, 3))
    return a.mean(dim=(2, 3)), b


def heads_pair(sd, names, pool, e=None):
    """the linear heads on a pool [B,C]: (C + 2) u (sum |W||p| + |b|), plus sum |W| e where the pool itself carries a bound"""
    p = torch.as_tensor(np.asarray(pool)).to(F64)
    out, b = [], []
    for n in names:
        w, bias = t64(sd, n + '.weight'), t64(sd, n + '.bias')
        out.append(p @ w.t() + bias)
        part = (p.shape[1] + 2) * U * (p.abs() @ w.abs().t() + bias.abs())
        if e is not None:
            part = part + torch.as_tensor(np.asarray(e)).to(F64) @ w.abs().t()
        b.append(part)
    return torch.cat(out, dim=1), torch.cat(b, dim=1)


def bias_conv_pair(sd, conv, a, e):
    """a 1x1 convolution with a bias and no BatchNorm (SE's conv_reduce / conv_expand, conv_head) on [B,C]: the conv rule with s = 1,
    (n + 8) u (sum |a||w| + |b|) + sum |w| e_in"""
    w, b = t64(sd, conv + '.weight').flatten(1), t64(sd, conv + '.bias')
    return affine_pair(w, b, b.abs(), a, e)


def affine_pair(w, b, b_abs, a, e):
    """a [B,K] times w [N,K] plus b: (K + 8) u (sum |a||w| + b_abs) + sum |w| e_in; b_abs = the sum of the absolute values of the terms
    the bias is folded from (they round before they cancel)"""
    bound = (w.shape[1] + 8) * U * (a.abs() @ w.abs().t() + b_abs)
    if e is not None:
        bound = bound + e @ w.abs().t()
    return a @ w.t() + b, bound


def hard_sigmoid_pair(z, e):
    """relu6(z + 3) / 6: e / 6 + 2 u"""
    return torch.clamp(z + 3.0, 0.0, 6.0) / 6.0, e / 6.0 + 2 * U


def gated_pair(a, e, g):
    """a [B,C,H,W] times a GIVEN gate g [B,C]: |g| e_a + u |a g|"""
    g = g.view(g.shape[0], -1, 1, 1)
    y = a * g
    return y, (g.abs() * e if e is not None else 0.0) + U * y.abs()


def avg_pool_pair(a, e, k, stride, pad, ceil_mode=False, count_include_pad=True):
    """An average pool that adds its k^2 window terms in fp32 and multiplies by a reciprocal: k^2 - 1 additions, the reciprocal (1 / 9 is
    no fp32 number) and the product are k^2 + 1 roundings, one to spare: (k^2 + 2) u avg|a| + avg(e), both averages with the pool's own
    divisor."""
    pool = lambda t: F.avg_pool2d(t, k, stride, pad, ceil_mode=ceil_mode, count_include_pad=count_include_pad)
    b = (k * k + 2) * U * pool(a.abs())
    return pool(a), b if e is None else b + pool(e)


EXPF_ULP = 1.0          # largest error of the device's expf in ulp, as the HIP math API documents it (1 ulp = 2 u relative)


def softmax2_pair(z0, e0, z1, e1):
    """The two-way softmax att0 = exp(z0 - m) / (exp(z0 - m) + exp(z1 - m)), m = max(z0, z1), and att1 alike -> (att0, bound, att1, bound).
    att0 = sigma(z0 - z1) and d sigma / dd = att0 (1 - att0) = att0 att1, so what the inputs carry and the rounding of the one
    subtraction that is not x - x move either output by att0 att1 (e_z0 + e_z1 + u |z0 - z1|).  The operations behind it act on the
    value relatively: the two expf 2 EXPF_ULP u each (att0 = E0 / (E0 + E1) has the sensitivities att1 and -att1 to relative changes
    of E0 and E1, in sum below one expf's 2 EXPF_ULP u twice over: 4 EXPF_ULP u), the addition, the division and the product one u
    each: (4 EXPF_ULP + 3) u, one u to spare.  An exponential below the normal range may be flushed: 2^-126 absolute.  First order, as
    every rule here; the constant comes from the count and the documented EXPF_ULP, not from a measurement."""
    a0, a1 = torch.softmax(torch.stack([z0, z1]), dim=0)
    slope = a0 * a1 * (e0 + e1 + U * (z0 - z1).abs())
    rel = (4 * EXPF_ULP + 4) * U
    return a0, slope + rel * a0 + 2.0 ** -126, a1, slope + rel * a1 + 2.0 ** -126


def separating(rng, v, e, count):
    """`count` draws from the quarter (at least 16) of the columns of v [8,C] that separate the distinct faces best: the widest gap between sorted
    neighbours with 2 .. 6 faces below it, over the column's largest bound e"""
    srt = np.sort(np.asarray(v), axis=0)
    score = (srt[2:7] - srt[1:6]).max(axis=0) / np.maximum(np.asarray(e).max(axis=0), 1e-300)
    best = np.argsort(score)[-max(v.shape[1] // 4, min(v.shape[1], 16)):]
    return rng.choice(best, size=count)
