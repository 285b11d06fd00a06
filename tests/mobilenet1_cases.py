"""Test infrastructure of the MobileNetV1 backbones: a torch-functional restatement of the reference network
(backbone_nets/mobilenetv1_backbone.py:21-44 DepthWiseBlock, :108-140 MobileNet.forward) with the BatchNorms folded, written against
the state_dict alone -- it shares nothing with the library's packing code (csrc/synergy_abi.hip pack_backbone_mobilenet1) -- plus the
inputs the CPU and GPU tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'mobilenet1_outputs.npz')
WIDTHS = {'mobilenet_1': 1.0, 'mobilenet_05': 0.5, 'mobilenet_2': 2.0}
ARCH_IDS = {'mobilenet_1': 2, 'mobilenet_05': 3, 'mobilenet_2': 4}
TAG = {1.0: '1', 0.5: '05', 2.0: '2'}           # suffix of a width's arrays in the golden file
SEEDS = {1.0: 1357, 0.5: 1358, 2.0: 1359}       # weights of the golden file (1, 05) and of the GPU tests (all three)
CROPS_SEED = 41
BLOCKS = ['dw2_1', 'dw2_2', 'dw3_1', 'dw3_2', 'dw4_1', 'dw4_2', 'dw5_1', 'dw5_2', 'dw5_3', 'dw5_4', 'dw5_5', 'dw5_6', 'dw6']
STRIDE2 = ('dw2_2', 'dw3_2', 'dw4_2', 'dw5_6')
TOL = 1e-4                                      # the project's bar (TOL of tests/test_gpu_parity.py)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _t(sd, key, dtype):
    v = sd[key]
    v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    return v.to(dtype)


def _conv_bn_relu(sd, x, conv, bn, stride, pad, groups, dtype):
    """conv, then y * scale + shift with scale = gamma / sqrt(var + 1e-5), shift = beta - mean * scale, then ReLU"""
    g, b = _t(sd, bn + '.weight', dtype), _t(sd, bn + '.bias', dtype)
    m, v = _t(sd, bn + '.running_mean', dtype), _t(sd, bn + '.running_var', dtype)
    scale = g / torch.sqrt(v + 1e-5)
    shift = b - m * scale
    y = F.conv2d(x, _t(sd, conv + '.weight', dtype), None, stride, pad, 1, groups)
    return torch.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))


def mobilenet1_forward(sd, x, width, dtype=torch.float32):
    """sd: state_dict (numpy or torch, reference key names, no prefix); x: [B,3,120,120] normalised crops.
    Returns (out102 [B,102] = ori | shape | exp | tex, pool [B, int(1024 width)]) as numpy."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    with torch.no_grad():
        y = _conv_bn_relu(sd, x, 'conv1', 'bn1', 2, 1, 1, dtype)
        for key in BLOCKS:
            y = _conv_bn_relu(sd, y, key + '.conv_dw', key + '.bn_dw', 2 if key in STRIDE2 else 1, 1, y.shape[1], dtype)
            y = _conv_bn_relu(sd, y, key + '.conv_sep', key + '.bn_sep', 1, 0, 1, dtype)
        assert y.shape[1] == int(1024 * width) and y.shape[2] == 4
        pool = y.mean(dim=(2, 3))
        heads = [pool @ _t(sd, n + '.weight', dtype).t() + _t(sd, n + '.bias', dtype) for n in ('fc_ori', 'fc_shape', 'fc_exp', 'fc_tex')]
        out = torch.cat(heads, dim=1)
    return out.numpy(), pool.numpy()


def normalize_u8(crops_u8):
    """uint8 HWC crops -> the fp32 CHW input of the reference (synergy3DMM.py:189-192)."""
    return ((np.asarray(crops_u8).astype(np.float32) - 127.5) / 128.0).transpose(0, 3, 1, 2).copy()


def border_crops():
    """uint8 crops [6,120,120,3] whose borders and neighbours tell schedules apart: constant 0 (a pad that were PIXEL 0 instead of
    normalised 0 would go unnoticed only here), constant 255, one-pixel checkerboards of both phases, and again 255 / 0 -- every
    batch slot differs from its neighbours, so a depthwise tap that read the next face's rows changes the result."""
    yy, xx = np.mgrid[0:120, 0:120]
    chk = (((yy + xx) & 1) * 255).astype(np.uint8)
    c = np.zeros((6, 120, 120, 3), dtype=np.uint8)
    c[1] = 255
    c[2] = chk[..., None]
    c[3] = 255 - chk[..., None]
    c[3, :, :, 1] = chk                      # one channel in the other phase
    c[4] = 255
    c[5] = 0
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# One layer at a time (syn_mobilenet1_layer, tests/test_gpu_mobilenet1_layers.py): layer 0 = stem, 1..13 = BLOCKS[layer - 1],
# 14 = pool + heads.  Activations between layers are NHWC, as the library keeps them.
# ---------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24                                  # unit roundoff of fp32
HEADS62 = ('fc_ori', 'fc_shape', 'fc_exp')      # the 62 outputs the library computes, in the cat order
V_STAR = np.float32(1) - np.float32(1e-5)       # running_var with fl32(v + 1e-5f) == 1: scale == gamma exactly (asserted in test_mobilenet1_cpu.py)
V_STAR64 = np.float64(1) - np.float64(1e-5)     # its float64 counterpart: v + 1e-5 == 1 in float64 (asserted there too)
PROBE_SEED = 20240
ARCH_OF = {w: a for a, w in WIDTHS.items()}


def layer_shapes(width):
    """[(hin, cin, hout, cout)] of layers 0..14; the stem reads 120^2 x 3, layer 14 reads 4^2 x pool and writes 62 numbers per face."""
    c0, shapes, h = int(32 * width), [], 60
    shapes.append((120, 3, 60, c0))
    chans = [(32, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512)] + [(512, 512)] * 5 + [(512, 1024), (1024, 1024)]
    for key, (ci, co) in zip(BLOCKS, chans):
        ho = (h - 1) // 2 + 1 if key in STRIDE2 else h
        shapes.append((h, int(ci * width), ho, int(co * width)))
        h = ho
    shapes.append((4, int(1024 * width), 1, 62))
    return shapes


def probe_batches(width, layer):
    """The batches of the integer probe, the smallest at which each tiling edge of a 64-pixel tile exists.  B = 1, every layer: 3600 =
    56 * 64 + 16, 900 = 14 * 64 + 4, 225 = 3 * 64 + 33, 64 = one tile, 16 = one MFMA tile and 48 dead pixels.  B = 3 where the map is
    15^2 (675 pixels: tiles straddle two faces).  B = 5 where it is 8^2 or 4^2 (320 and 80 pixels), and pool + heads."""
    hout = layer_shapes(width)[layer][2]
    return [1] + ([3] if hout == 15 else []) + ([5] if hout in (8, 4) or layer == 14 else [])


def _nchw(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def _block_args(layer):
    key = BLOCKS[layer - 1]
    return key, (2 if key in STRIDE2 else 1)


def heads_reference(sd, pool, dtype=torch.float64):
    """[B,62] = ori | shape | exp of a given pool [B,pool]"""
    p = torch.as_tensor(np.asarray(pool)).to(dtype)
    return torch.cat([p @ _t(sd, n + '.weight', dtype).t() + _t(sd, n + '.bias', dtype) for n in HEADS62], dim=1).numpy()


def pointwise_reference(sd, layer, dw, dtype=torch.float64):
    """the block's conv_sep + bn_sep + ReLU of a given depthwise output (NHWC in, NHWC out)"""
    key, _ = _block_args(layer)
    with torch.no_grad():
        return _nhwc(_conv_bn_relu(sd, _nchw(dw, dtype), key + '.conv_sep', key + '.bn_sep', 1, 0, 1, dtype))


def layer_reference(sd, width, layer, x, dtype=torch.float64):
    """One layer from the state_dict.  x: layer 0 the normalised crops [B,3,120,120] (CHW, as the reference module takes them), else
    the layer's NHWC input.  Returns NHWC numpy: the stem's output; for a block (depthwise_out, out); for layer 14 (pool, param62)."""
    with torch.no_grad():
        if layer == 0:
            return _nhwc(_conv_bn_relu(sd, torch.as_tensor(np.asarray(x)).to(dtype), 'conv1', 'bn1', 2, 1, 1, dtype))
        if layer == 14:
            pool = torch.as_tensor(np.asarray(x)).to(dtype).mean(dim=(1, 2))
            return pool.numpy(), heads_reference(sd, pool, dtype)
        key, stride = _block_args(layer)
        xin = _nchw(x, dtype)
        d = _conv_bn_relu(sd, xin, key + '.conv_dw', key + '.bn_dw', stride, 1, xin.shape[1], dtype)
        y = _conv_bn_relu(sd, d, key + '.conv_sep', key + '.bn_sep', 1, 0, 1, dtype)
        return _nhwc(d), _nhwc(y)


# ---- the fp32 bound of one layer -------------------------------------------------------------------------------------------------
# A length-n dot product summed in fp32 in ANY order, with or without FMA, is within n u sum |a_k||w_k| of the exact one (first order; the
# library's fold adds 3 roundings in scale and 2 in shift, the epilogue 2, one to spare: n + 8).  The shift enters as |beta| + |mean s|,
# not |beta - mean s|: the fold rounds both terms before they cancel.  ReLU is 1-Lipschitz, so the bound survives it.
def _conv_bound(sd, a, conv, bn, n, stride, pad, groups):
    """elementwise (n + 8) u (|s| sum |a||w| + |beta| + |mean s|), NCHW float64, and |s| [C]"""
    f = torch.float64
    g, b = _t(sd, bn + '.weight', f), _t(sd, bn + '.bias', f)
    m, v = _t(sd, bn + '.running_mean', f), _t(sd, bn + '.running_var', f)
    s = (g / torch.sqrt(v + 1e-5)).abs()
    mag = F.conv2d(a.abs(), _t(sd, conv + '.weight', f).abs(), None, stride, pad, 1, groups)
    return (n + 8) * U * (mag * s.view(1, -1, 1, 1) + (b.abs() + m.abs() * s).view(1, -1, 1, 1)), s


def bound_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound; an element whose bound is 0 (every term of it is 0) has to match exactly"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert err.shape == bound.shape and (bound >= 0).all()
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def pointwise_bound(sd, layer, dw):
    """bound of the block's pointwise half on a GIVEN depthwise output (NHWC): n = K"""
    key, _ = _block_args(layer)
    with torch.no_grad():
        a = _nchw(dw, torch.float64)
        return _nhwc(_conv_bound(sd, a, key + '.conv_sep', key + '.bn_sep', a.shape[1], 1, 0, 1)[0])


def heads_bound(sd, pool):
    """(C + 2) u (sum |W||pool| + |b|) of the 62 outputs on a GIVEN pool [B,C]"""
    p = torch.as_tensor(np.asarray(pool)).to(torch.float64).abs()
    mag = torch.cat([p @ _t(sd, n + '.weight', torch.float64).abs().t() + _t(sd, n + '.bias', torch.float64).abs() for n in HEADS62], dim=1)
    return ((p.shape[1] + 2) * U * mag).numpy()


def layer_bound(sd, width, layer, x):
    """Elementwise fp32 bound of |got - layer_reference(float64)|, NHWC, x as layer_reference takes it.  Stem: the bound with n = 27.
    Block: (depthwise bound with n = 9, whole-block bound = the pointwise bound on the reference's depthwise output plus the depthwise
    bound carried through |s| sum_k |w_nk| bound_dw,k).  Layer 14: (17 u mean|x| for the pool, None -- the heads are judged on the pool
    the library returned: heads_reference / heads_bound)."""
    f = torch.float64
    with torch.no_grad():
        if layer == 0:
            return _nhwc(_conv_bound(sd, torch.as_tensor(np.asarray(x)).to(f), 'conv1', 'bn1', 27, 2, 1, 1)[0])
        if layer == 14:
            return (17 * U * torch.as_tensor(np.asarray(x)).to(f).abs().mean(dim=(1, 2))).numpy(), None
        key, stride = _block_args(layer)
        xin = _nchw(x, f)
        K = xin.shape[1]
        bd, _ = _conv_bound(sd, xin, key + '.conv_dw', key + '.bn_dw', 9, stride, 1, K)
        d = _conv_bn_relu(sd, xin, key + '.conv_dw', key + '.bn_dw', stride, 1, K, f)
        bp, s = _conv_bound(sd, d, key + '.conv_sep', key + '.bn_sep', K, 1, 0, 1)
        carried = F.conv2d(bd, _t(sd, key + '.conv_sep.weight', f).abs()) * s.view(1, -1, 1, 1)
        return _nhwc(bd), _nhwc(bp + carried)


# ---- the integer probe: weights and inputs on which every layer is exact in fp32 whatever the order of summation -------------------
def integer_input(layer, width, B, seed=PROBE_SEED):
    """The probe input of a layer.  Stem: uint8 HWC crops over the full 0..255 ((x - 127.5) / 128 is exact in fp32, 8 fractional bits).
    Otherwise integer-valued fp32 in [-3, 3], NHWC -- the kernels are general, negative inputs are legitimate although a ReLU network
    never supplies them.  Every face draws its own values, so neighbouring faces always differ."""
    rng = np.random.default_rng([seed, layer, int(width * 10), B])
    hin, cin, _, _ = layer_shapes(width)[layer]
    if layer == 0:
        return rng.integers(0, 256, size=(B, 120, 120, 3), dtype=np.uint8)
    x = rng.integers(-3, 4, size=(B, hin, hin, cin)).astype(np.float32)
    if layer == 14:                              # no pooled feature of the probe is 0: a 4x4 sum that came out 0 has its first pixel moved by one
        dead = x.sum(axis=(1, 2)) == 0
        x[:, 0, 0, :] += np.where(dead, np.where(x[:, 0, 0, :] < 3, 1, -1), 0).astype(np.float32)
    return x


_INT_STATES = {}


def make_integer_state(seed, width):
    """A state_dict on which every layer of the network is exact in fp32 on integer_input: conv and head weights drawn from {-2, -1, 1, 2}
    (no zeros: a zero weight hides its term), running_mean 0, running_var V_STAR (the library's scale is then gamma itself), BN weight from
    {0.5, 1, 2, -1}, integer BN and head biases (with mean 0 the folded shift is the bias).
    The biases keep ReLU from hiding the probe.  In every convolution three channels in four (a random choice of positions, not one lane
    of a channel quad) get the smallest integer bias that lifts the whole channel above 0 on the canonical input integer_input(layer,
    width, 1); the fourth gets the integer bias that clamps a share of the channel drawn from 30 .. 70 % there (a draw from a fixed range
    such as [-8, 8] leaves a pointwise channel, whose values sit far from 0 because its input is non-negative, all positive or all
    clamped, and kills a narrow depthwise channel), raised where needed until one element of the channel is positive.  About an eighth of a map is then clamped and no channel is dead.  (Cached: the choice needs one float64 pass over one face.)"""
    if (seed, width) in _INT_STATES:
        return _INT_STATES[seed, width]
    rng = np.random.default_rng([seed, int(width * 10)])
    f = torch.float64
    sd = {}

    def conv_bn(conv, bn, shape, a, stride, pad, groups):
        cout = shape[0]
        sd[conv + '.weight'] = rng.choice(np.array([-2, -1, 1, 2], np.float32), size=shape)
        sd[bn + '.weight'] = rng.choice(np.array([0.5, 1, 2, -1], np.float32), size=cout)
        sd[bn + '.running_mean'] = np.zeros(cout, np.float32)
        sd[bn + '.running_var'] = np.full(cout, V_STAR, np.float32)
        sd[bn + '.num_batches_tracked'] = np.array(1000, dtype=np.int64)
        pre = F.conv2d(a, _t(sd, conv + '.weight', f), None, stride, pad, 1, groups) * _t(sd, bn + '.weight', f).view(1, -1, 1, 1)
        lo, hi = pre.amin(dim=(0, 2, 3)).numpy(), pre.amax(dim=(0, 2, 3)).numpy()
        bias = np.floor(-lo) + 1                                            # smallest integer with lo + bias > 0
        fourth = rng.permutation(cout)[:cout // 4]
        flat = np.sort(pre.permute(1, 0, 2, 3).reshape(cout, -1).numpy()[fourth], axis=1)
        cut = flat[np.arange(fourth.size), (rng.uniform(0.3, 0.7, fourth.size) * (flat.shape[1] - 1)).astype(int)]
        bias[fourth] = np.maximum(np.floor(-cut), np.floor(-hi[fourth]) + 1)
        sd[bn + '.bias'] = bias.astype(np.float32)
        return torch.relu(pre + torch.from_numpy(bias).view(1, -1, 1, 1))

    with torch.no_grad():
        c0 = int(32 * width)
        conv_bn('conv1', 'bn1', (c0, 3, 3, 3), torch.from_numpy(normalize_u8(integer_input(0, width, 1))).to(f), 2, 1, 1)
        for layer, key in enumerate(BLOCKS, start=1):
            _, cin, _, cout = layer_shapes(width)[layer]
            stride = 2 if key in STRIDE2 else 1
            d = conv_bn(key + '.conv_dw', key + '.bn_dw', (cin, 1, 3, 3), _nchw(integer_input(layer, width, 1), f), stride, 1, cin)
            conv_bn(key + '.conv_sep', key + '.bn_sep', (cout, cin, 1, 1), d, 1, 0, 1)
    pool = int(1024 * width)
    for name, n in (('fc_ori', 12), ('fc_shape', 40), ('fc_exp', 10), ('fc_tex', 40)):
        sd[name + '.weight'] = rng.choice(np.array([-2, -1, 1, 2], np.float32), size=(n, pool))
        sd[name + '.bias'] = rng.integers(-8, 9, size=n).astype(np.float32)
    _INT_STATES[seed, width] = sd
    return sd


def reference_state(sd):
    """The integer state as the float64 reference has to see it.  The library folds in fp32, where V_STAR + 1e-5f rounds to 1 and the
    scale is gamma; in float64 the same fp32 number plus 1e-5 is 1 - 1.4e-8, which would make the reference describe another network
    than the one the library runs.  So the reference gets the float64 number with the same property (V_STAR64) and nothing else changes."""
    assert all(np.all(v == V_STAR) for k, v in sd.items() if k.endswith('running_var'))
    return {k: (np.full(v.shape, V_STAR64, np.float64) if k.endswith('running_var') else v) for k, v in sd.items()}


def exactness_margin(sd, width, layer, x):
    """(largest magnitude any partial sum of the layer can reach) x (common denominator of every term), per stage: [(name, value)].
    Below 2^24 every partial sum, in any order, with or without FMA, is an fp32 number.  The magnitude is the analytic bound
    n max|a| max|w| max|gamma| + max|bias|; denominators: the normalised crop 256, BN weight 2, the 4x4 mean 16."""
    def stage(conv, bn, n, amax, den):
        w, g, b = np.abs(sd[conv + '.weight']).max(), np.abs(sd[bn + '.weight']).max(), np.abs(sd[bn + '.bias']).max()
        return (n * amax * w * g + b) * den * 2
    if layer == 0:
        return [('stem', stage('conv1', 'bn1', 27, 1.0, 256))]
    if layer == 14:
        amax = float(np.abs(x).max())
        w = max(np.abs(sd[n + '.weight']).max() for n in HEADS62)
        b = max(np.abs(sd[n + '.bias']).max() for n in HEADS62)
        return [('pool', 16 * amax * 16), ('heads', (np.asarray(x).shape[-1] * amax * w + b) * 16)]
    key, _ = _block_args(layer)
    d, _ = layer_reference(sd, width, layer, x)
    K = d.shape[-1]
    return [('depthwise', stage(key + '.conv_dw', key + '.bn_dw', 9, float(np.abs(x).max()), 1)),
            ('pointwise', stage(key + '.conv_sep', key + '.bn_sep', K, float(d.max()), 2))]
