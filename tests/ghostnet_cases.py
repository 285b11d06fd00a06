"""Test infrastructure of the GhostNet backbone: a torch-functional restatement of the reference network
(backbone_nets/ghostnet_backbone.py:41-233: SqueezeExcite, ConvBnAct, GhostModule, GhostBottleneck, GhostNet.forward) with the BatchNorms
folded, written against the state_dict alone -- it shares nothing with the library's packing code (csrc/synergy_abi.hip
pack_backbone_ghostnet) -- plus the shapes, seeds and inputs the CPU and GPU tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from mobilenet1_cases import border_crops, normalize_u8          # noqa: F401  (shared inputs)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ghostnet_outputs.npz')
ARCH_ID = 6
SEED = 2031                 # weights of the golden file and of the GPU tests
SEED_ALT = 2032
CROPS_SEED = 43
TOL = 1e-4                  # the project's bar (TOL of tests/test_gpu_parity.py)

# (key, in, mid, out, k, stride, SE reduced channels) as the issue's table states them; hin / hout follow from 60 and the strides
BLOCKS = [('blocks.0.0', 16, 16, 16, 3, 1, 0), ('blocks.1.0', 16, 48, 24, 3, 2, 0), ('blocks.2.0', 24, 72, 24, 3, 1, 0),
          ('blocks.3.0', 24, 72, 40, 5, 2, 20), ('blocks.4.0', 40, 120, 40, 5, 1, 32), ('blocks.5.0', 40, 240, 80, 3, 2, 0),
          ('blocks.6.0', 80, 200, 80, 3, 1, 0), ('blocks.6.1', 80, 184, 80, 3, 1, 0), ('blocks.6.2', 80, 184, 80, 3, 1, 0),
          ('blocks.6.3', 80, 480, 112, 3, 1, 120), ('blocks.6.4', 112, 672, 112, 3, 1, 168), ('blocks.7.0', 112, 672, 160, 5, 2, 168),
          ('blocks.8.0', 160, 960, 160, 5, 1, 0), ('blocks.8.1', 160, 960, 160, 5, 1, 240), ('blocks.8.2', 160, 960, 160, 5, 1, 0),
          ('blocks.8.3', 160, 960, 160, 5, 1, 240)]
SE_BLOCKS = [i for i, b in enumerate(BLOCKS) if b[6]]
HEADS = ('classifier_ori', 'classifier_shape', 'classifier_exp', 'classifier_texture')


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def block_shapes():
    """Per hook block 0..17: dict(cin, cout, hin, hout, mid, se, k, stride, aux) -- in = [B,hin,hin,cin], out = [B,hout,hout,cout] NHWC
    (block 17: out = [B,62]); aux = per-face element count of the hook's second output (SE gate / pool), 0 where there is none."""
    out, h = [], 60
    for key, cin, mid, cout, k, s, se in BLOCKS:
        ho = (h - 1) // s + 1
        out.append(dict(key=key, cin=cin, cout=cout, hin=h, hout=ho, mid=mid, se=se, k=k, stride=s, aux=mid if se else 0))
        h = ho
    assert h == 4
    out.append(dict(key='blocks.9.0', cin=160, cout=960, hin=4, hout=4, mid=0, se=0, k=1, stride=1, aux=0))
    out.append(dict(key='tail', cin=960, cout=62, hin=4, hout=1, mid=0, se=0, k=1, stride=1, aux=1280))
    return out


def mac_per_face():
    """Multiply-accumulates of the module with all four heads, from block_shapes() alone."""
    mac = 27 * 16 * 3600
    for b in block_shapes()[:16]:
        hw, hw2, m1, o1 = b['hin'] ** 2, b['hout'] ** 2, b['mid'] // 2, b['cout'] // 2
        mac += hw * (b['cin'] * m1 + 9 * m1)                                  # ghost1
        if b['stride'] == 2:
            mac += hw2 * b['k'] ** 2 * b['mid']
        mac += 2 * b['se'] * b['mid']
        mac += hw2 * (b['mid'] * o1 + 9 * o1)                                 # ghost2
        if b['cin'] != b['cout'] or b['stride'] != 1:
            mac += hw2 * (b['k'] ** 2 * b['cin'] + b['cin'] * b['cout'])
    return mac + 16 * 160 * 960 + 960 * 1280 + 1280 * 102


def _t(sd, key, dtype):
    v = sd[key]
    v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    return v.to(dtype)


def _conv_bn(sd, x, conv, bn, stride, pad, groups, relu, dtype):
    """conv, then y * scale + shift with scale = gamma / sqrt(var + 1e-5), shift = beta - mean * scale, then optionally ReLU"""
    g, b = _t(sd, bn + '.weight', dtype), _t(sd, bn + '.bias', dtype)
    m, v = _t(sd, bn + '.running_mean', dtype), _t(sd, bn + '.running_var', dtype)
    scale = g / torch.sqrt(v + 1e-5)
    shift = b - m * scale
    y = F.conv2d(x, _t(sd, conv + '.weight', dtype), None, stride, pad, 1, groups)
    y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def _ghost(sd, x, key, relu, dtype):
    p = _conv_bn(sd, x, key + '.primary_conv.0', key + '.primary_conv.1', 1, 0, 1, relu, dtype)
    c = _conv_bn(sd, p, key + '.cheap_operation.0', key + '.cheap_operation.1', 1, 1, p.shape[1], relu, dtype)
    return torch.cat([p, c], dim=1)


def _bottleneck(sd, x, blk, dtype):
    """One GhostBottleneck on NCHW x -> (output, SE gate [B,mid] or None)."""
    key, cin, mid, cout, k, s, se = blk
    y = _ghost(sd, x, key + '.ghost1', True, dtype)
    if s == 2:
        y = _conv_bn(sd, y, key + '.conv_dw', key + '.bn_dw', 2, k // 2, mid, False, dtype)
    gate = None
    if se:
        z = y.mean(dim=(2, 3), keepdim=True)
        z = torch.relu(F.conv2d(z, _t(sd, key + '.se.conv_reduce.weight', dtype), _t(sd, key + '.se.conv_reduce.bias', dtype)))
        z = F.conv2d(z, _t(sd, key + '.se.conv_expand.weight', dtype), _t(sd, key + '.se.conv_expand.bias', dtype))
        gate = torch.clamp(z + 3.0, 0.0, 6.0) / 6.0
        y = y * gate
        gate = gate.flatten(1)
    y = _ghost(sd, y, key + '.ghost2', False, dtype)
    if cin != cout or s != 1:
        r = _conv_bn(sd, x, key + '.shortcut.0', key + '.shortcut.1', s, k // 2, cin, False, dtype)
        r = _conv_bn(sd, r, key + '.shortcut.2', key + '.shortcut.3', 1, 0, 1, False, dtype)
    else:
        r = x
    return y + r, gate


def _tail(sd, y, dtype):
    """[B,960,4,4] -> (out102, pool1280)"""
    p = y.mean(dim=(2, 3))
    pool = torch.relu(p @ _t(sd, 'conv_head.weight', dtype).flatten(1).t() + _t(sd, 'conv_head.bias', dtype))
    out = torch.cat([pool @ _t(sd, n + '.weight', dtype).t() + _t(sd, n + '.bias', dtype) for n in HEADS], dim=1)
    return out, pool


def ghostnet_forward(sd, x, dtype=torch.float32, details=False):
    """sd: state_dict (numpy or torch, reference key names, no prefix); x: [B,3,120,120] normalised crops.  Returns (out102 [B,102] =
    ori | shape | exp | texture, pool [B,1280] = the act2 output) as numpy; with details also (block outputs: 17 NCHW arrays, blocks
    0..15 and blocks.9.0; gates: {block index: [B,mid]})."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    outs, gates = [], {}
    with torch.no_grad():
        y = _conv_bn(sd, x, 'conv_stem', 'bn1', 2, 1, 1, True, dtype)
        for i, blk in enumerate(BLOCKS):
            y, g = _bottleneck(sd, y, blk, dtype)
            outs.append(y.numpy())
            if g is not None:
                gates[i] = g.numpy()
        y = _conv_bn(sd, y, 'blocks.9.0.conv', 'blocks.9.0.bn1', 1, 0, 1, True, dtype)
        outs.append(y.numpy())
        assert y.shape[1:] == (960, 4, 4)
        out, pool = _tail(sd, y, dtype)
    if details:
        return out.numpy(), pool.numpy(), outs, gates
    return out.numpy(), pool.numpy()


def block_reference(sd, block, x_nhwc, dtype=torch.float64):
    """The hook's block (syn_ghostnet_block) on NHWC input, in `dtype`: (out NHWC -- [B,62] for block 17 --, aux or None) as numpy:
    aux = the SE gate [B,mid] of an SE block, the pool [B,1280] of block 17."""
    x = torch.as_tensor(np.asarray(x_nhwc)).to(dtype).permute(0, 3, 1, 2)
    with torch.no_grad():
        if block < 16:
            y, g = _bottleneck(sd, x, BLOCKS[block], dtype)
            return y.permute(0, 2, 3, 1).contiguous().numpy(), None if g is None else g.numpy()
        if block == 16:
            y = _conv_bn(sd, x, 'blocks.9.0.conv', 'blocks.9.0.bn1', 1, 0, 1, True, dtype)
            return y.permute(0, 2, 3, 1).contiguous().numpy(), None
        out, pool = _tail(sd, x, dtype)
        return out[:, :62].numpy(), pool.numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# One block at a time, every element judged (tests/test_gpu_ghostnet_blocks.py): the integer probe, its conditions, the one-place
# mistakes the probe has to see, and the elementwise fp32 bound of a block.  Shared machinery: tests/exact_probe.py.  Hook blocks:
# 0..15 bottlenecks, 16 ConvBnAct, 17 pool + conv_head + heads, 18 conv_stem + bn1 + ReLU.
# ---------------------------------------------------------------------------------------------------------------------------------
import exact_probe as ep          # noqa: E402

PROBE_SEED = 20261
N_FACES = ep.N_FACES
STEM = 18
WSET = (-2, -1, 1, 2)              # conv, conv_head and head weights of the probe
GSET = (1, -1)                     # BN weights of the bottlenecks: five chained stages leave no room for denominators
GSET_STEM = (0.5, 1, 2, -1)
SE_DOMINANT = 4096                 # one weight of every SE filter is that large (see make_integer_state)
HEADS62 = HEADS[:3]


def hook_counts(block):
    """per-face shapes (in, out, aux or None) of a hook block"""
    if block == STEM:
        return (3, 120, 120), (60, 60, 16), None
    s = block_shapes()[block]
    return (s['hin'], s['hin'], s['cin']), ((62,) if block == 17 else (s['hout'], s['hout'], s['cout'])), ((s['aux'],) if s['aux'] else None)


def integer_faces(block, n=N_FACES, seed=PROBE_SEED):
    """The n distinct faces of a block's probe.  Block 18: normalised crops [n,3,120,120], (x - 127.5) / 128 of uint8 x over the full range.
    Otherwise NHWC integers in [-3, 3]: every (face, channel) draws an offset from {-2 .. 2} and every pixel adds {-1, 0, 1} to it, so
    that the channel means -- what squeeze-and-excite sees -- differ between the faces by as much as the pixels differ within one."""
    rng = np.random.default_rng([seed, block, n])
    if block == STEM:
        return normalize_u8(rng.integers(0, 256, size=(n, 120, 120, 3), dtype=np.uint8))
    h, _, c = hook_counts(block)[0]
    return (rng.integers(-2, 3, size=(n, 1, 1, c)) + rng.integers(-1, 2, size=(n, h, h, c))).astype(np.float32)


def integer_input(block, B):
    """a probe batch: slot i holds distinct face exact_probe.batch_index(B)[i]"""
    return np.ascontiguousarray(integer_faces(block)[ep.batch_index(B)])


def _fold(sd, bn, dtype):
    g, b = _t(sd, bn + '.weight', dtype), _t(sd, bn + '.bias', dtype)
    m, v = _t(sd, bn + '.running_mean', dtype), _t(sd, bn + '.running_var', dtype)
    scale = g / torch.sqrt(v + 1e-5)
    return scale, b - m * scale


def _se_z(sd, key, y, dtype):
    """pre-activation of the SE gate [B,mid] of y [B,mid,H,W]"""
    m = y.mean(dim=(2, 3))
    r = torch.relu(m @ _t(sd, key + '.se.conv_reduce.weight', dtype).flatten(1).t() + _t(sd, key + '.se.conv_reduce.bias', dtype))
    return r @ _t(sd, key + '.se.conv_expand.weight', dtype).flatten(1).t() + _t(sd, key + '.se.conv_expand.bias', dtype)


def _se_pair(sd, key, y, e):
    """(z, bound of z) by the rules of exact_probe: the mean over HW, two bias-only 1x1 convolutions, ReLU between them"""
    m, em = ep.mean_pair(y, e)
    r, er = ep.bias_conv_pair(sd, key + '.se.conv_reduce', m, em)
    return ep.bias_conv_pair(sd, key + '.se.conv_expand', torch.relu(r), er)


# ---- the mistakes a port could make, each confined to ONE place of one block ---------------------------------------------------------
#   tap         ghost1's cheap operation at output pixel (1, 1): the centre tap read one pixel to the right
#   pad         ghost1's cheap operation at the corner pixel (0, 0): the padded tap (-1, -1) read from the clamped address instead of 0
#   kslot       a primary convolution with K = 8 mod 16 (ghost2's where mid is, else ghost1's): the first two k slots of the last, ragged
#               16-step (K - 8 and K - 7) swapped for the output channel quad 0..3
#   ntail       a primary convolution whose N is no multiple of 16 (ghost2's where it is ragged, else ghost1's): the last channel quad
#               takes the scale and shift of the quad before it
#   gate_face   the SE gate of the next face of the batch
#   halves      the two halves of the shortcut swapped where ghost2 adds it (pass_out)
#   dw_s2_edge  the stride-2 depthwise of the odd 15 -> 8 map: the padded taps of the last row and column read from the clamped address
VARIANTS = ('tap', 'pad', 'kslot', 'ntail', 'gate_face', 'halves', 'dw_s2_edge')


def _kslot_site(blk):
    key, cin, mid, cout, k, s, se = blk
    return 'ghost2' if mid % 16 == 8 else 'ghost1' if cin % 16 == 8 else None


def _ntail_site(blk):
    key, cin, mid, cout, k, s, se = blk
    return 'ghost2' if (cout // 2) % 16 else 'ghost1' if (mid // 2) % 16 else None


def variants_of(block):
    """the VARIANTS that exist on a hook block"""
    if block >= 16:
        return ()
    blk = BLOCKS[block]
    have = {'tap': True, 'pad': True, 'halves': True, 'kslot': _kslot_site(blk), 'ntail': _ntail_site(blk), 'gate_face': blk[6],
            'dw_s2_edge': blk[5] == 2 and block_shapes()[block]['hin'] % 2 == 1}
    return tuple(v for v in VARIANTS if have[v])


def _bottleneck_staged(sd, x, blk, dtype, variant=None, gate=None):
    """_bottleneck stage by stage -> (output, SE gate or None), with one of VARIANTS applied and / or the SE gate GIVEN ([B,mid]: the
    block that follows the gate is then judged apart from squeeze-and-excite)."""
    key, cin, mid, cout, k, s, se = blk
    assert variant is None or variant in VARIANTS

    def cb(a, conv, bn, stride, pad, groups, relu, fix=None, tail=False):
        y = F.conv2d(a, _t(sd, conv + '.weight', dtype), None, stride, pad, 1, groups)
        if fix is not None:
            y = fix(y, a, _t(sd, conv + '.weight', dtype))
        scale, shift = _fold(sd, bn, dtype)
        if tail:
            scale, shift = scale.clone(), shift.clone()
            scale[-4:], shift[-4:] = scale[-8:-4].clone(), shift[-8:-4].clone()
        y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        return torch.relu(y) if relu else y

    def kslot(y, a, w):
        K = a.shape[1]
        y = y.clone()
        y[:, 0:4] += (w[0:4, K - 8, 0, 0] - w[0:4, K - 7, 0, 0]).view(1, 4, 1, 1) * (a[:, K - 7] - a[:, K - 8]).unsqueeze(1)
        return y

    def tap(y, a, w):
        y = y.clone()
        y[:, :, 1, 1] += w[:, 0, 1, 1] * (a[:, :, 1, 2] - a[:, :, 1, 1])
        return y

    def pad(y, a, w):
        y = y.clone()
        y[:, :, 0, 0] += w[:, 0, 0, 0] * a[:, :, 0, 0]
        return y

    def edge(y, a, w):
        p = k // 2
        wrong = F.conv2d(F.pad(a, (p, p, p, p), mode='replicate'), w, None, 2, 0, 1, a.shape[1])
        y = y.clone()
        y[:, :, -1, :], y[:, :, :, -1] = wrong[:, :, -1, :], wrong[:, :, :, -1]
        return y

    def ghost(a, name, relu):
        site = key + '.' + name
        p = cb(a, site + '.primary_conv.0', site + '.primary_conv.1', 1, 0, 1, relu,
               fix=kslot if variant == 'kslot' and _kslot_site(blk) == name else None, tail=variant == 'ntail' and _ntail_site(blk) == name)
        c = cb(p, site + '.cheap_operation.0', site + '.cheap_operation.1', 1, 1, p.shape[1], relu,
               fix={'tap': tap, 'pad': pad}.get(variant) if name == 'ghost1' else None)
        return torch.cat([p, c], dim=1)

    y = ghost(x, 'ghost1', True)
    if s == 2:
        y = cb(y, key + '.conv_dw', key + '.bn_dw', 2, k // 2, mid, False, fix=edge if variant == 'dw_s2_edge' else None)
    g = None
    if se:
        g = torch.clamp(_se_z(sd, key, y, dtype) + 3.0, 0.0, 6.0) / 6.0 if gate is None else torch.as_tensor(np.asarray(gate)).to(dtype)
        y = y * (torch.roll(g, -1, dims=0) if variant == 'gate_face' else g).view(g.shape[0], -1, 1, 1)
    y = ghost(y, 'ghost2', False)
    r = x
    if cin != cout or s != 1:
        r = cb(x, key + '.shortcut.0', key + '.shortcut.1', s, k // 2, cin, False)
        r = cb(r, key + '.shortcut.2', key + '.shortcut.3', 1, 0, 1, False)
    if variant == 'halves':
        r = torch.cat([r[:, cout // 2:], r[:, :cout // 2]], dim=1)
    return y + r, g


def heads_reference(sd, pool, dtype=torch.float64):
    """[B,62] = ori | shape | exp of a given pool [B,1280]"""
    return ep.heads_pair(sd, HEADS62, pool)[0].to(dtype).numpy()


def heads_bound(sd, pool):
    """(C + 2) u (sum |W||pool| + |b|) of the 62 outputs on a GIVEN pool"""
    return ep.heads_pair(sd, HEADS62, pool)[1].numpy()


def probe_reference(sd, block, x, dtype=torch.float64, variant=None, gate=None):
    """block_reference for every hook block, 18 included (x: NCHW crops there), with one of VARIANTS applied or the SE gate given"""
    with torch.no_grad():
        if block == STEM:
            y = _conv_bn(sd, torch.as_tensor(np.asarray(x)).to(dtype), 'conv_stem', 'bn1', 2, 1, 1, True, dtype)
            return y.permute(0, 2, 3, 1).contiguous().numpy(), None
        if block >= 16 or (variant is None and gate is None):
            return block_reference(sd, block, x, dtype)
        xin = torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)
        y, g = _bottleneck_staged(sd, xin, BLOCKS[block], dtype, variant, gate)
        return y.permute(0, 2, 3, 1).contiguous().numpy(), None if g is None else g.numpy()


# ---- the probe's weights ----------------------------------------------------------------------------------------------------------------
_INT_STATE = {}


def make_integer_state(seed=PROBE_SEED):
    """A state_dict on which every hook block is exact in fp32 on integer_faces(block).  Convolutions: weights {-2, -1, 1, 2}, running_mean 0,
    running_var V_STAR, BN weight +-1 (the stem: {0.5, 1, 2, -1}), integer biases -- in front of a ReLU by the rule of
    exact_probe.probe_conv_bn on the 8 distinct faces, from [-3, 3] on the linear stages.
    Squeeze-and-excite: the gate must be an fp32 number whatever the rounding of the 225-pixel mean, and must depend on the face.
    conv_reduce has weights {-2, -1, 1, 2} and the bias of a ReLU stage, conv_expand weights {+-64, +-128}; per mid channel the 8
    pre-activations z (one per distinct face) are sorted, a wide gap that leaves 2 .. 6 faces below it is taken and the integer bias
    puts its middle at 0.  That rounding may not move z across the gap, so one weight of every conv_reduce and conv_expand filter is
    SE_DOMINANT times the others (+-1), on an input that separates the faces well (exact_probe.separating).  Every z is then far outside [-3, 3] (tests/test_ghostnet_cpu.py: |z| - 3 > 100 x the fp32 bound of z), the
    gate is exactly 0 or 1, and a channel is open on some faces and closed on the others.
    conv_head: weights {-2, -1, 1, 2}, the bias of a ReLU stage; heads: weights {-2, -1, 1, 2}, integer biases in [-8, 8]."""
    if seed in _INT_STATE:
        return _INT_STATE[seed]
    rng = np.random.default_rng(seed)
    sd, f = {}, ep.F64

    def cbn(conv, bn, shape, a, stride, pad, groups, relu, gset=GSET):
        return ep.probe_conv_bn(rng, sd, conv, bn, shape, a, stride, pad, groups, WSET, gset, relu=relu)

    def ghost(key, a, cout, relu):
        p = cbn(key + '.primary_conv.0', key + '.primary_conv.1', (cout // 2, a.shape[1], 1, 1), a, 1, 0, 1, relu)
        c = cbn(key + '.cheap_operation.0', key + '.cheap_operation.1', (cout // 2, 1, 3, 3), p, 1, 1, cout // 2, relu)
        return torch.cat([p, c], dim=1)

    def biased(conv, shape, a, wset, dominant=None):
        """a bias-only 1x1 convolution in front of a ReLU, on [B,C]; dominant: per filter the input whose weight is SE_DOMINANT times larger"""
        sd[conv + '.weight'] = rng.choice(np.asarray(wset, np.float32), size=shape)
        if dominant is not None:
            sd[conv + '.weight'][np.arange(shape[0]), dominant] *= SE_DOMINANT
        pre = a @ _t(sd, conv + '.weight', f).flatten(1).t()
        sd[conv + '.bias'] = ep.relu_bias(rng, pre.view(pre.shape[0], -1, 1, 1), per_face=False).astype(np.float32)
        return torch.relu(pre + _t(sd, conv + '.bias', f))

    with torch.no_grad():
        cbn('conv_stem', 'bn1', (16, 3, 3, 3), torch.from_numpy(integer_faces(STEM)).to(f), 2, 1, 1, True, GSET_STEM)
        for i, (key, cin, mid, cout, k, s, se) in enumerate(BLOCKS):
            x = torch.from_numpy(integer_faces(i)).to(f).permute(0, 3, 1, 2)
            y = ghost(key + '.ghost1', x, mid, True)
            if s == 2:
                y = cbn(key + '.conv_dw', key + '.bn_dw', (mid, 1, k, k), y, 2, k // 2, mid, False)
            if se:
                m, em = ep.mean_pair(*_stage_bound_to(sd, i, x))
                red = biased(key + '.se.conv_reduce', (se, mid, 1, 1), m, (-1, 1), ep.separating(rng, m, em, se))
                _, er = ep.bias_conv_pair(sd, key + '.se.conv_reduce', m, em)
                we = rng.choice(np.asarray((-1, 1), np.float32), size=(mid, se, 1, 1))
                we[np.arange(mid), ep.separating(rng, red, er, mid)] *= SE_DOMINANT
                sd[key + '.se.conv_expand.weight'] = we
                sd[key + '.se.conv_expand.bias'] = np.zeros(mid, np.float32)
                z, ez = (t.numpy() for t in ep.bias_conv_pair(sd, key + '.se.conv_expand', red, er))      # [8, mid]
                v = np.sort(z, axis=0)
                gaps = v[2:7] - v[1:6]                                                               # 2 .. 6 faces below the gap
                wide = gaps / 2 - 3 > 400 * ez.max(axis=0)                                           # four times the margin asked for
                wide[gaps.argmax(axis=0), np.arange(mid)] = True
                at = (rng.random(gaps.shape) * wide).argmax(axis=0) + 1                              # any of the wide gaps
                cols = np.arange(mid)
                bias = -np.rint((v[at, cols] + v[at + 1, cols]) / 2)
                sd[key + '.se.conv_expand.bias'] = bias.astype(np.float32)
                y = y * torch.from_numpy(((z + bias) > 0).astype(np.float64)).view(N_FACES, -1, 1, 1)
            ghost(key + '.ghost2', y, cout, False)
            if cin != cout or s != 1:
                r = cbn(key + '.shortcut.0', key + '.shortcut.1', (cin, 1, k, k), x, s, k // 2, cin, False)
                cbn(key + '.shortcut.2', key + '.shortcut.3', (cout, cin, 1, 1), r, 1, 0, 1, False)
        cbn('blocks.9.0.conv', 'blocks.9.0.bn1', (960, 160, 1, 1), torch.from_numpy(integer_faces(16)).to(f).permute(0, 3, 1, 2), 1, 0, 1, True)
        biased('conv_head', (1280, 960, 1, 1), torch.from_numpy(integer_faces(17)).to(f).mean(dim=(1, 2)), WSET)
    for name, n in zip(HEADS, (12, 40, 10, 40)):
        sd[name + '.weight'] = rng.choice(np.asarray(WSET, np.float32), size=(n, 1280))
        sd[name + '.bias'] = rng.integers(-8, 9, size=n).astype(np.float32)
    _INT_STATE[seed] = sd
    return sd


# ---- the conditions under which the probe is exact ------------------------------------------------------------------------------------
SE_MARGIN = {}                     # block -> smallest (|z| - 3) / bound of z that exactness_violations has seen, for the record


def exactness_violations(block, x, sd_ref=None):
    """The conditions of the probe on the float64 trace of one hook block (x as probe_reference takes it); returns the list of violations,
    empty = all hold.  Every convolution stage, the residual add included: the output is a multiple of 2^-q; 2^q (|s| sum |a||w| +
    |shift| (+ |residual|)) < 2^24, so every partial sum in any order is an fp32 number; the output is not constant; every ReLU map is
    partly clamped and has no dead channel.  q = 0 in the bottlenecks and the ConvBnAct, 9 in the stem (the normalised pixel and BN
    weight 0.5), 4 behind the mean of 16.  Squeeze-and-excite, where rounding is allowed because the gate is saturated: |z| - 3 > 100 x the
    fp32 bound of z (exact_probe's rules: mean, two bias-only convolutions, carried through ghost1); the gate is 0 or 1; 25 .. 75 % of
    it is open; every mid channel is open on one distinct face and closed on another; neighbouring faces of the batch differ."""
    sd = ep.reference_state(make_integer_state()) if sd_ref is None else sd_ref
    f, bad = ep.F64, []
    x = torch.as_tensor(np.asarray(x)).to(f)

    def stage(name, conv, bn, a, stride, pad, groups, relu, q=0, res=None):
        y = _conv_bn(sd, a, conv, bn, stride, pad, groups, relu, f)
        mag = ep.conv_magnitude(sd, conv, bn, a, stride, pad, groups)
        if res is not None:
            y, mag = y + res, mag + res.abs()
        if not ep.is_multiple(y, q):
            bad.append(f'{name}: output is no multiple of 2^-{q}')
        if not float(mag.max()) * 2.0 ** q < 2.0 ** 24:
            bad.append(f'{name}: 2^{q} (|s| sum |a||w| + |shift| + |residual|) = {float(mag.max()) * 2.0 ** q:.4g} >= 2^24')
        if float(y.min()) == float(y.max()):
            bad.append(f'{name}: constant output')
        if relu and not ep.relu_is_partly_clamped(y):
            bad.append(f'{name}: the ReLU map is not partly clamped, or a channel is dead')
        return y

    with torch.no_grad():
        if block == STEM:
            stage('conv_stem', 'conv_stem', 'bn1', x, 2, 1, 1, True, q=9)
            return bad
        x = x.permute(0, 3, 1, 2)
        if block == 16:
            stage('blocks.9.0', 'blocks.9.0.conv', 'blocks.9.0.bn1', x, 1, 0, 1, True)
            return bad
        if block == 17:
            m = x.mean(dim=(2, 3))
            w, b = _t(sd, 'conv_head.weight', f).flatten(1), _t(sd, 'conv_head.bias', f)
            pool = torch.relu(m @ w.t() + b)
            out, omag = ep.heads_pair(sd, HEADS62, pool)
            if not (ep.is_multiple(m, 4) and ep.is_multiple(pool, 4) and ep.is_multiple(out, 4)):
                bad.append('tail: no multiple of 2^-4')
            mags = (float(x.abs().sum(dim=(2, 3)).max()), 16 * float((m.abs() @ w.abs().t() + b.abs()).max()),
                    16 * float(omag.max()) / ((1280 + 2) * ep.U))
            if not max(mags) < 2.0 ** 24:
                bad.append(f'tail: partial sums {mags} reach 2^24')
            if not (bool((pool == 0).any(dim=1).all()) and bool((pool > 0).any(dim=1).all())) or float(out.min()) == float(out.max()):
                bad.append('tail: the pool of a face is not partly clamped, or the output is constant')
            return bad
        key, cin, mid, cout, k, s, se = BLOCKS[block]
        m1, o1 = mid // 2, cout // 2
        g1, g2 = key + '.ghost1', key + '.ghost2'
        p = stage(key + ' ghost1 primary', g1 + '.primary_conv.0', g1 + '.primary_conv.1', x, 1, 0, 1, True)
        c = stage(key + ' ghost1 cheap', g1 + '.cheap_operation.0', g1 + '.cheap_operation.1', p, 1, 1, m1, True)
        y = torch.cat([p, c], dim=1)
        if s == 2:
            y = stage(key + ' conv_dw', key + '.conv_dw', key + '.bn_dw', y, 2, k // 2, mid, False)
        if se:
            z, ez = _se_pair(sd, key, *_stage_bound_to(sd, block, x))
            g = torch.clamp(z + 3.0, 0.0, 6.0) / 6.0
            SE_MARGIN[block] = min(SE_MARGIN.get(block, np.inf), float(((z.abs() - 3.0) / ez).min()))
            if not bool((z.abs() - 3.0 > 100.0 * ez).all()):
                bad.append(f'{key} SE: |z| - 3 is within 100 x the bound of z (smallest ratio {float(((z.abs() - 3.0) / ez).min()):.3g})')
            if not bool(((g == 0) | (g == 1)).all()):
                bad.append(f'{key} SE: a gate is neither 0 nor 1')
            if not 0.25 <= float(g.mean()) <= 0.75:
                bad.append(f'{key} SE: {float(g.mean()):.2f} of the gate is open')
            if x.shape[0] > 1:
                if x.shape[0] == N_FACES and not bool(((g.amax(dim=0) == 1) & (g.amin(dim=0) == 0)).all()):
                    bad.append(f'{key} SE: a mid channel has the same gate on all distinct faces')
                if any(bool((g[i] == g[j]).all()) for i in range(g.shape[0]) for j in range(i) if not bool((x[i] == x[j]).all())):
                    bad.append(f'{key} SE: two different faces have the same gate')
            y = y * g.view(g.shape[0], -1, 1, 1)
        r = x
        if cin != cout or s != 1:
            r = stage(key + ' shortcut depthwise', key + '.shortcut.0', key + '.shortcut.1', x, s, k // 2, cin, False)
            r = stage(key + ' shortcut 1x1', key + '.shortcut.2', key + '.shortcut.3', r, 1, 0, 1, False)
        p2 = _conv_bn(sd, y, g2 + '.primary_conv.0', g2 + '.primary_conv.1', 1, 0, 1, False, f)
        stage(key + ' ghost2 primary + shortcut', g2 + '.primary_conv.0', g2 + '.primary_conv.1', y, 1, 0, 1, False, res=r[:, :o1])
        stage(key + ' ghost2 cheap + shortcut', g2 + '.cheap_operation.0', g2 + '.cheap_operation.1', p2, 1, 1, o1, False, res=r[:, o1:])
    return bad


# ---- the fp32 bound of a block --------------------------------------------------------------------------------------------------------
def _ghost_pair(sd, key, a, e, relu):
    p, ep_ = ep.conv_bn_pair(sd, key + '.primary_conv.0', key + '.primary_conv.1', a, e, 1, 0, 1)
    if relu:
        p = torch.relu(p)
    c, ec = ep.conv_bn_pair(sd, key + '.cheap_operation.0', key + '.cheap_operation.1', p, ep_, 1, 1, p.shape[1])
    if relu:
        c = torch.relu(c)
    return torch.cat([p, c], dim=1), torch.cat([ep_, ec], dim=1)


def _stage_bound_to(sd, block, x):
    """(activation, bound) of what squeeze-and-excite reads: ghost1 and, on a stride-2 block, conv_dw; x NCHW float64"""
    key, cin, mid, cout, k, s, se = BLOCKS[block]
    y, e = _ghost_pair(sd, key + '.ghost1', x, None, True)
    if s == 2:
        y, e = ep.conv_bn_pair(sd, key + '.conv_dw', key + '.bn_dw', y, e, 2, k // 2, mid)
    return y, e


def block_bound(sd, block, x, gate=None):
    """Elementwise bound of |got - probe_reference(float64)| for fp32 arithmetic on the fp32 input x -> (bound of out, bound of aux or
    None), in the layouts of probe_reference.  The hook returns no intermediate but the gate, so the bound is carried through the
    stages (exact_probe).  SE blocks: the gate's own bound (mean, reduce, expand, hard sigmoid, behind ghost1's bound); with `gate` GIVEN
    the output's bound is that of the block behind the gate -- the product |g| e + u |a g| in place of squeeze-and-excite -- against
    probe_reference(gate=gate).  Block 17: the pool's bound (the 16-term mean, conv_head, ReLU); the heads are judged on the returned
    pool (heads_reference / heads_bound), so out's bound is None."""
    f = ep.F64
    x = torch.as_tensor(np.asarray(x)).to(f)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().numpy()
    with torch.no_grad():
        if block == STEM:
            return nhwc(ep.conv_bn_pair(sd, 'conv_stem', 'bn1', x, None, 2, 1, 1)[1]), None
        x = x.permute(0, 3, 1, 2)
        if block == 16:
            return nhwc(ep.conv_bn_pair(sd, 'blocks.9.0.conv', 'blocks.9.0.bn1', x, None, 1, 0, 1)[1]), None
        if block == 17:
            return None, ep.bias_conv_pair(sd, 'conv_head', *ep.mean_pair(x, None))[1].numpy()
        key, cin, mid, cout, k, s, se = BLOCKS[block]
        y, e = _stage_bound_to(sd, block, x)
        eg = None
        if se:
            g, eg = ep.hard_sigmoid_pair(*_se_pair(sd, key, y, e))
            if gate is not None:
                g = torch.as_tensor(np.asarray(gate)).to(f)
            else:
                e = e + y.abs() * eg.view(eg.shape[0], -1, 1, 1)          # the gate's own error moves the product by |a| e_g
            y, e = ep.gated_pair(y, e, g)
        y, e = _ghost_pair(sd, key + '.ghost2', y, e, False)
        r, er = x, None
        if cin != cout or s != 1:
            r, er = ep.conv_bn_pair(sd, key + '.shortcut.0', key + '.shortcut.1', x, None, s, k // 2, cin)
            r, er = ep.conv_bn_pair(sd, key + '.shortcut.2', key + '.shortcut.3', r, er, 1, 0, 1)
        return nhwc(ep.add_pair(y, e, r, er)[1]), None if eg is None else eg.numpy()


def judge(sd, block, x, out, aux):
    """[(part, max err / bound)] of a hook block's results (numpy) on the fp32 input x against the float64 reference.  An SE block: the
    gate under its own bound, the output against the float64 block that uses the RETURNED gate (which isolates squeeze-and-excite from
    the two ghost modules).  Block 17: the pool under its bound, the heads on the returned pool."""
    ref, ref_aux = probe_reference(sd, block, x)
    if block == 17:
        return [('pool', ep.bound_ratio(aux, ref_aux, block_bound(sd, 17, x)[1])),
                ('heads', ep.bound_ratio(out, heads_reference(sd, aux), heads_bound(sd, aux)))]
    if block < 16 and BLOCKS[block][6]:
        return [('gate', ep.bound_ratio(aux, ref_aux, block_bound(sd, block, x)[1])),
                ('out', ep.bound_ratio(out, probe_reference(sd, block, x, gate=aux)[0], block_bound(sd, block, x, gate=aux)[0]))]
    return [('out', ep.bound_ratio(out, ref, block_bound(sd, block, x)[0]))]
