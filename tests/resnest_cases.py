"""Test infrastructure of the ResNeSt-50 backbone: a torch-functional restatement of the reference network
(backbone_nets/ResNeSt/resnet.py:29-324 Bottleneck and ResNet.forward, splat.py:11-98 SplAtConv2d and rSoftMax, built as resnest.py:33-41
builds it) with the BatchNorms folded, written against the state_dict alone -- it shares nothing with the library's packing code
(csrc/synergy_abi.hip pack_backbone_resnest50) -- plus the shapes, seeds and inputs the CPU and GPU tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from mobilenet1_cases import border_crops, normalize_u8          # noqa: F401  (shared inputs)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'resnest50_outputs.npz')
ARCH_ID = 8
SEED = 2741                 # weights of the golden file and of the GPU tests
CROPS_SEED = 47
TOL = 1e-4                  # the project's bar (TOL of tests/test_gpu_parity.py)

# (key, in, group width C, gate width, avd, downsample) as the issue states the network: layers 3 / 4 / 6 / 3 of C = 64 / 128 / 256 / 512,
# gate width max(C / 2, 32), avd in layer2.0 / 3.0 / 4.0, a downsample branch in every layerN.0
BLOCKS = []
_cin = 64
for _l, (_c, _count) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3))):
    for _i in range(_count):
        BLOCKS.append((f'layer{_l + 1}.{_i}', _cin, _c, max(_c // 2, 32), _l > 0 and _i == 0, _i == 0))
        _cin = 4 * _c
HEADS62 = ('fc_ori', 'fc_shape', 'fc_exp')      # what the module's forward concatenates; fc_tex is never called


def golden_crops():
    """The 2 synthetic uint8 crops [2,120,120,3] of the golden file: synth.make_crops noise blended half and half with one plane wave per
    face and colour channel.  Pure noise is the same face twice to this network -- four average pools leave nothing of it -- while a
    colour cast and a gradient survive them, as the differences between photographs do."""
    from synergynet_amd import synth
    f = synth.make_crops(2, seed=CROPS_SEED).astype(np.float32)
    rng = np.random.default_rng(CROPS_SEED)
    yy, xx = np.mgrid[0:120, 0:120] / 120.0
    for i in range(2):
        for ch in range(3):
            a, b, ph = rng.uniform(-1, 1, 3)
            f[i, :, :, ch] = 0.5 * f[i, :, :, ch] + 0.5 * (127.5 + 110.0 * np.sin(2 * np.pi * (a * yy + b * xx + ph)))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def block_shapes():
    """Per hook block 0..17: dict(key, cin, cout, hin, hout, C, inter, avd, down, aux) -- in = [B,hin,hin,cin], out = [B,hout,hout,cout]
    NHWC (block 17: out = [B,62]); aux = per-face element count of the hook's second output (attention / pool), 0 where there is none."""
    out = [dict(key='stem', cin=3, cout=64, hin=120, hout=30, C=0, inter=0, avd=False, down=False, aux=0)]
    h = 30
    for key, cin, c, inter, avd, down in BLOCKS:
        ho = (h + 1) // 2 if avd else h
        out.append(dict(key=key, cin=cin, cout=4 * c, hin=h, hout=ho, C=c, inter=inter, avd=avd, down=down, aux=2 * c))
        h = ho
    assert h == 4
    out.append(dict(key='tail', cin=2048, cout=62, hin=4, hout=1, C=0, inter=0, avd=False, down=False, aux=2048))
    return out


def mac_per_face():
    """Every product of the module's forward (Conv2d and Linear; fc_tex is never called), from block_shapes() alone."""
    mac = 3600 * 9 * (3 * 32 + 32 * 32 + 32 * 64)
    for b in block_shapes()[1:17]:
        hw, hw2, c = b['hin'] ** 2, b['hout'] ** 2, b['C']
        mac += hw * b['cin'] * c                        # conv1
        mac += hw * 9 * (c // 2) * 2 * c                # conv2.conv, two groups
        mac += c * b['inter'] + b['inter'] * 2 * c      # fc1, fc2 on the 1x1 map
        mac += hw2 * c * 4 * c                          # conv3
        if b['down']:
            mac += hw2 * b['cin'] * 4 * c
    return mac + 2048 * 62


def _t(sd, key, dtype):
    v = sd[key]
    v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
    return v.to(dtype)


def _bn(sd, y, bn, dtype):
    """y * scale + shift with scale = gamma / sqrt(var + 1e-5), shift = beta - mean * scale"""
    g, b = _t(sd, bn + '.weight', dtype), _t(sd, bn + '.bias', dtype)
    m, v = _t(sd, bn + '.running_mean', dtype), _t(sd, bn + '.running_var', dtype)
    scale = g / torch.sqrt(v + 1e-5)
    shift = b - m * scale
    return y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)


def _conv_bn(sd, x, conv, bn, stride, pad, groups, relu, dtype):
    y = _bn(sd, F.conv2d(x, _t(sd, conv + '.weight', dtype), None, stride, pad, 1, groups), bn, dtype)
    return torch.relu(y) if relu else y


def _bottleneck(sd, x, blk, dtype, avd_real_count=False, down_div4=False):
    """One bottleneck on NCHW x -> (output, attention [B,2C] in fc2's order).  avd_real_count / down_div4 are the two WRONG border rules
    a port could take (the avd pool dividing by the samples inside, the downsample pool dividing by 4 everywhere): test_resnest_cpu.py
    shows that either moves the output of layer3.0 far beyond TOL."""
    key, cin, c, inter, avd, down = blk
    B = x.shape[0]
    y = _conv_bn(sd, x, key + '.conv1', key + '.bn1', 1, 0, 1, True, dtype)
    u = _conv_bn(sd, y, key + '.conv2.conv', key + '.conv2.bn0', 1, 1, 2, True, dtype)
    gap = (u[:, :c] + u[:, c:]).mean(dim=(2, 3), keepdim=True)
    g = F.conv2d(gap, _t(sd, key + '.conv2.fc1.weight', dtype), _t(sd, key + '.conv2.fc1.bias', dtype))
    g = torch.relu(_bn(sd, g, key + '.conv2.bn1', dtype))
    z = F.conv2d(g, _t(sd, key + '.conv2.fc2.weight', dtype), _t(sd, key + '.conv2.fc2.bias', dtype)).view(B, 2, c)
    att = torch.softmax(z, dim=1)                               # cardinality 1: across the two radix halves
    v = att[:, 0].view(B, c, 1, 1) * u[:, :c] + att[:, 1].view(B, c, 1, 1) * u[:, c:]
    if avd:
        v = F.avg_pool2d(v, 3, 2, 1, count_include_pad=not avd_real_count)
    o = _conv_bn(sd, v, key + '.conv3', key + '.bn3', 1, 0, 1, False, dtype)
    r = x
    if down:
        if avd:
            if down_div4:
                r = F.avg_pool2d(F.pad(r, (0, r.shape[3] % 2, 0, r.shape[2] % 2)), 2, 2)
            else:
                r = F.avg_pool2d(r, 2, 2, ceil_mode=True, count_include_pad=False)
        r = _conv_bn(sd, r, key + '.downsample.1', key + '.downsample.2', 1, 0, 1, False, dtype)
    return torch.relu(o + r), att.reshape(B, 2 * c)


def _stem(sd, x, dtype):
    y = _conv_bn(sd, x, 'conv1.0', 'conv1.1', 2, 1, 1, True, dtype)
    y = _conv_bn(sd, y, 'conv1.3', 'conv1.4', 1, 1, 1, True, dtype)
    y = _conv_bn(sd, y, 'conv1.6', 'bn1', 1, 1, 1, True, dtype)
    return F.max_pool2d(y, 3, 2, 1)


def _tail(sd, y, dtype):
    """[B,2048,4,4] -> (out62, pool2048)"""
    pool = y.mean(dim=(2, 3))
    out = torch.cat([pool @ _t(sd, n + '.weight', dtype).t() + _t(sd, n + '.bias', dtype) for n in HEADS62], dim=1)
    return out, pool


def resnest_forward(sd, x, dtype=torch.float32, details=False):
    """sd: state_dict (numpy or torch, reference key names, no prefix); x: [B,3,120,120] normalised crops.  Returns (out62 [B,62] = ori |
    shape | exp, pool [B,2048]) as numpy; with details also (block outputs: 17 NCHW arrays, the stem + max pool and the 16 bottlenecks;
    attentions: 16 arrays [B,2C])."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    outs, atts = [], []
    with torch.no_grad():
        y = _stem(sd, x, dtype)
        outs.append(y.numpy())
        for blk in BLOCKS:
            y, a = _bottleneck(sd, y, blk, dtype)
            outs.append(y.numpy())
            atts.append(a.numpy())
        assert y.shape[1:] == (2048, 4, 4)
        out, pool = _tail(sd, y, dtype)
    if details:
        return out.numpy(), pool.numpy(), outs, atts
    return out.numpy(), pool.numpy()


def block_reference(sd, block, x_nhwc, dtype=torch.float64, **wrong):
    """The hook's block (syn_resnest50_block) on NHWC input, in `dtype`: (out NHWC -- [B,62] for block 17 --, aux or None) as numpy:
    aux = the attention [B,2C] of a bottleneck, the pool [B,2048] of block 17."""
    x = torch.as_tensor(np.asarray(x_nhwc)).to(dtype).permute(0, 3, 1, 2)
    with torch.no_grad():
        if block == 0:
            return _stem(sd, x, dtype).permute(0, 2, 3, 1).contiguous().numpy(), None
        if block <= 16:
            y, a = _bottleneck(sd, x, BLOCKS[block - 1], dtype, **wrong)
            return y.permute(0, 2, 3, 1).contiguous().numpy(), a.numpy()
        out, pool = _tail(sd, x, dtype)
        return out.numpy(), pool.numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# One block at a time, every element judged (tests/test_gpu_resnest_blocks.py): the integer probe, its conditions, the one-place
# mistakes the probe or the bound has to see, the elementwise fp32 bound of a block, and the fused tail's grid rule.  Shared machinery:
# tests/exact_probe.py.  Hook blocks: 0 stem + max pool, 1..16 bottlenecks, 17 pool + heads.
# ---------------------------------------------------------------------------------------------------------------------------------
import exact_probe as ep          # noqa: E402

PROBE_SEED = 20263
N_FACES = ep.N_FACES
TAIL = 17
HEADS = HEADS62 + ('fc_tex',)
GATE_DOMINANT = 4096               # one weight of every fc1 filter and of every fc2 row pair is that large (see make_integer_state)
EXP_ZERO = 104.0                   # exp(float32(-104)) == 0 (asserted in tests/test_resnest_cpu.py): beyond it the softmax is exactly (1, 0)
NINE_RANGE = 1864135               # float32(9 k) * (float32(1) / float32(9)) == k for every integer k up to here (asserted there too)
# Value sets of the probe by group width C: (face offsets, pixel steps, conv weights, every ReLU channel of conv1 / conv2 clamped).  An
# input element is offset[face, channel] + step[face, y, x, channel]: the channel means -- what the gate sees -- then differ between the
# faces as much as the pixels within one.  The wide sets of the other families do not fit behind the factor 9 of the avd pool.
WIDE = ((-2, -1, 0, 1, 2), (-1, 0, 1), (-2, -1, 1, 2), False)
NARROW = ((-1, 0, 1), (-1, 0, 1), (-1, 1), True)
SETS = {64: WIDE, 128: NARROW, 256: NARROW, 512: NARROW}
GSET = (1, -1)                     # BN weights: the chain conv1 -> conv2 -> 9 x -> conv3 leaves no room for denominators
STEM_KEYS = (('conv1.0', 'conv1.1', 2), ('conv1.3', 'conv1.4', 1), ('conv1.6', 'bn1', 1))


def hook_counts(block):
    """per-face shapes (in, out, aux or None) of a hook block"""
    s = block_shapes()[block]
    f_in = (s['hin'], s['hin'], s['cin'])
    return f_in, ((62,) if block == TAIL else (s['hout'], s['hout'], s['cout'])), ((s['aux'],) if s['aux'] else None)


def integer_faces(block, n=N_FACES, seed=PROBE_SEED):
    """The n distinct faces of a block's probe, NHWC.  Block 0: normalised crops, (x - 127.5) / 128 of uint8 x over the full range.  Block 17:
    integers in [-3, 3], and no pooled feature is 0 (a 4x4 sum that came out 0 has its first pixel moved by one).  Bottlenecks: see SETS."""
    rng = np.random.default_rng([seed, block, n])
    if block == 0:
        return np.ascontiguousarray(normalize_u8(rng.integers(0, 256, size=(n, 120, 120, 3), dtype=np.uint8)).transpose(0, 2, 3, 1))
    if block == TAIL:
        x = rng.integers(-3, 4, size=(n, 4, 4, 2048)).astype(np.float32)
        dead = x.sum(axis=(1, 2)) == 0
        x[:, 0, 0, :] += np.where(dead, np.where(x[:, 0, 0, :] < 3, 1, -1), 0).astype(np.float32)
        return x
    (h, _, c), (off, step, _, _) = hook_counts(block)[0], SETS[BLOCKS[block - 1][2]]
    return (rng.choice(np.asarray(off), size=(n, 1, 1, c)) + rng.choice(np.asarray(step), size=(n, h, h, c))).astype(np.float32)


def integer_input(block, B):
    """a probe batch: slot i holds distinct face exact_probe.batch_index(B)[i]"""
    return np.ascontiguousarray(integer_faces(block)[ep.batch_index(B)])


def _fold(sd, bn, dtype):
    g, b = _t(sd, bn + '.weight', dtype), _t(sd, bn + '.bias', dtype)
    m, v = _t(sd, bn + '.running_mean', dtype), _t(sd, bn + '.running_var', dtype)
    scale = g / torch.sqrt(v + 1e-5)
    return scale, b - m * scale


def _gate_z(sd, key, gap, dtype, drop_fc1_bias=False):
    """fc1 + bn1 + ReLU + fc2 on gap [B,C] -> z [B,2C]"""
    g = gap @ _t(sd, key + '.conv2.fc1.weight', dtype).flatten(1).t()
    if not drop_fc1_bias:
        g = g + _t(sd, key + '.conv2.fc1.bias', dtype)
    scale, shift = _fold(sd, key + '.conv2.bn1', dtype)
    return torch.relu(g * scale + shift) @ _t(sd, key + '.conv2.fc2.weight', dtype).flatten(1).t() + _t(sd, key + '.conv2.fc2.bias', dtype)


# ---- the mistakes a port could make, each confined to ONE place of one block ---------------------------------------------------------
# The probe sees (its float64 reference changes, so the equality on the GPU fails):
#   avd_real_count  the avd pool divides by the samples inside the map (the flag of _bottleneck)
#   down_div4       the downsample pool divides by 4 at the odd map's last row and column (the flag of _bottleneck)
#   att_swap        the two radix halves of the attention swapped where it multiplies U
#   softmax_adjacent the softmax over the adjacent pairs (z[2i], z[2i + 1]) instead of the halves (z[c], z[C + c])
#   att_face        the attention of the next face of the batch
#   res_face        the residual of the next face of the batch
#   avd_start       the avd window's rows start at 2 oy instead of 2 oy - 1
#   ds_clamped      the downsample pool adds the clamped sample for a tap past the odd map's edge (the divisor stays right)
#   group_slice     conv2's second group reads the first group's input slice
#   tap             conv2's centre tap of output pixel (1, 1) read one pixel to the right
# A saturated gate hides a wrong gate INPUT by design; these the bound of the attention sees on the gaussian checkpoint:
#   gap_first       the gap from U[:, :C] only
#   gap_last_pixel  the gap without its last pixel
#   gap_div_hout    the gap divided by hout^2 instead of hin^2 (avd blocks)
#   fc1_bias        fc1's bias dropped
PROBE_VARIANTS = ('avd_real_count', 'down_div4', 'att_swap', 'softmax_adjacent', 'att_face', 'res_face', 'avd_start', 'ds_clamped',
                  'group_slice', 'tap')
BOUND_VARIANTS = ('gap_first', 'gap_last_pixel', 'gap_div_hout', 'fc1_bias')
VARIANTS = PROBE_VARIANTS + BOUND_VARIANTS


def variants_of(block):
    """the VARIANTS that exist on a hook block"""
    if not 0 < block < TAIL:
        return ()
    s = block_shapes()[block]
    odd = s['avd'] and s['hin'] % 2 == 1
    only = {'avd_real_count': s['avd'], 'avd_start': s['avd'], 'gap_div_hout': s['avd'], 'down_div4': odd, 'ds_clamped': odd}
    return tuple(v for v in VARIANTS if only.get(v, True))


def _bottleneck_staged(sd, x, blk, dtype, variant=None, att=None):
    """_bottleneck stage by stage -> (output, attention [B,2C]), with one of VARIANTS applied and / or the attention GIVEN ([B,2C]: the
    tail that follows the gate is then judged apart from it)."""
    key, cin, c, inter, avd, down = blk
    assert variant is None or variant in VARIANTS
    B, H = x.shape[0], x.shape[2]
    y = _conv_bn(sd, x, key + '.conv1', key + '.bn1', 1, 0, 1, True, dtype)
    w2 = _t(sd, key + '.conv2.conv.weight', dtype)
    u = F.conv2d(y, w2, None, 1, 1, 1, 2)
    if variant == 'group_slice':
        u[:, c:] = F.conv2d(y[:, :c // 2], w2[c:], None, 1, 1)
    if variant == 'tap':
        for g in range(2):
            ys = y[:, g * (c // 2):(g + 1) * (c // 2)]
            u[:, g * c:(g + 1) * c, 1, 1] += (ys[:, :, 1, 2] - ys[:, :, 1, 1]) @ w2[g * c:(g + 1) * c, :, 1, 1].t()
    u = torch.relu(_bn(sd, u, key + '.conv2.bn0', dtype))
    if att is None:
        s = u[:, :c] if variant == 'gap_first' else u[:, :c] + u[:, c:]
        gap = s.mean(dim=(2, 3))
        if variant == 'gap_last_pixel':
            gap = (s.sum(dim=(2, 3)) - s[:, :, -1, -1]) / (H * H)
        if variant == 'gap_div_hout':
            gap = s.sum(dim=(2, 3)) / ((H + 1) // 2) ** 2
        z = _gate_z(sd, key, gap, dtype, drop_fc1_bias=variant == 'fc1_bias')
        a = (torch.softmax(z.view(B, c, 2), dim=2) if variant == 'softmax_adjacent' else torch.softmax(z.view(B, 2, c), dim=1)).reshape(B, 2 * c)
    else:
        a = torch.as_tensor(np.asarray(att)).to(dtype)
    use = a
    if variant == 'att_swap':
        use = torch.cat([a[:, c:], a[:, :c]], dim=1)
    if variant == 'att_face':
        use = torch.roll(a, -1, dims=0)
    v = use[:, :c].reshape(B, c, 1, 1) * u[:, :c] + use[:, c:].reshape(B, c, 1, 1) * u[:, c:]
    if avd:
        if variant == 'avd_start':
            v = F.avg_pool2d(F.pad(v, (1, 1, 0, 2)), 3, 2, 0)
        else:
            v = F.avg_pool2d(v, 3, 2, 1, count_include_pad=variant != 'avd_real_count')
    o = _conv_bn(sd, v, key + '.conv3', key + '.bn3', 1, 0, 1, False, dtype)
    r = x
    if down:
        if avd and variant == 'down_div4':
            r = F.avg_pool2d(F.pad(r, (0, H % 2, 0, H % 2)), 2, 2)
        elif avd and variant == 'ds_clamped':
            inside = F.avg_pool2d(F.pad(torch.ones(1, 1, H, H, dtype=dtype), (0, H % 2, 0, H % 2)), 2, 2)      # samples inside / 4
            r = F.avg_pool2d(F.pad(r, (0, H % 2, 0, H % 2), mode='replicate'), 2, 2) / inside
        elif avd:
            r = F.avg_pool2d(r, 2, 2, ceil_mode=True, count_include_pad=False)
        r = _conv_bn(sd, r, key + '.downsample.1', key + '.downsample.2', 1, 0, 1, False, dtype)
    if variant == 'res_face':
        r = torch.roll(r, -1, dims=0)
    return torch.relu(o + r), a


def probe_reference(sd, block, x, dtype=torch.float64, variant=None, att=None):
    """block_reference (NHWC in and out, numpy) with one of VARIANTS applied or the attention given"""
    if not 0 < block < TAIL or (variant is None and att is None):
        return block_reference(sd, block, x, dtype)
    if variant in ('avd_real_count', 'down_div4') and att is None:
        return block_reference(sd, block, x, dtype, **{variant: True})
    with torch.no_grad():
        xin = torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2)
        y, a = _bottleneck_staged(sd, xin, BLOCKS[block - 1], dtype, variant, att)
        return y.permute(0, 2, 3, 1).contiguous().numpy(), a.numpy()


variant_reference = probe_reference          # the name the BasicBlock family uses


def heads_reference(sd, pool, dtype=torch.float64):
    """[B,62] = ori | shape | exp of a given pool [B,2048]"""
    return ep.heads_pair(sd, HEADS62, pool)[0].to(dtype).numpy()


def heads_bound(sd, pool):
    """(C + 2) u (sum |W||pool| + |b|) of the 62 outputs on a GIVEN pool"""
    return ep.heads_pair(sd, HEADS62, pool)[1].numpy()


# ---- the fp32 bound of a block --------------------------------------------------------------------------------------------------------
def _u_pair(sd, blk, x):
    """(U, bound of U): conv1 + ReLU, the grouped conv2 + ReLU; x NCHW float64"""
    key = blk[0]
    y, e = ep.relu_pair(*ep.conv_bn_pair(sd, key + '.conv1', key + '.bn1', x, None, 1, 0, 1))
    return ep.relu_pair(*ep.conv_bn_pair(sd, key + '.conv2.conv', key + '.conv2.bn0', y, e, 1, 1, 2))


def _hidden_pair(sd, key, gap, eg):
    """fc1 with bn1 folded on gap [B,C], before the ReLU: the shift is folded from fc1's bias, beta and the mean"""
    sc, shift, shift_abs = ep.fold64(sd, key + '.conv2.bn1')
    w1, b1 = ep.t64(sd, key + '.conv2.fc1.weight').flatten(1), ep.t64(sd, key + '.conv2.fc1.bias')
    return ep.affine_pair(w1 * sc.view(-1, 1), b1 * sc + shift, (b1 * sc).abs() + shift_abs, gap, eg)


def _gate_pair(sd, blk, u, eu, exact_sums=False):
    """(att [B,2C], its bound, z [B,2C], its bound) by the rules of exact_probe: U0 + U1, the mean over HW, fc1 with bn1 folded (its
    shift is folded from fc1's bias, beta and the mean: three terms that round before they cancel), ReLU, fc2, the two-way softmax.
    eu = None: U given exactly.  exact_sums: U holds integers and no face's sum of |U0 + U1| over the pixels reaches 2^24 (asserted
    here), so every partial sum of the gap is an fp32 number in any order and only the reciprocal of HW and the product with it round:
    2 u |gap|, one u to spare."""
    key, cin, c, inter, avd, down = blk
    e0, e1 = (None, None) if eu is None else (eu[:, :c], eu[:, c:])
    if exact_sums:
        s = u[:, :c] + u[:, c:]
        assert eu is None and ep.is_multiple(u, 0) and float(s.abs().sum(dim=(2, 3)).max()) < 2.0 ** 24
        gap = s.mean(dim=(2, 3))
        eg = 3 * ep.U * gap.abs()
    else:
        gap, eg = ep.mean_pair(*ep.add_pair(u[:, :c], e0, u[:, c:], e1))
    h, eh = _hidden_pair(sd, key, gap, eg)
    z, ez = ep.bias_conv_pair(sd, key + '.conv2.fc2', torch.relu(h), eh)
    a0, b0, a1, b1_ = ep.softmax2_pair(z[:, :c], ez[:, :c], z[:, c:], ez[:, c:])
    return torch.cat([a0, a1], dim=1), torch.cat([b0, b1_], dim=1), z, ez


def _tail_pair(sd, blk, x, u, eu, att, e_att):
    """(output, bound) of what follows the gate: the combination with the attention `att` (e_att = None: given exactly), the avd pool,
    conv3, the downsample branch, the add, ReLU"""
    key, cin, c, inter, avd, down = blk
    parts = []
    for h in (0, 1):
        sl = slice(h * c, (h + 1) * c)
        v, e = ep.gated_pair(u[:, sl], None if eu is None else eu[:, sl], att[:, sl])
        if e_att is not None:
            e = e + u[:, sl].abs() * e_att[:, sl].view(e_att.shape[0], -1, 1, 1)
        parts += [v, e]
    v, e = ep.add_pair(*parts)
    if avd:
        v, e = ep.avg_pool_pair(v, e, 3, 2, 1)
    o, eo = ep.conv_bn_pair(sd, key + '.conv3', key + '.bn3', v, e, 1, 0, 1)
    r, er = x, None
    if down:
        if avd:
            r, er = ep.avg_pool_pair(x, None, 2, 2, 0, ceil_mode=True, count_include_pad=False)
        r, er = ep.conv_bn_pair(sd, key + '.downsample.1', key + '.downsample.2', r, er, 1, 0, 1)
    return ep.relu_pair(*ep.add_pair(o, eo, r, er))


def block_bound(sd, block, x, att=None):
    """Elementwise bound of |got - probe_reference(float64)| for fp32 arithmetic on the fp32 input x -> (bound of out, bound of aux or
    None), in the layouts of probe_reference.  The hook returns no intermediate but the attention, so the bound is carried through the
    stages (exact_probe).  Block 0: three convolutions, the largest bound of the max pool's window.  Bottlenecks: the attention's own
    bound (U0 + U1, mean, fc1 + bn1, ReLU, fc2, softmax, behind the bound of U); with `att` GIVEN the output's bound is that of the tail
    behind the gate on that attention -- against probe_reference(att=att) --, else the attention's bound enters through |U| e_att.
    Block 17: the pool's bound (the 16-term mean); the heads are judged on the returned pool (heads_reference / heads_bound), so out's
    bound is None."""
    f = ep.F64
    x = torch.as_tensor(np.asarray(x)).to(f).permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().numpy()
    with torch.no_grad():
        if block == 0:
            a, e = x, None
            for conv, bn, stride in STEM_KEYS:
                a, e = ep.relu_pair(*ep.conv_bn_pair(sd, conv, bn, a, e, stride, 1, 1))
            return nhwc(ep.max_pool_pair(a, e, 3, 2, 1)[1]), None
        if block == TAIL:
            return None, ep.mean_pair(x, None)[1].numpy()
        blk = BLOCKS[block - 1]
        u, eu = _u_pair(sd, blk, x)
        a, ea, _, _ = _gate_pair(sd, blk, u, eu)
        if att is not None:
            out = _tail_pair(sd, blk, x, u, eu, torch.as_tensor(np.asarray(att)).to(f), None)
        else:
            out = _tail_pair(sd, blk, x, u, eu, a, ea)
        return nhwc(out[1]), ea.numpy()


def judge(sd, block, x, out, aux):
    """[(part, max err / bound)] of a hook block's results (numpy) on the fp32 input x against the float64 reference.  A bottleneck: the
    attention under its own bound, the output against the float64 tail that uses the RETURNED attention (which isolates the gate from
    the convolutions).  Block 17: the pool under its bound, the heads on the returned pool."""
    results = {'out': out, 'aux': aux}
    return [(name, ep.bound_ratio(results[which], ref, bound)) for name, which, ref, bound in judge_parts(sd, block, x, aux)]


def judge_parts(sd, block, x, aux):
    """[(part, 'out' | 'aux', float64 reference, bound)] that judge holds a block's results against; they depend on the results only
    through the returned aux"""
    if block == 0:
        return [('out', 'out', probe_reference(sd, 0, x)[0], block_bound(sd, 0, x)[0])]
    if block == TAIL:
        return [('pool', 'aux', probe_reference(sd, TAIL, x)[1], block_bound(sd, TAIL, x)[1]),
                ('heads', 'out', heads_reference(sd, aux), heads_bound(sd, aux))]
    b_out, b_att = block_bound(sd, block, x, att=aux)
    return [('att', 'aux', probe_reference(sd, block, x)[1], b_att), ('out', 'out', probe_reference(sd, block, x, att=aux)[0], b_out)]


# ---- the probe's weights ----------------------------------------------------------------------------------------------------------------
_INT_STATE = {}


def _half_channels(sd, key, c):
    """[C] bool: the channels whose two fc2 rows and biases are identical (attention exactly 0.5 / 0.5)"""
    w, b = np.asarray(sd[key + '.conv2.fc2.weight']).reshape(2 * c, -1), np.asarray(sd[key + '.conv2.fc2.bias'])
    return (w[:c] == w[c:]).all(axis=1) & (b[:c] == b[c:])


def _probe_gate(rng, sd, blk, u):
    """Draws fc1 / bn1 / fc2 of one bottleneck into sd and returns the attention [8,2C] of the distinct faces, which is exact by design.
    The gate's arithmetic rounds (the mean of 900 or 225 pixels does), so its two outputs per channel are made to survive any rounding:
      * a quarter of the channels has identical fc2 rows and biases in both halves: z0 == z1 bit for bit, attention 0.5 / 0.5;
      * the others are saturated: fc1 (weights +-1, integer bias in [-3, 3], bn1 weight +-1 and the bias of a ReLU stage) and fc2 (+-1)
        each carry one weight GATE_DOMINANT times the others on an input that separates the faces well (exact_probe.separating), with
        opposite signs in fc2's two halves; per channel the 8 differences z0 - z1 are sorted, a wide gap with 2 .. 6 faces below it is
        taken (of the wide ones the gap that parts the pair of faces parted least so far) and fc2's bias of the first half puts its
        middle at 0.  Then |z0 - z1| > EXP_ZERO by far more than rounding can move it
        (exactness_violations), expf(z - max) is exactly 0 on one side, and which side depends on the face."""
    key, cin, c, inter, avd, down = blk
    f32 = np.float32
    gap, eg = ep.mean_pair(*ep.add_pair(u[:, :c], None, u[:, c:], None))
    w1 = rng.choice(np.asarray((-1, 1), f32), size=(inter, c, 1, 1))
    w1[np.arange(inter), ep.separating(rng, gap, eg, inter)] *= GATE_DOMINANT
    bn = key + '.conv2.bn1'
    sd[key + '.conv2.fc1.weight'], sd[key + '.conv2.fc1.bias'] = w1, rng.integers(-3, 4, size=inter).astype(f32)
    sd[bn + '.weight'], sd[bn + '.running_mean'] = rng.choice(np.asarray(GSET, f32), size=inter), np.zeros(inter, f32)
    sd[bn + '.running_var'], sd[bn + '.num_batches_tracked'] = np.full(inter, ep.V_STAR, f32), np.array(1000, dtype=np.int64)
    pre = (gap @ _t(sd, key + '.conv2.fc1.weight', ep.F64).flatten(1).t() + _t(sd, key + '.conv2.fc1.bias', ep.F64)) * _t(sd, bn + '.weight', ep.F64)
    sd[bn + '.bias'] = ep.relu_bias(rng, pre.view(pre.shape[0], -1, 1, 1), per_face=False).astype(f32)
    h, eh = _hidden_pair(ep.reference_state({k: v for k, v in sd.items() if k.startswith(key + '.conv2.')}), key, gap, eg)
    h = torch.relu(h)
    w2 = rng.choice(np.asarray((-1, 1), f32), size=(2 * c, inter, 1, 1))
    rows, j = np.arange(c), ep.separating(rng, h, eh, c)
    w2[rows, j] *= GATE_DOMINANT
    w2[c + rows, j] = -w2[rows, j]
    half = rng.permutation(c)[:c // 4]
    w2[c + half] = w2[half]
    b2 = np.zeros(2 * c, f32)
    sd[key + '.conv2.fc2.weight'], sd[key + '.conv2.fc2.bias'] = w2, b2
    z, ez = (t.numpy() for t in ep.bias_conv_pair(sd, key + '.conv2.fc2', h, eh))
    d, ed = z[:, :c] - z[:, c:], ez[:, :c] + ez[:, c:] + ep.U * np.abs(z[:, :c] - z[:, c:])
    v = np.sort(d, axis=0)
    gaps = v[2:7] - v[1:6]                                                               # 2 .. 6 faces below the gap
    wide = gaps / 2 - EXP_ZERO > 400 * ed.max(axis=0)                                    # four times the margin asked for
    wide[gaps.argmax(axis=0), rows] = True
    split, pairs = np.zeros((N_FACES, N_FACES)), np.triu_indices(N_FACES, 1)             # channels so far in which two faces take different sides
    for ch in np.setdiff1d(rng.permutation(c), half, assume_unique=True):                # of the wide gaps the one that parts the least parted faces
        best = None
        for at in np.flatnonzero(wide[:, ch]) + 1:
            side = d[:, ch] > (v[at, ch] + v[at + 1, ch]) / 2
            new = split + (side[:, None] != side[None, :])
            score = tuple(np.sort(new[pairs])[:4]) + (rng.random(),)
            if best is None or score > best[0]:
                best = (score, at, new)
        _, at, split = best
        b2[ch] = -np.rint((v[at, ch] + v[at + 1, ch]) / 2)
    b2[half] = b2[c + half] = rng.integers(-3, 4, size=half.size)
    a0 = (d + b2[:c].astype(np.float64) > 0).astype(np.float64)
    a0[:, half] = 0.5
    return torch.from_numpy(np.concatenate([a0, 1.0 - a0], axis=1))


def make_integer_state(seed=PROBE_SEED):
    """A state_dict on which every hook block is exact in fp32 on integer_faces(block).  Convolutions: weights by group width (SETS: {-2, -1,
    1, 2} for C = 64, {-1, 1} above and in the stem), running_mean 0, running_var V_STAR, BN weight +-1, integer biases -- in front of
    a ReLU by the rule of exact_probe.probe_conv_bn on the 8 distinct faces (conv3's on conv3 + residual; with the narrow sets, in the stem
    and on conv2.bn0 of the avd blocks every channel is clamped by 30 .. 70 %, which halves what the next stage has to add), from
    [-3, 3] on the downsample.  layer2.0 / 3.0 / 4.0: conv2.bn0's weight and bias are 9 times that, so U, and with a 0.5 / 0.5 gate 2 U,
    is a multiple of 9 and the avd pool's product with fl(1 / 9) is exact (NINE_RANGE).  The gate: _probe_gate.  Heads: weights {-2, -1,
    1, 2}, integer biases in [-8, 8]."""
    if seed in _INT_STATE:
        return _INT_STATE[seed]
    rng = np.random.default_rng(seed)
    sd, f = {}, ep.F64
    faces = lambda b: torch.from_numpy(integer_faces(b)).to(f).permute(0, 3, 1, 2)
    with torch.no_grad():
        a = faces(0)
        for (conv, bn, stride), shape in zip(STEM_KEYS, ((32, 3, 3, 3), (32, 32, 3, 3), (64, 32, 3, 3))):
            a = ep.probe_conv_bn(rng, sd, conv, bn, shape, a, stride, 1, 1, (-1, 1), GSET, clamp_all=True)
        for i, blk in enumerate(BLOCKS, start=1):
            key, cin, c, inter, avd, down = blk
            w, clamp = SETS[c][2:]
            x = faces(i)
            y = ep.probe_conv_bn(rng, sd, key + '.conv1', key + '.bn1', (c, cin, 1, 1), x, 1, 0, 1, w, GSET, clamp_all=clamp)
            u = ep.probe_conv_bn(rng, sd, key + '.conv2.conv', key + '.conv2.bn0', (2 * c, c // 2, 3, 3), y, 1, 1, 2, w, GSET, clamp_all=clamp or avd)
            if avd:
                sd[key + '.conv2.bn0.weight'], sd[key + '.conv2.bn0.bias'], u = 9 * sd[key + '.conv2.bn0.weight'], 9 * sd[key + '.conv2.bn0.bias'], 9 * u
            att = _probe_gate(rng, sd, blk, u)
            v = att[:, :c].reshape(N_FACES, c, 1, 1) * u[:, :c] + att[:, c:].reshape(N_FACES, c, 1, 1) * u[:, c:]
            r = x
            if avd:
                v, r = F.avg_pool2d(v, 3, 2, 1), F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)
            if down:
                r = ep.probe_conv_bn(rng, sd, key + '.downsample.1', key + '.downsample.2', (4 * c, cin, 1, 1), r, 1, 0, 1, w, GSET, relu=False)
            ep.probe_conv_bn(rng, sd, key + '.conv3', key + '.bn3', (4 * c, c, 1, 1), v, 1, 0, 1, w, GSET, add=r)
    for name, n in zip(HEADS, (12, 40, 10, 40)):
        sd[name + '.weight'] = rng.choice(np.asarray((-2, -1, 1, 2), np.float32), size=(n, 2048))
        sd[name + '.bias'] = rng.integers(-8, 9, size=n).astype(np.float32)
    _INT_STATE[seed] = sd
    return sd


# ---- the gate on its own: the probe's convolutions in front of an ordinary gate -----------------------------------------------------------
# On the gaussian checkpoint the attention's bound has to carry the worst case of conv1 and conv2 through sum |w| e of two dense layers,
# which leaves it between 0.02 (layer1.0) and 46 (layer4.2) for a number in (0, 1): it holds, and judges nothing.  The hook returns no U,
# so the gate is isolated from the other side: make_gate_state keeps every convolution of the integer state -- U is then an fp32 number
# that every summation order reproduces, which the integer probe verifies on the device through the block's output -- and draws fc1 / bn1 /
# fc2 as an ordinary checkpoint has them.  The attention's bound then starts at an exact U (gate_reference) and is the gate's own
# arithmetic, 1e-6 .. 1e-4; a wrong gate INPUT (BOUND_VARIANTS), which the saturated probe hides by design, shows against it.
_GATE_STATE = {}


def make_gate_state(seed=PROBE_SEED):
    """The integer state with fc1 / bn1 / fc2 of every bottleneck redrawn: gaussian weights scaled to the gap's size on integer_faces, so
    that the pre-activations are of order 1 and the attention lies inside (0, 1) and differs between the faces; biases, BN weight, bias,
    running_mean and running_var are all non-trivial, so the fold of bn1 with fc1's bias is exercised too."""
    if seed in _GATE_STATE:
        return _GATE_STATE[seed]
    rng = np.random.default_rng([seed, 1])
    sd, ref, f32 = dict(make_integer_state(seed)), ep.reference_state(make_integer_state(seed)), np.float32
    with torch.no_grad():
        for i, (key, cin, c, inter, avd, down) in enumerate(BLOCKS, start=1):
            x = torch.from_numpy(integer_faces(i)).to(ep.F64).permute(0, 3, 1, 2)
            u = _conv_bn(ref, _conv_bn(ref, x, key + '.conv1', key + '.bn1', 1, 0, 1, True, ep.F64), key + '.conv2.conv', key + '.conv2.bn0', 1, 1, 2, True, ep.F64)
            gap = (u[:, :c] + u[:, c:]).mean(dim=(2, 3))
            spread = float((gap - gap.mean(dim=0)).pow(2).mean().sqrt())                 # what tells the faces apart
            g = key + '.conv2.'
            sd[g + 'fc1.weight'] = (rng.standard_normal((inter, c, 1, 1)) / (np.sqrt(c) * spread)).astype(f32)
            centre = (gap.mean(dim=0).numpy() @ sd[g + 'fc1.weight'].reshape(inter, c).T.astype(np.float64))
            sd[g + 'fc1.bias'] = (-centre + rng.standard_normal(inter)).astype(f32)      # the faces' common part taken out, a bias of the pre-activation's size left
            sd[g + 'bn1.weight'], sd[g + 'bn1.bias'] = rng.uniform(0.5, 1.5, inter).astype(f32), (0.3 * rng.standard_normal(inter)).astype(f32)
            sd[g + 'bn1.running_mean'], sd[g + 'bn1.running_var'] = (0.3 * rng.standard_normal(inter)).astype(f32), rng.uniform(0.5, 1.5, inter).astype(f32)
            sd[g + 'fc2.weight'] = (rng.standard_normal((2 * c, inter, 1, 1)) * (1.5 / np.sqrt(inter))).astype(f32)
            sd[g + 'fc2.bias'] = (0.5 * rng.standard_normal(2 * c)).astype(f32)
    _GATE_STATE[seed] = sd
    return sd


def gate_reference_state(sd):
    """exact_probe.reference_state for the gate state: only the probe's own running_var (V_STAR) gets its float64 counterpart"""
    return {k: (np.full(v.shape, ep.V_STAR64, np.float64) if k.endswith('running_var') and np.all(v == ep.V_STAR) else v) for k, v in sd.items()}


def gate_reference(sd_ref, block, x, variant=None):
    """(attention [B,2C] in float64, its elementwise fp32 bound from an EXACT U) of a bottleneck of the gate state on probe input x (NHWC);
    variant: one of BOUND_VARIANTS applied to the attention"""
    blk = BLOCKS[block - 1]
    with torch.no_grad():
        xin = torch.as_tensor(np.asarray(x)).to(ep.F64).permute(0, 3, 1, 2)
        key = blk[0]
        u = _conv_bn(sd_ref, _conv_bn(sd_ref, xin, key + '.conv1', key + '.bn1', 1, 0, 1, True, ep.F64), key + '.conv2.conv', key + '.conv2.bn0', 1, 1, 2, True, ep.F64)
        att, bound, _, _ = _gate_pair(sd_ref, blk, u, None, exact_sums=True)
        if variant is not None:
            assert variant in BOUND_VARIANTS
            att = _bottleneck_staged(sd_ref, xin, blk, ep.F64, variant)[1]
        return att.numpy(), bound.numpy()


# ---- the conditions under which the probe is exact ------------------------------------------------------------------------------------
GATE_MARGIN = {}                 # block -> smallest (|z0 - z1| - EXP_ZERO) / bound of z0 - z1 that exactness_violations has seen
MAGNITUDE = {}                     # stage -> largest 2^q x magnitude that exactness_violations has seen, for the record


def exactness_violations(block, x, sd_ref=None):
    """The conditions of the probe on the float64 trace of one hook block (x NHWC as probe_reference takes it); returns the list of
    violations, empty = all hold.  Every stage -- stem x 3, conv1, conv2, the combination, the avd pool's nine-term sum, the downsample
    pool and convolution, conv3 + residual, the mean of 16, the heads: the output is a multiple of 2^-q; 2^q x (the sum of the absolute
    values of all its terms) < 2^24, so every partial sum in any order, with or without FMA, is an fp32 number; the output is not
    constant; every ReLU map is partly clamped and has no dead channel.  The max pool: not constant, one window clamped throughout.
    q: 8 in the stem (the normalised pixel); 0 up to U; 1 behind a 0.5 gate; 2 behind the downsample pool and where its branch is added;
    4 behind the mean of 16.  avd blocks: U is a multiple of 9 and twice the nine-term sum is 9 k with k <= NINE_RANGE.  The odd map: the
    last row, the last column and the corner of every input face differ from their neighbours.  The gate, where rounding is allowed
    because nothing depends on it: a quarter of the channels has z0 == z1 by identical fc2 rows; on the others |z0 - z1| - EXP_ZERO >
    100 x the fp32 bound of z0 - z1 (exact_probe's rules from an exact U: U0 + U1, mean, fc1 + bn1, ReLU, fc2, the subtraction); the
    attention is 0, 0.5 or 1; on the 8 distinct faces at least half of the saturated channels take both sides, and any two different
    faces differ in the side of at least one saturated channel in eight; neighbouring residuals of a batch differ."""
    sd = ep.reference_state(make_integer_state()) if sd_ref is None else sd_ref
    f, bad = ep.F64, []
    x = torch.as_tensor(np.asarray(x)).to(f).permute(0, 3, 1, 2)

    def check(name, y, mag, q, relu=False):
        MAGNITUDE[name.split(' ', 1)[-1]] = max(MAGNITUDE.get(name.split(' ', 1)[-1], 0.0), float(mag.max()) * 2.0 ** q)
        if not ep.is_multiple(y, q):
            bad.append(f'{name}: output is no multiple of 2^-{q}')
        if not float(mag.max()) * 2.0 ** q < 2.0 ** 24:
            bad.append(f'{name}: 2^{q} x magnitude = {float(mag.max()) * 2.0 ** q:.4g} >= 2^24')
        if float(y.min()) == float(y.max()):
            bad.append(f'{name}: constant output')
        if relu and not ep.relu_is_partly_clamped(y):
            bad.append(f'{name}: the ReLU map is not partly clamped, or a channel is dead')
        return y

    def stage(name, conv, bn, a, stride, pad, groups, relu, q, res=None):
        y = _conv_bn(sd, a, conv, bn, stride, pad, groups, False, f)
        mag = ep.conv_magnitude(sd, conv, bn, a, stride, pad, groups)
        if res is not None:
            y, mag = y + res, mag + res.abs()
        return check(name, torch.relu(y) if relu else y, mag, q, relu)

    with torch.no_grad():
        if block == 0:
            for i, (conv, bn, stride) in enumerate(STEM_KEYS):
                x = stage(f'stem stem{i + 1}', conv, bn, x, stride, 1, 1, True, 8)
            p = F.max_pool2d(x, 3, 2, 1)
            if float(p.min()) == float(p.max()) or not bool((p == 0).any()):
                bad.append('max pool: constant, or no window is clamped throughout')
            return bad
        if block == TAIL:
            pool = check('tail mean of 16', x.mean(dim=(2, 3)), x.abs().sum(dim=(2, 3)), 4)
            out, omag = ep.heads_pair(sd, HEADS62, pool)
            check('tail heads', out, omag / ((2048 + 2) * ep.U), 4)
            if bool((pool == 0).any()):
                bad.append('tail: a pooled feature is 0')
            return bad
        blk = BLOCKS[block - 1]
        key, cin, c, inter, avd, down = blk
        B, H = x.shape[0], x.shape[2]
        y = stage(key + ' conv1', key + '.conv1', key + '.bn1', x, 1, 0, 1, True, 0)
        u = stage(key + ' conv2', key + '.conv2.conv', key + '.conv2.bn0', y, 1, 1, 2, True, 0)
        if avd and not ep.is_multiple(u / 9, 0):
            bad.append(key + ' conv2: U is no multiple of 9')
        # the gate
        att, _, z, ez = _gate_pair(sd, blk, u, None)
        d = z[:, :c] - z[:, c:]
        ed = ez[:, :c] + ez[:, c:] + ep.U * d.abs()
        half = torch.from_numpy(_half_channels(sd, key, c))
        sat = ~half
        if not 0.2 <= float(half.double().mean()) <= 0.3:
            bad.append(f'{key} gate: {float(half.double().mean()):.2f} of the channels are 0.5 / 0.5')
        if not bool((d[:, half] == 0).all()):
            bad.append(key + ' gate: z0 != z1 on a 0.5 / 0.5 channel')
        margin = float(((d.abs() - EXP_ZERO) / ed)[:, sat].min())
        GATE_MARGIN[block] = min(GATE_MARGIN.get(block, np.inf), margin)
        if not margin > 100.0:
            bad.append(f'{key} gate: |z0 - z1| - {EXP_ZERO:g} is within 100 x the bound of z0 - z1 (smallest ratio {margin:.3g})')
        side = d > 0
        want = torch.where(half, torch.full_like(d, 0.5), side.to(f))
        if not bool(torch.equal(att, torch.cat([want, 1.0 - want], dim=1))):
            bad.append(key + ' gate: an attention is not the 0, 0.5 or 1 its channel was built for')
        distinct = [(i, j) for i in range(B) for j in range(i) if not bool((x[i] == x[j]).all())]
        if B == N_FACES and not float((side.any(dim=0) & ~side.all(dim=0))[sat].double().mean()) >= 0.5:
            bad.append(key + ' gate: fewer than half of the saturated channels take both sides')
        if any(float((side[i] != side[j])[sat].double().mean()) < 0.125 for i, j in distinct):
            bad.append(key + ' gate: two different faces share the side of more than 7 saturated channels in 8')
        # the tail
        a0, a1 = att[:, :c].reshape(B, c, 1, 1), att[:, c:].reshape(B, c, 1, 1)
        v = check(key + ' combine', a0 * u[:, :c] + a1 * u[:, c:], a0 * u[:, :c] + a1 * u[:, c:], 1)
        r = x
        if avd:
            s9 = check(key + ' avd sum', 9 * F.avg_pool2d(v, 3, 2, 1), 9 * F.avg_pool2d(v, 3, 2, 1), 1)
            k = 2 * s9 / 9
            if not (ep.is_multiple(k, 0) and float(k.max()) <= NINE_RANGE):
                bad.append(f'{key} avd sum: twice the sum is no 9 k with k <= {NINE_RANGE} (largest {float(k.max()):.4g})')
            v = s9 / 9
            r = check(key + ' downsample pool', F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False), 4 * F.avg_pool2d(x.abs(), 2, 2, ceil_mode=True), 2)
            if H % 2:
                e = x[:, :, -1, -1]
                differ = [(x[:, :, -1] != x[:, :, -2]), (x[:, :, :, -1] != x[:, :, :, -2])] + [(e != o).unsqueeze(2) for o in (x[:, :, -1, -2], x[:, :, -2, -1], x[:, :, -2, -2])]
                if not all(bool(t.flatten(1).any(dim=1).all()) for t in differ):
                    bad.append(key + ': the last row, the last column or the corner of a face equals its neighbour')
        if down:
            r = stage(key + ' downsample', key + '.downsample.1', key + '.downsample.2', r, 1, 0, 1, False, 2 if avd else 0)
        stage(key + ' conv3 + residual', key + '.conv3', key + '.bn3', v, 1, 0, 1, True, 2 if avd else 1, res=r)
        if any(bool((r[i] == r[i - 1]).all()) for i in range(1, B)):
            bad.append(key + ': neighbouring faces have the same residual')
    return bad


# ---- the fused tail's grid ---------------------------------------------------------------------------------------------------------------
TAIL_GROUPS = 1024


def tail_split(M, K, N):
    """The channel ranges (gridDim.y) of the fused tail on M output pixels, K operand channels and N output channels, restated from
    DESIGN 5.15: a workgroup owns 16 MT pixels (MT = 4 for K <= 128, 2 for 256, 1 for 512); while that gives fewer than 1024 workgroups
    the channels are halved, down to ranges of 128."""
    pt = 16 * (4 if K <= 128 else 2 if K == 256 else 1)
    groups, split = (M + pt - 1) // pt, 1
    while groups * split < TAIL_GROUPS and N // (2 * split) >= 128 and N % (256 * split) == 0:
        split *= 2
    return split


def block_tails(block):
    """[(operand, output pixels per face, K, N)] of the fused tail launches of a bottleneck: conv3's (combine, or avd on layer2.0 / 3.0 /
    4.0) and, where the pooled input fits the LDS tile (K <= 512), the downsample's behind its pool"""
    s = block_shapes()[block]
    tails = [('avd' if s['avd'] else 'combine', s['hout'] ** 2, s['C'], s['cout'])]
    if s['avd'] and s['cin'] <= 512:
        tails.append(('dspool', s['hout'] ** 2, s['cin'], s['cout']))
    return tails


def splits_at(block, B):
    return tuple(tail_split(B * hw, K, N) for _, hw, K, N in block_tails(block))


# (block key, batch, what the fused tail's grid is there).  Every batch runs fused; the largest of a block also per layer.
TAIL_CASES = [
    ('layer4.2', 127, 'combine, MT = 1: 127 workgroups, channels in 16 ranges of 128 (as at every smaller batch)'),
    ('layer4.2', 128, 'combine, MT = 1: 8 ranges'),
    ('layer4.2', 255, 'combine, MT = 1: the last batch with 8 ranges'),
    ('layer4.2', 256, 'combine, MT = 1: 4 ranges'),
    ('layer4.2', 511, 'combine, MT = 1: the last batch with 4 ranges'),
    ('layer4.2', 512, 'combine, MT = 1: 2 ranges'),
    ('layer4.2', 1023, 'combine, MT = 1: the last batch with 2 ranges'),
    ('layer4.2', 1024, 'combine, MT = 1: 1024 workgroups, one walks all 2048 channels'),
    ('layer3.0', 1, 'avd, MT = 2, and the downsample pool, MT = 1, 15 -> 8: both in 8 ranges of 128'),
    ('layer3.0', 255, 'downsample pool: the last batch with 2 ranges (avd: 4)'),
    ('layer3.0', 256, 'downsample pool: 1024 workgroups, unsplit (avd: 2)'),
    ('layer3.0', 511, 'avd: the last batch with 2 ranges'),
    ('layer3.0', 512, 'avd: 1024 workgroups, unsplit'),
    ('layer1.1', 72, 'combine, MT = 4, N = 256: 1013 workgroups of 64 pixels, 2 ranges'),
    ('layer1.1', 73, 'combine, MT = 4, N = 256: 1027 workgroups, unsplit'),
]
