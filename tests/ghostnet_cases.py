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
