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
