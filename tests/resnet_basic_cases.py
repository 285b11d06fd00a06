"""Test infrastructure of the BasicBlock ResNets (resnet18 / resnet34): a torch-functional restatement of the reference network
(backbone_nets/resnet_backbone.py:50-87 BasicBlock, :227-249 ResNet._forward_impl) with the BatchNorms folded, written against the
state_dict alone -- it shares nothing with the library's packing code (csrc/synergy_abi.hip pack_backbone_resnet_basic) -- plus the shapes,
seeds and inputs the CPU and GPU tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from mobilenet1_cases import border_crops, normalize_u8          # noqa: F401  (shared inputs)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'resnet_basic_outputs.npz')
ARCHS = ('resnet18', 'resnet34')
ARCH_ID = {'resnet18': 10, 'resnet34': 11}
LAYERS = {'resnet18': (2, 2, 2, 2), 'resnet34': (3, 4, 6, 3)}
SEED = 3187                 # weights of the golden file and of the GPU tests (synth.make_resnet_basic_state(arch, SEED))
CROPS_SEED = 53
TOL = 1e-4                  # the project's bar (TOL of tests/test_gpu_parity.py)
HEADS62 = ('fc_ori', 'fc_shape', 'fc_exp')      # the first 62 of the forward's cat (ori | shape | exp | tex)
FLAT_COUNT = {'resnet18': 11238438, 'resnet34': 21354022}
MAC_FORWARD = {'resnet18': 553011200, 'resnet34': 1129564160}      # as the issue states them, without fc_tex


def blocks(arch):
    """(key, in, out, stride, downsample) as the issue states the network: [2,2,2,2] / [3,4,6,3] BasicBlocks of 64 / 128 / 256 / 512
    channels, stride 2 and a 1x1 stride-2 downsample on layer2.0 / 3.0 / 4.0."""
    out, cin = [], 64
    for l, (c, count) in enumerate(zip((64, 128, 256, 512), LAYERS[arch])):
        for i in range(count):
            s = 2 if l > 0 and i == 0 else 1
            out.append((f'layer{l + 1}.{i}', cin, c, s, s == 2))
            cin = c
    return out


def golden_crops():
    """The 2 synthetic uint8 crops [2,120,120,3] of the golden file: synth.make_crops noise blended half and half with one plane wave per
    face and colour channel (as resnest_cases.golden_crops: pure noise is the same face twice after the global mean)."""
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


def block_shapes(arch):
    """Per hook block 0 .. last: dict(key, cin, cout, hin, hout, stride, down) -- in = [B,hin,hin,cin], out = [B,hout,hout,cout] NHWC
    (block 0: in = NCHW crops [B,3,120,120]; the last block: out = [B,62])."""
    out = [dict(key='stem', cin=3, cout=64, hin=120, hout=30, stride=4, down=False)]
    h = 30
    for key, cin, c, s, down in blocks(arch):
        ho = (h + 1) // 2 if s == 2 else h
        out.append(dict(key=key, cin=cin, cout=c, hin=h, hout=ho, stride=s, down=down))
        h = ho
    assert h == 4
    out.append(dict(key='tail', cin=512, cout=62, hin=4, hout=1, stride=1, down=False))
    return out


def mac_per_face(arch):
    """Every product the forward runs (Conv2d and the three heads), from block_shapes() alone."""
    mac = 3600 * 49 * 3 * 64
    for b in block_shapes(arch)[1:-1]:
        hw2 = b['hout'] ** 2
        mac += hw2 * 9 * b['cin'] * b['cout'] + hw2 * 9 * b['cout'] * b['cout']
        if b['down']:
            mac += hw2 * b['cin'] * b['cout']
    return mac + 512 * 62


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


def _basic_block(sd, x, blk, dtype, taps_pad0=False, down_odd=False):
    """One BasicBlock on NCHW x.  taps_pad0 / down_odd are the two WRONG alignments a port could take on a strided block (the stride-2
    taps moved by one pixel: window rows 2y .. 2y + 2 instead of 2y - 1 .. 2y + 1; the downsample read at (2y + 1, 2x + 1) instead of
    (2y, 2x)): test_resnet_basic_cpu.py shows that either moves the output of layer3.0 far beyond TOL."""
    key, cin, c, s, down = blk
    w1 = _t(sd, key + '.conv1.weight', dtype)
    if s == 2 and taps_pad0:
        y = F.conv2d(F.pad(x, (0, 2, 0, 2)), w1, None, 2, 0)[:, :, :(x.shape[2] + 1) // 2, :(x.shape[3] + 1) // 2]
    else:
        y = F.conv2d(x, w1, None, s, 1)
    y = torch.relu(_bn(sd, y, key + '.bn1', dtype))
    y = _bn(sd, F.conv2d(y, _t(sd, key + '.conv2.weight', dtype), None, 1, 1), key + '.bn2', dtype)
    r = x
    if down:
        if down_odd:
            r = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]
        r = _bn(sd, F.conv2d(r, _t(sd, key + '.downsample.0.weight', dtype), None, 2, 0), key + '.downsample.1', dtype)
    return torch.relu(y + r)


def _stem(sd, x, dtype):
    y = torch.relu(_bn(sd, F.conv2d(x, _t(sd, 'conv1.weight', dtype), None, 2, 3), 'bn1', dtype))
    return F.max_pool2d(y, 3, 2, 1)


def _tail(sd, y, dtype):
    """[B,512,4,4] -> (out62, pool512)"""
    pool = y.mean(dim=(2, 3))
    out = torch.cat([pool @ _t(sd, n + '.weight', dtype).t() + _t(sd, n + '.bias', dtype) for n in HEADS62], dim=1)
    return out, pool


def resnet_basic_forward(sd, arch, x, dtype=torch.float32, details=False):
    """sd: state_dict (numpy or torch, reference key names, no prefix); x: [B,3,120,120] normalised crops.  Returns (out62 [B,62] = ori |
    shape | exp, pool [B,512]) as numpy; with details also the block outputs (NCHW arrays: the stem + max pool, then the BasicBlocks)."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    outs = []
    with torch.no_grad():
        y = _stem(sd, x, dtype)
        outs.append(y.numpy())
        for blk in blocks(arch):
            y = _basic_block(sd, y, blk, dtype)
            outs.append(y.numpy())
        assert y.shape[1:] == (512, 4, 4)
        out, pool = _tail(sd, y, dtype)
    if details:
        return out.numpy(), pool.numpy(), outs
    return out.numpy(), pool.numpy()


def block_reference(sd, arch, block, x, dtype=torch.float64, **wrong):
    """The hook's block (syn_resnet_basic_block) in `dtype` as numpy: block 0 on NCHW crops, the others on NHWC input; out NHWC ([B,62]
    for the last block)."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    last = len(blocks(arch)) + 1
    with torch.no_grad():
        if block == 0:
            return _stem(sd, x, dtype).permute(0, 2, 3, 1).contiguous().numpy()
        x = x.permute(0, 3, 1, 2)
        if block < last:
            return _basic_block(sd, x, blocks(arch)[block - 1], dtype, **wrong).permute(0, 2, 3, 1).contiguous().numpy()
        return _tail(sd, x, dtype)[0].numpy()
