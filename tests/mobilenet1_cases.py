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
