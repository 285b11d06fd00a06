"""MI355X drop-in for the reference's inference class `synergy3DMM.SynergyNet`.

Same method set and return types as reference synergy3DMM.py:70-207
(`get_all_outputs`, `forward_test`, `reconstruct_vertex_62`, `load_weights`, attributes
`triangles`, `keypoints`, `data_param`, buffers `param_mean ... w_exp_base`), but every
piece of arithmetic runs in hand-written gfx950 kernels behind the C ABI of
include/synergy_hip.h (ctypes, see abi.py).  There is no CPU fallback.

Additions that the reference does not have (all optional):
  * batched entry points (`forward_crops_u8`, `reconstruct`, `predict_pose_batch`) - the
    reference loops over faces in Python (synergy3DMM.py:177-205);
  * `rects=` on `get_all_outputs`: the FaceBoxes detector is out of scope, so
    detections are passed in or produced by a pluggable `face_detector` callable;
  * `get_all_outputs_frames`: a list of frames in, faces out, the detections kept on the device between detector and crop
    (`face_tables`, `lanczos4_tables_device`: the ROI / box / Lanczos tap arithmetic of get_all_outputs as kernels);
  * constants can come from an in-memory pack / state_dict (synthetic assets) and can be
    broadcast from rank 0 over RCCL instead of being loaded on every rank.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import abi
from .params import ParamsPack
from .synth import (GHOSTNET_HEADS, HEADS, MOBILENET1_HEADS, RESNEST_HEADS, RESNET_HEADS, ghostnet_blocks, mbv2_layers, mobilenet1_blocks,
                    resnest50_blocks, resnet50_convs, resnet_basic_blocks)

BACKBONE_PREFIX = 'I2P.backbone.'
# the keys of SynergyNet.forward's dict in the reference's order (model_building.py:80-85), weights 0.05 / 0.05 / 0.02 / 0.02 / 0.001
LOSS_NAMES = ('loss_LMK_f0', 'loss_LMK_pointNet', 'loss_Param_In', 'loss_Param_S2', 'loss_Param_S1S2')
PARAM_LOSS_MODES = ('normal', 'only_3dmm')
_BASIS_BUFFERS = ('param_mean', 'param_std', 'w_shp', 'u', 'w_exp', 'u_base', 'w_shp_base', 'w_exp_base')


def parse_param_62(param):
    """reference synergy3DMM.py:30-37 (tensor views only; kept for callers that import it)."""
    p_ = param[:, :12].reshape(-1, 3, 4)
    p = p_[:, :, :3]
    offset = p_[:, :, -1].reshape(-1, 3, 1)
    alpha_shp = param[:, 12:52].reshape(-1, 40, 1)
    alpha_exp = param[:, 52:62].reshape(-1, 10, 1)
    return p, offset, alpha_shp, alpha_exp


# backbone ids of the C ABI (include/synergy_hip.h; the `arch` word of the constants header).  5, 7 and 9: never assigned.
ARCH_IDS = {'mobilenet_v2': 0, 'resnet50': 1, 'mobilenet_1': 2, 'mobilenet_05': 3, 'mobilenet_2': 4, 'ghostnet': 6, 'resnest50': 8,
            'resnet18': 10, 'resnet34': 11}
ARCH_BY_ID = {i: n for n, i in ARCH_IDS.items()}
ARCH_NAMES = ('mobilenet_v2', 'resnet50', 'mobilenet_1', 'mobilenet_05', 'mobilenet_2')      # ids 0..4 by position (kept for callers that index it)
_ARCH_CHOICES = ('mobilenet_v2', 'resnet50', 'resnest50', 'ghostnet', 'mobilenet_1', 'mobilenet_05', 'mobilenet_2')      # as the refusal message lists them
RESNET_BASIC = ('resnet18', 'resnet34')      # the BasicBlock ResNets; named after the bracket of the refusal message
MOBILENET1_WIDTHS = {'mobilenet_1': 1.0, 'mobilenet_05': 0.5, 'mobilenet_2': 2.0}      # the widths whose channel counts are all multiples of 16

_HDR_MAGIC = 0x53594e4833353558          # "SYNH355X" (csrc/synergy_abi.hip ConstHeader)
_HDR_VERSION = 6                         # kConstVersion: bumped whenever the packed encoding changes


def parse_constants_header(raw: bytes) -> dict:
    """The 256-byte header of an exported constants blob (csrc/synergy_abi.hip `ConstHeader`): little-endian
    u64 magic | u32 version, has_backbone, has_basis, n_vert, n_lmk, nvp, nlp, arch | u64 backbone_floats, basis_floats,
    total_bytes.  Host-side twin of the checks syn_import_constants makes; raises ValueError on a blob it would refuse."""
    import struct
    if len(raw) < 256:
        raise ValueError(f'constants blob: {len(raw)} bytes is smaller than the 256-byte header')
    magic, version, has_bb, has_basis, n_vert, n_lmk, nvp, nlp, arch, bb_fl, basis_fl, total = struct.unpack_from('<Q8I3Q', raw, 0)
    if magic != _HDR_MAGIC or version != _HDR_VERSION:
        raise ValueError('constants blob: bad magic/version')
    if has_bb and arch not in ARCH_BY_ID:
        raise ValueError(f'constants blob: unknown backbone arch {arch}')
    if has_basis and not (0 < n_vert <= nvp and 0 < n_lmk <= nlp and nvp % 32 == 0 and nlp % 32 == 0):
        raise ValueError('constants blob: inconsistent basis sizes')
    payload = 256 + 4 * ((bb_fl if has_bb else 0) + (basis_fl if has_basis else 0))
    if payload > total:
        raise ValueError(f'constants blob: header + payload = {payload} bytes exceeds total_bytes = {total}')
    return dict(version=version, has_backbone=bool(has_bb), has_basis=bool(has_basis), n_vert=n_vert, n_lmk=n_lmk, nvp=nvp, nlp=nlp,
                arch=arch, backbone_floats=bb_fl, basis_floats=basis_fl, total_bytes=total)


def backbone_keys():
    """(state_dict key, shape) of every backbone tensor, in the order syn_load_backbone expects."""
    out = []
    for L in mbv2_layers():
        if L['kind'] == 'dw':
            shape = (L['cout'], 1, 3, 3)
        elif L['kind'] == 'stem':
            shape = (L['cout'], L['cin'], 3, 3)
        else:
            shape = (L['cout'], L['cin'], 1, 1)
        out.append((L['key'] + '.weight', shape))
        for s in ('weight', 'bias', 'running_mean', 'running_var'):
            out.append((L['bn'] + '.' + s, (L['cout'],)))
    for name, n in HEADS:
        out.append((name + '.weight', (n, 1280)))
        out.append((name + '.bias', (n,)))
    return out


def resnet50_keys():
    """(state_dict key, shape) of every ResNet-50 tensor, in the order syn_load_backbone_resnet50 expects."""
    out = []
    for c in resnet50_convs():
        out.append((c['key'] + '.weight', (c['cout'], c['cin'], c['k'], c['k'])))
        for s in ('weight', 'bias', 'running_mean', 'running_var'):
            out.append((c['bn'] + '.' + s, (c['cout'],)))
    for name, n in RESNET_HEADS:
        out.append((name + '.weight', (n, 2048)))
        out.append((name + '.bias', (n,)))
    return out


def mobilenet1_keys(width: float = 1.0):
    """(state_dict key, shape) of every MobileNetV1 tensor in the module's own state_dict() order (num_batches_tracked left out):
    the order syn_load_backbone_mobilenet1 expects."""
    bn = ('weight', 'bias', 'running_mean', 'running_var')
    c0 = int(32 * width)
    out = [('conv1.weight', (c0, 3, 3, 3))] + [('bn1.' + s, (c0,)) for s in bn]
    for key, cin, cout, _ in mobilenet1_blocks(width):
        out.append((key + '.conv_dw.weight', (cin, 1, 3, 3)))
        out += [(key + '.bn_dw.' + s, (cin,)) for s in bn]
        out.append((key + '.conv_sep.weight', (cout, cin, 1, 1)))
        out += [(key + '.bn_sep.' + s, (cout,)) for s in bn]
    for name, n in MOBILENET1_HEADS:
        out.append((name + '.weight', (n, int(1024 * width))))
        out.append((name + '.bias', (n,)))
    return out


def ghostnet_keys():
    """(state_dict key, shape) of every GhostNet tensor in the module's own state_dict() order (num_batches_tracked left out): the
    order syn_load_backbone_ghostnet expects.  Written from the block table (synth.ghostnet_blocks), not from the module."""
    bn = ('weight', 'bias', 'running_mean', 'running_var')
    out = []

    def conv_bn(conv, norm, shape):
        out.append((conv + '.weight', shape))
        out.extend((norm + '.' + s, (shape[0],)) for s in bn)

    def ghost(key, cin, cout):
        assert cout % 2 == 0, f'{key}: GhostModule({cin} -> {cout}) with an odd width: the [:, :oup] slice would drop a channel'
        conv_bn(key + '.primary_conv.0', key + '.primary_conv.1', (cout // 2, cin, 1, 1))
        conv_bn(key + '.cheap_operation.0', key + '.cheap_operation.1', (cout // 2, 1, 3, 3))

    conv_bn('conv_stem', 'bn1', (16, 3, 3, 3))
    for key, cin, mid, cout, k, stride, se in ghostnet_blocks():
        ghost(key + '.ghost1', cin, mid)
        if stride == 2:
            conv_bn(key + '.conv_dw', key + '.bn_dw', (mid, 1, k, k))
        if se:
            out += [(key + '.se.conv_reduce.weight', (se, mid, 1, 1)), (key + '.se.conv_reduce.bias', (se,)),
                    (key + '.se.conv_expand.weight', (mid, se, 1, 1)), (key + '.se.conv_expand.bias', (mid,))]
        ghost(key + '.ghost2', mid, cout)
        if cin != cout or stride != 1:
            conv_bn(key + '.shortcut.0', key + '.shortcut.1', (cin, 1, k, k))
            conv_bn(key + '.shortcut.2', key + '.shortcut.3', (cout, cin, 1, 1))
    conv_bn('blocks.9.0.conv', 'blocks.9.0.bn1', (960, 160, 1, 1))
    out += [('conv_head.weight', (1280, 960, 1, 1)), ('conv_head.bias', (1280,))]
    for name, n in GHOSTNET_HEADS:
        out += [(name + '.weight', (n, 1280)), (name + '.bias', (n,))]
    return out


def resnest50_keys():
    """(state_dict key, shape) of every ResNeSt-50 tensor in the module's own state_dict() order (num_batches_tracked left out): the
    order syn_load_backbone_resnest50 expects, fc_tex included.  Written from the block table (synth.resnest50_blocks), not from the
    module."""
    bn = ('weight', 'bias', 'running_mean', 'running_var')
    out = []

    def conv_bn(conv, norm, shape):
        out.append((conv + '.weight', shape))
        out.extend((norm + '.' + s, (shape[0],)) for s in bn)

    conv_bn('conv1.0', 'conv1.1', (32, 3, 3, 3))
    conv_bn('conv1.3', 'conv1.4', (32, 32, 3, 3))
    conv_bn('conv1.6', 'bn1', (64, 32, 3, 3))
    for key, cin, c, inter, avd, down in resnest50_blocks():
        conv_bn(key + '.conv1', key + '.bn1', (c, cin, 1, 1))
        conv_bn(key + '.conv2.conv', key + '.conv2.bn0', (2 * c, c // 2, 3, 3))
        out += [(key + '.conv2.fc1.weight', (inter, c, 1, 1)), (key + '.conv2.fc1.bias', (inter,))]
        out.extend((key + '.conv2.bn1.' + s, (inter,)) for s in bn)
        out += [(key + '.conv2.fc2.weight', (2 * c, inter, 1, 1)), (key + '.conv2.fc2.bias', (2 * c,))]
        conv_bn(key + '.conv3', key + '.bn3', (4 * c, c, 1, 1))
        if down:
            conv_bn(key + '.downsample.1', key + '.downsample.2', (4 * c, cin, 1, 1))
    for name, n in RESNEST_HEADS:
        out += [(name + '.weight', (n, 2048)), (name + '.bias', (n,))]
    return out


def resnet_basic_keys(arch: str):
    """(state_dict key, shape) of every resnet18 / resnet34 tensor in the module's own state_dict() order (num_batches_tracked left out):
    the order syn_load_backbone_resnet_basic expects, fc_tex included.  Written from the block table (synth.resnet_basic_blocks), not from
    the module."""
    bn = ('weight', 'bias', 'running_mean', 'running_var')
    out = []

    def conv_bn(conv, norm, shape):
        out.append((conv + '.weight', shape))
        out.extend((norm + '.' + s, (shape[0],)) for s in bn)

    conv_bn('conv1', 'bn1', (64, 3, 7, 7))
    for key, cin, c, stride, down in resnet_basic_blocks(arch):
        conv_bn(key + '.conv1', key + '.bn1', (c, cin, 3, 3))
        conv_bn(key + '.conv2', key + '.bn2', (c, c, 3, 3))
        if down:
            conv_bn(key + '.downsample.0', key + '.downsample.1', (c, cin, 1, 1))
    for name, n in RESNET_HEADS:
        out += [(name + '.weight', (n, 512)), (name + '.bias', (n,))]
    return out


def arch_keys(arch: str):
    """The (key, shape) table of a backbone by name."""
    if arch in RESNET_BASIC:
        return resnet_basic_keys(arch)
    if arch == 'ghostnet':
        return ghostnet_keys()
    if arch == 'resnest50':
        return resnest50_keys()
    if arch in MOBILENET1_WIDTHS:
        return mobilenet1_keys(MOBILENET1_WIDTHS[arch])
    return resnet50_keys() if arch == 'resnet50' else backbone_keys()


def flatten_backbone(sd: dict, prefix: str = '', arch: str = 'mobilenet_v2') -> np.ndarray:
    """state_dict -> the flat fp32 host array of syn_load_backbone[_resnet50 | _mobilenet1 | _ghostnet | _resnest50] (include/synergy_hip.h).
    For ghostnet, resnest50, resnet18 and resnet34 the keys under `prefix` must be exactly the module's: a missing or an unexpected key is refused, like a
    wrong shape."""
    parts = []
    table = arch_keys(arch)
    if arch in ('ghostnet', 'resnest50') + RESNET_BASIC:          # strict: exactly the module's tensors
        have = {k[len(prefix):] for k in sd if k.startswith(prefix) and not k.endswith('num_batches_tracked')}
        want = {k for k, _ in table}
        if have - want:
            raise RuntimeError(f'{arch} state_dict: unexpected keys {sorted(have - want)[:4]}')
        if want - have:
            raise RuntimeError(f'{arch} state_dict: missing keys {sorted(want - have)[:4]}')
    for k, shape in table:
        v = sd[prefix + k]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if tuple(v.shape) != tuple(shape):
            raise RuntimeError(f'backbone tensor {k}: shape {tuple(v.shape)} != {tuple(shape)}')
        parts.append(np.ascontiguousarray(v, dtype=np.float32).reshape(-1))
    return np.concatenate(parts)


def synergy_state_from_checkpoint(state_dict):
    """The forwardDirection.* / reverseDirection.* tensors (MLP_for / MLP_rev, reference synergy3DMM.py:82-84) of a checkpoint's
    state_dict, DataParallel 'module.' prefixes stripped, as {key: tensor}; None when the checkpoint carries none of them.  A
    checkpoint that carries only some is broken: KeyError names what is missing.  Device-free."""
    from .synth import synergy_layers, SYNERGY_PREFIXES
    found = {}
    for k, v in state_dict.items():
        kk = k.replace('module.', '')
        if kk.startswith(SYNERGY_PREFIXES) and not kk.endswith('num_batches_tracked'):
            found[kk] = v
    if not found:
        return None
    missing = [k for k, _ in synergy_layers() if k not in found]
    if missing:
        raise KeyError(f'checkpoint carries {len(found)} synergy tensors but lacks {missing[:4]}{" ..." if len(missing) > 4 else ""}')
    return {k: found[k] for k, _ in synergy_layers()}


class _Container(nn.Module):
    """Empty node of the state_dict key tree (so state_dict() keys equal the reference's)."""


def _register_by_key(root: nn.Module, key: str, tensor: torch.Tensor):
    node = root
    parts = key.split('.')
    for p in parts[:-1]:
        if p not in node._modules:
            node.add_module(p, _Container())
        node = node._modules[p]
    node.register_buffer(parts[-1], tensor)


_DL_STREAMS = {}


def _download_stream(dev):
    """ONE extra stream per device and process for result downloads behind the compute stream (every further stream costs all of them)."""
    key = torch.device(dev).index
    if key not in _DL_STREAMS:
        _DL_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _DL_STREAMS[key]


class _WingLossFn(torch.autograd.Function):
    """SynergyNet.wing_loss under autograd: syn_wing_loss forward, syn_wing_loss_backward for the gradient"""

    @staticmethod
    def forward(ctx, model, pred, target, omega, epsilon):
        ctx.model, ctx.omega, ctx.epsilon = model, omega, epsilon
        ctx.save_for_backward(pred, target)
        return model._wing_loss(pred, target, omega, epsilon)

    @staticmethod
    @once_differentiable                                  # first order only: a double backward raises
    def backward(ctx, grad):
        pred, target = ctx.saved_tensors
        g = grad.to(device=pred.device, dtype=torch.float32).contiguous()
        d = ctx.model._wing_loss_backward(pred, target, ctx.omega, ctx.epsilon, g)
        return None, d if ctx.needs_input_grad[1] else None, -d if ctx.needs_input_grad[2] else None, None, None


class _ParamLossFn(torch.autograd.Function):
    """SynergyNet.param_loss under autograd: syn_param_loss forward, syn_param_loss_backward for the gradients"""

    @staticmethod
    def forward(ctx, model, input, target, mode):
        ctx.model, ctx.mode = model, mode
        ctx.save_for_backward(input, target)
        return model._param_loss(input, target, mode)

    @staticmethod
    @once_differentiable                                  # first order only: a double backward raises
    def backward(ctx, grad):
        input, target = ctx.saved_tensors
        g = grad.to(device=input.device, dtype=torch.float32).contiguous()
        da, db = ctx.model._param_loss_backward(input, target, ctx.mode, g, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return None, da, db, None


class _LossHeadFn(torch.autograd.Function):
    """SynergyNet.loss_head under autograd: syn_synergy_losses forward; the backward packs the five incoming gradients into
    g_scalars [2] / g_per_face [3][B] on the device and calls syn_synergy_losses_backward.  No gradient for target."""

    @staticmethod
    def forward(ctx, model, param, pool, target):
        ctx.model = model
        ctx.save_for_backward(param, pool, target)
        d = model._losses(param, pool, target)
        return tuple(d[k].clone() for k in LOSS_NAMES)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        param, pool, target = ctx.saved_tensors
        B = param.shape[0]
        f32 = dict(device=param.device, dtype=torch.float32)
        gs = torch.stack([(g if g is not None else torch.zeros((), **f32)).to(**f32).reshape(()) for g in grads[:2]]).contiguous()
        gp = torch.stack([(g if g is not None else torch.zeros((B,), **f32)).to(**f32).reshape(B) for g in grads[2:]]).contiguous()
        d_param, d_pool = ctx.model._losses_backward(param, pool, target, gs, gp)
        return None, d_param, d_pool, None


class _LossHeadWeightsFn(torch.autograd.Function):
    """_LossHeadFn with the MLPs' learnable tensors among its inputs (model.synergy_parameters()): ONE call of
    syn_synergy_losses_backward_weights gives d param, d pool and the flat weight gradient, whose slices go to the tensors."""

    @staticmethod
    def forward(ctx, model, param, pool, target, *weights):
        ctx.model = model
        ctx.save_for_backward(param, pool, target)
        d = model._losses(param, pool, target)
        return tuple(d[k].clone() for k in LOSS_NAMES)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        param, pool, target = ctx.saved_tensors
        B = param.shape[0]
        f32 = dict(device=param.device, dtype=torch.float32)
        gs = torch.stack([(g if g is not None else torch.zeros((), **f32)).to(**f32).reshape(()) for g in grads[:2]]).contiguous()
        gp = torch.stack([(g if g is not None else torch.zeros((B,), **f32)).to(**f32).reshape(B) for g in grads[2:]]).contiguous()
        d_param, d_pool, d_flat = ctx.model._losses_backward_weights(param, pool, target, gs, gp)
        dw = [d_flat[at:at + n].reshape(shape) if need else None
              for (at, n, shape), need in zip(ctx.model._syn_slices, ctx.needs_input_grad[4:])]
        return (None, d_param if ctx.needs_input_grad[1] else None, d_pool if ctx.needs_input_grad[2] else None, None, *dw)


class SynergyNet(nn.Module):
    """Drop-in for reference synergy3DMM.SynergyNet (inference only), backed by HIP kernels."""

    def __init__(self, device=None, checkpoint_fp=None, data_dir=None, pack=None, backbone_state=None,
                 face_detector=None, load_constants=True, arch='mobilenet_v2'):
        """arch: 'mobilenet_v2' (the reference's hard-coded choice, synergy3DMM.py:76) or 'resnet50' (BASELINE
        config 5; the reference's own wrapper cannot run it -- SURVEY F6 -- so the first 62 of ResNet's 102
        outputs are taken, the adapter a maintainer would add), or the MobileNetV1 family 'mobilenet_1' / 'mobilenet_05' /
        'mobilenet_2' (main_train.py --arch mobilenet_1; the same [:, :62] adapter, pool_dim = 1024 x width), or 'ghostnet'
        (main_train.py --arch ghostnet; the reference's module returns only the [B,102] tensor, so its own wrapper cannot run it: here the
        pooled feature is the 1280-vector after conv_head + ReLU that the heads consume, and the synergy refinement accepts it), or
        'resnest50' (main_train.py --arch resnest50, the reference's I2P selector synergy3DMM.py:45-56; the module returns the 62
        parameters and the 2048 channel means, pool_dim = 2048, so the synergy refinement is refused for it), or the BasicBlock
        ResNets 'resnet18' / 'resnet34' (main_train.py --arch resnet18; the [:, :62] adapter of resnet50, pool_dim = 512, the refinement
        refused likewise).  resnet101 / resnet152 and the ResNeXt / wide variants stay refused by name."""
        super().__init__()
        if arch not in ARCH_IDS:
            raise RuntimeError(f"Please choose [{', '.join(_ARCH_CHOICES)}], {' or '.join(RESNET_BASIC)}")
        self.arch = arch
        if not torch.cuda.is_available():
            raise RuntimeError('synergynet_amd.SynergyNet needs a ROCm GPU (MI355X); there is no CPU path')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._lib = abi.lib()
        h = C.c_void_p()
        abi.check(self._lib.syn_create(self.device.index, C.byref(h)))
        self._h = h
        self.face_detector = face_detector
        self.triangles = None
        self.keypoints = None
        self.data_param = None
        self._n_vert = self._n_lmk = 0
        self._have_backbone = self._have_basis = False
        self._range_checked = False
        self.has_synergy = False        # MLP_for / MLP_rev weights uploaded (load_weights / load_synergy_state)
        self._syn_flat = None           # the flat state of the last load_synergy_state (host)
        self._syn_params = None         # synergy_parameters(): {key: nn.Parameter}, created on first call
        if not load_constants:          # constants arrive later through import_constants() (synergynet_amd/dist.py)
            self.eval()
            from . import inference
            inference.set_default_model(self)
            return

        # --- 3DMM constants (reference synergy3DMM.py:8-9,73-74,95-107) ---
        pp = ParamsPack(data_dir=data_dir, pack=pack)            # raises RuntimeError('Missing data')
        self.param_pack = pp
        if pp.tri is not None:
            self.triangles = torch.Tensor((np.asarray(pp.tri) - 1).astype(np.int64)).long()
        self.register_buffer('param_mean', torch.Tensor(np.asarray(pp.param_mean, dtype=np.float32)))
        self.register_buffer('param_std', torch.Tensor(np.asarray(pp.param_std, dtype=np.float32)))
        self.register_buffer('w_shp', torch.Tensor(np.asarray(pp.w_shp, dtype=np.float32)))
        self.register_buffer('u', torch.Tensor(np.asarray(pp.u, dtype=np.float32)))
        self.register_buffer('w_exp', torch.Tensor(np.asarray(pp.w_exp, dtype=np.float32)))
        self.register_buffer('u_base', torch.Tensor(np.asarray(pp.u_base, dtype=np.float32)))
        self.register_buffer('w_shp_base', torch.Tensor(np.asarray(pp.w_shp_base, dtype=np.float32)))
        self.register_buffer('w_exp_base', torch.Tensor(np.asarray(pp.w_exp_base, dtype=np.float32)))
        self.keypoints = torch.Tensor(np.asarray(pp.keypoints)).long()
        self.data_param = [self.param_mean, self.param_std, self.w_shp_base, self.u_base, self.w_exp_base]
        self._upload_basis()

        # --- backbone weights: key tree identical to the reference's I2P.backbone.* ---
        for k, shape in arch_keys(arch):
            _register_by_key(self, BACKBONE_PREFIX + k, torch.zeros(shape, dtype=torch.float32))
        if backbone_state is not None:
            sd = {BACKBONE_PREFIX + k: torch.as_tensor(np.asarray(v)) for k, v in backbone_state.items()
                  if not k.endswith('num_batches_tracked')}
            self.load_state_dict(sd, strict=False)
            self._upload_backbone()
        else:
            fp = checkpoint_fp or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               'pretrained', 'best.pth.tar')
            try:
                self.load_weights(fp)
            except Exception as e:      # the reference swallows this silently (synergy3DMM.py:109-113)
                warnings.warn(f'SynergyNet: could not load weights from {fp} ({e}); backbone weights are zero')
                self._upload_backbone()
        self.eval()
        from . import inference
        inference.set_default_model(self)

    # nn.Module device moves must not drag the host-side constant copies around
    def _apply(self, fn, *a, **k):
        return self

    def __del__(self):
        try:
            if getattr(self, '_h', None) is not None and self._h.value:
                self._lib.syn_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ------------------------------------------------------------------ constants
    def _upload_basis(self):
        f32 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        w_shp, w_exp, u = f32(self.w_shp), f32(self.w_exp), f32(self.u).reshape(-1)
        mean, std = f32(self.param_mean).reshape(-1), f32(self.param_std).reshape(-1)
        if mean.size < 62 or std.size < 62:
            raise RuntimeError('param_mean/param_std shorter than 62')
        kp = np.ascontiguousarray(self.keypoints.numpy(), dtype=np.int64)
        n_vert = w_shp.shape[0] // 3
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        abi.check(self._lib.syn_load_basis(self._h, ptr(w_shp), ptr(w_exp), ptr(u), ptr(mean), ptr(std), ptr(kp),
                                           kp.size // 3, n_vert))
        self._n_vert, self._n_lmk = n_vert, kp.size // 3
        self._have_basis = True

    def _upload_backbone(self):
        flat = flatten_backbone(self.state_dict(), BACKBONE_PREFIX, self.arch)
        if self.arch in RESNET_BASIC:
            a = ARCH_IDS[self.arch]
            assert flat.size == self._lib.syn_resnet_basic_flat_count(a)
            abi.check(self._lib.syn_load_backbone_resnet_basic(self._h, a, flat.ctypes.data_as(C.c_void_p), flat.size))
        elif self.arch == 'resnest50':
            assert flat.size == self._lib.syn_resnest50_flat_count()
            abi.check(self._lib.syn_load_backbone_resnest50(self._h, flat.ctypes.data_as(C.c_void_p), flat.size))
        elif self.arch == 'ghostnet':
            assert flat.size == self._lib.syn_ghostnet_flat_count()
            abi.check(self._lib.syn_load_backbone_ghostnet(self._h, flat.ctypes.data_as(C.c_void_p), flat.size))
        elif self.arch in MOBILENET1_WIDTHS:
            a = ARCH_IDS[self.arch]
            assert flat.size == self._lib.syn_mobilenet1_flat_count(a)
            abi.check(self._lib.syn_load_backbone_mobilenet1(self._h, a, flat.ctypes.data_as(C.c_void_p), flat.size))
        elif self.arch == 'resnet50':
            assert flat.size == self._lib.syn_resnet50_flat_count()
            abi.check(self._lib.syn_load_backbone_resnet50(self._h, flat.ctypes.data_as(C.c_void_p), flat.size))
        else:
            assert flat.size == self._lib.syn_backbone_flat_count()
            abi.check(self._lib.syn_load_backbone(self._h, flat.ctypes.data_as(C.c_void_p), flat.size))
        self._have_backbone = True
        self._range_checked = False
        self._range_events = 0
        self._warn_numerics()

    def _guarded(self, launch):
        """Runs a backbone launch.  ResNet-50 has no static activation bound, so its fp16 convolutions are guarded at run time
        (include/synergy_hip.h syn_backbone_range_status): the FIRST forward after a weight load is checked on the host, and a tensor
        outside the fp16 window switches the handle to the exact fp32-MFMA convolutions and repeats the launch; any later forward that
        leaves the window returns NaN (checked on the device, no synchronisation) AND tells the library through a page-locked word,
        which switches the handle by itself at the entry of the next forward (syn_backbone_range_events; a warning here): a caller
        sees the NaN batch(es) already in flight, never NaN for ever."""
        launch()
        if self.arch != 'resnet50':
            return
        if not self._range_checked:
            self._range_checked = True
            if self.range_status(fallback=True)[0] > 0:
                self._range_events = self._lib.syn_backbone_range_events(self._h)
                warnings.warn('SynergyNet(resnet50): activations leave the range of the fp16x2 convolutions; '
                              'this model now runs the exact fp32-MFMA convolutions')
                launch()
        elif self._lib.syn_backbone_range_events(self._h) > getattr(self, '_range_events', 0):
            self._range_events = self._lib.syn_backbone_range_events(self._h)
            warnings.warn('SynergyNet(resnet50): an earlier batch left the range of the fp16x2 convolutions (its results are NaN); '
                          'this model now runs the exact fp32-MFMA convolutions')

    def range_status(self, fallback=False):
        """(number of guarded tensors outside the fp16 window in the last forward, per-tensor max |x| [54]); synchronises."""
        mx = np.ones(64, dtype=np.float32)
        n = self._lib.syn_backbone_range_status(self._h, mx.ctypes.data_as(C.c_void_p), 64, int(fallback))
        if n < 0:
            abi.check(n)
        return n, mx[:54]

    def calibrate(self, crops_u8, tol=2e-5):
        """Range verdict checked on the caller's OWN crops (include/synergy_hip.h syn_backbone_calibrate): block by block, the default
        fp16x2 schedule against the exact fp32-MFMA one; blocks that differ by more than `tol` are switched to the exact kernel (and a
        warning says which).  Returns the number of blocks switched.  The load-time analysis cannot rule out a checkpoint whose
        interval bounds are far looser than its real activations; a few representative crops here do."""
        crops = crops_u8 if isinstance(crops_u8, torch.Tensor) else torch.as_tensor(np.asarray(crops_u8))
        if crops.dtype != torch.uint8 or crops.dim() != 4 or tuple(crops.shape[1:]) != (120, 120, 3):
            raise RuntimeError('calibrate expects uint8 [B,120,120,3]')
        x = crops.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            n = self._lib.syn_backbone_calibrate(self._h, x.data_ptr(), x.shape[0], float(tol), self._stream())
        if n < 0:
            abi.check(n)
        if n > 0:
            self._warn_numerics()
        return n

    def check_numerics(self, crops_u8, rois=None):
        """Self-check on the caller's OWN checkpoint and images, no oracle involved: the same crops through the default schedule (fp16x2
        operands) and through the exact fp32-MFMA schedule of the same library (syn_set_schedule), parameters -> landmarks -> mesh.
        Returns the largest per-face relative differences {'param', 'lmk', 'mesh'} (max |a - b| / max |b| per face); the default
        schedule is fp32-class when they are ~1e-6.  Synchronises; not for use while other calls on this model are in flight."""
        crops = crops_u8 if isinstance(crops_u8, torch.Tensor) else torch.as_tensor(np.asarray(crops_u8))
        crops = crops.to(self.device)
        out = {}

        def run():
            p = self.forward_crops_u8(crops)
            return p, self.reconstruct(p, roi=rois, dense=False), self.reconstruct(p, roi=rois, dense=True)
        torch.cuda.synchronize(self.device)
        got = run()
        torch.cuda.synchronize(self.device)
        prev = self._lib.syn_set_schedule(self._h, 1)
        if prev < 0:
            abi.check(prev)
        try:
            want = run()
            torch.cuda.synchronize(self.device)
        finally:
            self._lib.syn_set_schedule(self._h, prev)
        for name, a, b in zip(('param', 'lmk', 'mesh'), got, want):
            a, b = a.reshape(a.shape[0], -1).double(), b.reshape(b.shape[0], -1).double()
            out[name] = float(((a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-30)).max())
        return out

    def numerics_report(self):
        """(number of blocks that do not run the default fp16x2 kernel, text) -- the load-time range verdict on the loaded weights
        (include/synergy_hip.h syn_numerics_report): fp16 operands must stay inside 2^-14 .. 65504."""
        buf = C.create_string_buffer(8192)
        n = self._lib.syn_numerics_report(self._h, buf, len(buf))
        if n < 0:
            abi.check(n)
        return n, buf.value.decode()

    def _warn_numerics(self):
        n, text = self.numerics_report()
        if n > 0:
            bad = '\n'.join(l for l in text.splitlines() if not l.endswith('-> fp16x2'))
            warnings.warn(f'SynergyNet: {n} block(s) of the loaded weights leave the range of the fp16x2 kernels and run a slower exact schedule:\n{bad}')

    def load_weights(self, path):
        """reference synergy3DMM.py:156-164: torch checkpoint {'state_dict': ...} with DataParallel
        'module.' prefixes.  The two point-MLPs (forwardDirection.* / reverseDirection.*) are uploaded for refine_landmarks /
        landmarks_to_param when the checkpoint carries them (has_synergy); other keys this class does not have are ignored.
        A checkpoint that carries the 3DMM buffers overrides the .npy values, as in the reference."""
        model_dict = self.state_dict()
        checkpoint = torch.load(path, map_location=lambda storage, loc: storage)['state_dict']
        basis_touched = False
        for k in checkpoint.keys():
            kk = k.replace('module.', '')
            if kk in model_dict:
                model_dict[kk] = checkpoint[k]
                basis_touched |= kk in _BASIS_BUFFERS
        self.load_state_dict(model_dict, strict=False)
        self._upload_backbone()
        if basis_touched:
            self._upload_basis()
        syn_sd = synergy_state_from_checkpoint(checkpoint)
        if syn_sd is not None:
            self.load_synergy_state(syn_sd)

    def load_synergy_state(self, sd, prefix=''):
        """Uploads MLP_for / MLP_rev from a state_dict with the reference's key names (forwardDirection.* / reverseDirection.*;
        synth.make_synergy_state for synthetic ones).  Calling it again replaces the weights."""
        from .synth import flatten_synergy
        flat = flatten_synergy({k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}, prefix)
        assert flat.size == self._lib.syn_synergy_flat_count()
        abi.check(self._lib.syn_load_synergy(self._h, flat.ctypes.data_as(C.c_void_p), flat.size))
        self.has_synergy = True
        self._syn_flat = flat
        self._syn_flat_stale = False
        if self._syn_params is not None:                     # the parameters follow the new state; the handle already holds it
            with torch.no_grad():
                for k, t in self._syn_tensors.items():
                    at, n, shape = self._syn_where[k]
                    t.copy_(torch.from_numpy(flat[at:at + n].reshape(shape)))
            self._syn_uploaded = self._syn_versions()

    # --- fine-tuning the two point-MLPs with frozen BatchNorm statistics ---
    def synergy_parameters(self):
        """Ordered {state_dict key: nn.Parameter} of the learnable tensors of MLP_for / MLP_rev (conv weight and bias, BatchNorm weight
        and bias; the reference's key names and shapes), device tensors created on the first call from the loaded state.  They are NOT
        registered on the module: state_dict() and parameters() stay what they were.  `loss_head` returns their gradients when they
        require grad and re-uploads them when an optimiser has changed them (syn_update_synergy_device)."""
        self._need_synergy()
        if self._syn_params is None:
            from .synth import synergy_layers
            self._syn_where, self._syn_tensors, at = {}, {}, 0
            for key, shape in synergy_layers():
                n = int(np.prod(shape))
                self._syn_where[key] = (at, n, shape)
                t = torch.from_numpy(self._host_flat()[at:at + n].reshape(shape).copy()).to(self.device)
                self._syn_tensors[key] = t if 'running_' in key else nn.Parameter(t)
                at += n
            self._syn_params = {k: t for k, t in self._syn_tensors.items() if isinstance(t, nn.Parameter)}
            self._syn_slices = [self._syn_where[k] for k in self._syn_params]
            self._syn_uploaded = self._syn_versions()
        return dict(self._syn_params)

    def _syn_versions(self):
        return tuple(t._version for t in self._syn_tensors.values())

    def _sync_synergy(self):
        """the handle's weights follow the parameters: one flat device tensor and syn_update_synergy_device, only after a change"""
        if self._syn_params is None or self._syn_versions() == self._syn_uploaded:
            return
        with torch.cuda.device(self.device), torch.no_grad():
            flat = torch.cat([t.detach().reshape(-1) for t in self._syn_tensors.values()]).contiguous()
            abi.check(self._lib.syn_update_synergy_device(self._h, flat.data_ptr(), flat.numel(), self._stream()))
        self._syn_uploaded = self._syn_versions()

    def _export_synergy_flat(self):
        """the handle's flat state as one device tensor (syn_export_synergy_flat: a copy, no arithmetic)"""
        with torch.cuda.device(self.device):
            flat = torch.empty((int(self._lib.syn_synergy_flat_count()),), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_export_synergy_flat(self._h, flat.data_ptr(), flat.numel(), self._stream()))
        return flat

    def _running_moved(self):
        """after a call that moved the running statistics on the handle (loss_head(bn='batch')): the running_* tensors behind
        synergy_parameters() take them over, and the host copy is marked stale"""
        self._syn_flat_stale = True
        if self._syn_params is not None:
            flat = self._export_synergy_flat()
            with torch.no_grad():
                for k, t in self._syn_tensors.items():
                    if 'running_' in k:
                        at, n, shape = self._syn_where[k]
                        t.copy_(flat[at:at + n].reshape(shape))
            self._syn_uploaded = self._syn_versions()        # the handle already holds them: nothing stale goes up

    def _host_flat(self):
        if getattr(self, '_syn_flat_stale', False):
            self._syn_flat = self._export_synergy_flat().cpu().numpy()
            self._syn_flat_stale = False
        return self._syn_flat

    def synergy_state_dict(self):
        """the current flat state as {key: tensor} with the reference's key names (load_synergy_state takes it back); after
        loss_head(bn='batch') / recalibrate_synergy_bn the running statistics are the moved ones"""
        self._need_synergy()
        if self._syn_params is not None:
            return {k: t.detach().clone() for k, t in self._syn_tensors.items()}
        from .synth import synergy_layers
        flat = self._host_flat()
        out, at = {}, 0
        for key, shape in synergy_layers():
            n = int(np.prod(shape))
            out[key] = torch.from_numpy(flat[at:at + n].reshape(shape).copy()).to(self.device)
            at += n
        return out

    # --- multi-GPU: rank `src` loads, everybody else receives ---
    def constants_nbytes(self) -> int:
        return int(self._lib.syn_constants_bytes(self._h))

    def export_constants(self) -> torch.Tensor:
        """Packed constants (header | folded backbone | MFMA-ordered basis) as a uint8 device tensor."""
        n = self.constants_nbytes()
        buf = torch.empty(n, dtype=torch.uint8, device=self.device)
        abi.check(self._lib.syn_export_constants(self._h, buf.data_ptr(), n, self._stream()))
        return buf

    def import_constants(self, buf: torch.Tensor):
        assert buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()
        hdr = parse_constants_header(buf[:256].cpu().numpy().tobytes())
        abi.check(self._lib.syn_import_constants(self._h, buf.data_ptr(), buf.numel(), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        self._follow_constants(hdr)

    def _after_import(self):
        """The C handle has imported constants on its own (syn_bcast_constants): read back what it holds now."""
        raw = C.create_string_buffer(256)
        abi.check(self._lib.syn_describe_constants(self._h, raw, 256))
        self._follow_constants(parse_constants_header(raw.raw))

    def _follow_constants(self, hdr):
        if hdr['has_backbone']:
            # the blob decides which backbone the C handle now runs: follow it, or pool buffers would be sized for the wrong one
            self.arch = ARCH_BY_ID[hdr['arch']]
            self._have_backbone = True
            self._range_checked = False
            self._range_events = 0          # the C side starts counting from 0 again on an import (a stale count here hid the next warning)
            self._warn_numerics()
        if hdr['has_basis']:
            self._n_vert, self._n_lmk = hdr['n_vert'], hdr['n_lmk']
            self._have_basis = True

    # ------------------------------------------------------------------ helpers
    @property
    def pool_dim(self):
        if self.arch in MOBILENET1_WIDTHS:
            return int(1024 * MOBILENET1_WIDTHS[self.arch])
        if self.arch in RESNET_BASIC:
            return 512
        return 2048 if self.arch in ('resnet50', 'resnest50') else 1280

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev_f32(self, t):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ reference API
    def forward_test(self, input, return_pool=False):
        """reference synergy3DMM.py:151-154: [B,3,120,120] fp32 (already (x-127.5)/128) -> [B,62]."""
        was_cpu = isinstance(input, torch.Tensor) and not input.is_cuda
        x = self._dev_f32(input)
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, 120, 120):
            raise RuntimeError(f'forward_test expects [B,3,120,120], got {tuple(x.shape)}')
        B = x.shape[0]
        with torch.cuda.device(self.device):
            param = torch.empty((B, 62), dtype=torch.float32, device=self.device)
            pool = torch.empty((B, self.pool_dim), dtype=torch.float32, device=self.device) if return_pool else None
            self._guarded(lambda: abi.check(self._lib.syn_backbone_forward(self._h, x.data_ptr(), B, param.data_ptr(),
                                                                          pool.data_ptr() if return_pool else None, self._stream())))
        if was_cpu:
            param = param.cpu()
            pool = pool.cpu() if return_pool else None
        return (param, pool) if return_pool else param

    def forward_crops_u8(self, crops, return_pool=False):
        """uint8 crops [B,120,120,3] (HWC BGR, the output of cv2.resize at synergy3DMM.py:188) -> [B,62];
        the HWC->CHW permute and (x-127.5)/128 of :189-192 are fused into the first convolution."""
        if not isinstance(crops, torch.Tensor):
            crops = torch.as_tensor(np.asarray(crops))
        if crops.dtype != torch.uint8 or crops.dim() != 4 or tuple(crops.shape[1:]) != (120, 120, 3):
            raise RuntimeError('forward_crops_u8 expects uint8 [B,120,120,3]')
        x = crops.to(self.device).contiguous()
        B = x.shape[0]
        with torch.cuda.device(self.device):
            param = torch.empty((B, 62), dtype=torch.float32, device=self.device)
            pool = torch.empty((B, self.pool_dim), dtype=torch.float32, device=self.device) if return_pool else None
            self._guarded(lambda: abi.check(self._lib.syn_backbone_forward_u8(self._h, x.data_ptr(), B, param.data_ptr(),
                                                                             pool.data_ptr() if return_pool else None, self._stream())))
        return (param, pool) if return_pool else param

    def reconstruct(self, param, roi=None, dense=False, transform=True, out=None):
        """Batched reconstruct_vertex_62 (+ optional ROI affine of utils/inference.py:127-138) on device."""
        p = self._dev_f32(param)
        if p.dim() != 2:
            raise RuntimeError('param must be [B,62]')
        B = p.shape[0]
        n = self._n_vert if dense else self._n_lmk
        r = None
        if roi is not None:
            r = self._dev_f32(roi)
            if tuple(r.shape) != (B, 5):
                raise RuntimeError('roi must be [B,5] (sx,sy,ex,ey,score)')
        with torch.cuda.device(self.device):
            if out is None:
                out = self.empty_vertices(B, dense)
            if tuple(out.shape) != (B, 3, n) or out.dtype != torch.float32 or out.device != self.device:
                raise RuntimeError(f'out must be a float32 [B,3,{n}] tensor on {self.device}')
            pitch = out.stride(1)
            if out.stride(2) != 1 or pitch < n or (B > 1 and out.stride(0) != 3 * pitch):
                raise RuntimeError('out must have unit column stride and equally pitched rows (a [B,3,pitch][..., :n] view)')
            try:
                abi.check(self._lib.syn_reconstruct_pitched(self._h, p.data_ptr(), B, p.shape[1], int(dense), int(transform),
                                                            r.data_ptr() if r is not None else None, out.data_ptr(), int(pitch),
                                                            int(getattr(out, '_syn_pad_writable', False)), self._stream()))
            except abi.SynergyHipError as e:
                if e.code == abi.SYN_ERR_PARAM_LEN:
                    raise RuntimeError('length of params mismatch') from None
                raise
        return out

    def empty_vertices(self, B, dense=True):
        """Output buffer for `reconstruct`: a [B,3,n] float32 view whose rows are 512-byte aligned (row pitch rounded up to 128
        floats: 53215 -> 53248, +0.06 % memory; the pad columns receive unspecified values).  Same shape and values as the reference's packed tensor
        (synergy3DMM.py:131-147), but every store of the kernel is a whole HBM line (include/synergy_hip.h,
        syn_reconstruct_pitched); `.contiguous()` gives the packed copy where a consumer needs one."""
        n = self._n_vert if dense else self._n_lmk
        pitch = (n + 127) // 128 * 128 if n >= 1024 else n          # whole 128-vertex store runs (csrc/recon_kernels.hip)
        out = torch.empty((B, 3, pitch), dtype=torch.float32, device=self.device)[:, :, :n]
        out._syn_pad_writable = pitch > n        # this very tensor object owns its pad columns (views / slices of it do not inherit the mark)
        return out

    def reconstruct_vertex_62(self, param, whitening=True, dense=False, transform=True, lmk_pts=68):
        """reference synergy3DMM.py:116-149.  [B,62] whitened -> [B,3,68] or [B,3,53215] in 120x120 crop
        coordinates (no ROI affine), on the device of `param`."""
        if not whitening:
            # the reference leaves `param_` unbound on this branch (synergy3DMM.py:125-131)
            raise UnboundLocalError("local variable 'param_' referenced before assignment")
        if not dense and lmk_pts != self._n_lmk:
            raise RuntimeError(f'lmk_pts={lmk_pts} but the landmark basis has {self._n_lmk} points')
        was_cpu = isinstance(param, torch.Tensor) and not param.is_cuda
        out = self.reconstruct(param, roi=None, dense=dense, transform=transform)
        return out.cpu() if was_cpu else out

    def predict_pose_batch(self, param, roi=None):
        """Batched predict_pose (utils/inference.py:146-157): angles [B,3] float64 degrees, t3d [B,3] fp32."""
        p = self._dev_f32(param)
        if p.dim() != 2 or p.shape[1] != 62:
            raise RuntimeError('length of params mismatch')
        B = p.shape[0]
        r = self._dev_f32(roi) if roi is not None else None
        if r is not None and tuple(r.shape) != (B, 5):
            raise RuntimeError('roi must be [B,5] (sx,sy,ex,ey,score)')
        with torch.cuda.device(self.device):
            ang = torch.empty((B, 3), dtype=torch.float64, device=self.device)
            t3d = torch.empty((B, 3), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_pose(self._h, p.data_ptr(), B, r.data_ptr() if r is not None else None,
                                         ang.data_ptr(), t3d.data_ptr(), self._stream()))
        return ang, t3d

    def landmarks_and_pose(self, param, roi=None, transform=True, out=None):
        """`reconstruct(param, roi, dense=False, transform)` and `predict_pose_batch(param, roi)` in ONE launch (syn_landmarks_pose): what
        get_all_outputs needs per face besides the mesh (reference synergy3DMM.py:194-201).  Returns (lmk [B,3,68], (angles [B,3] float64, t3d
        [B,3])); landmarks equal to `reconstruct`'s to fp32 rounding, pose as `predict_pose_batch` (translation the same bits, angles within 1e-4 degree)."""
        p = self._dev_f32(param)
        if p.dim() != 2:
            raise RuntimeError('param must be [B,62]')
        if p.shape[1] != 62:
            raise RuntimeError('length of params mismatch')
        B, n = p.shape[0], self._n_lmk
        r = self._dev_f32(roi) if roi is not None else None
        if r is not None and tuple(r.shape) != (B, 5):
            raise RuntimeError('roi must be [B,5] (sx,sy,ex,ey,score)')
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((B, 3, n), dtype=torch.float32, device=self.device)
            if tuple(out.shape) != (B, 3, n) or out.dtype != torch.float32 or out.device != self.device:
                raise RuntimeError(f'out must be a float32 [B,3,{n}] tensor on {self.device}')
            if not out.is_contiguous():
                # the one-launch kernel writes packed rows only; an equally pitched / sliced view (which `reconstruct` has always taken) goes
                # through the two calls it replaces -- same landmarks to fp32 rounding, same pose (do not narrow the API silently)
                self.reconstruct(p, roi=r, dense=False, transform=transform, out=out)
                return out, self.predict_pose_batch(p, roi=r)
            ang = torch.empty((B, 3), dtype=torch.float64, device=self.device)
            t3d = torch.empty((B, 3), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_landmarks_pose(self._h, p.data_ptr(), B, 62, int(transform), r.data_ptr() if r is not None else None,
                                                   out.data_ptr(), ang.data_ptr(), t3d.data_ptr(), self._stream()))
        return out, (ang, t3d)

    # ------------------------------------------------------------------ synergy refinement (MLP_for / MLP_rev)
    def _need_synergy(self):
        if self.arch not in ('mobilenet_v2', 'ghostnet'):
            raise RuntimeError(f'the synergy refinement needs the 1280-d pooled feature of mobilenet_v2 or ghostnet; arch={self.arch} pools {self.pool_dim}')
        if not self.has_synergy:
            raise RuntimeError('synergy weights not loaded: the checkpoint carried no forwardDirection.* / reverseDirection.* keys '
                               '(load_synergy_state)')
        if self._syn_params is not None:
            self._sync_synergy()

    def _check_faces(self, name, t, shape):
        t = self._dev_f32(t)
        if t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != shape:
            raise RuntimeError(f'{name} must be [B,{",".join(map(str, shape))}], got {tuple(t.shape)}')
        return t

    def refine_landmarks(self, param, pool, roi=None, transform=True, return_coarse=False):
        """model_building.py:149-152 on device: Lc = reconstruct_vertex_62(param), Lr = Lc + 0.05 MLP_for(Lc, pool, shape code, expression
        code) -> [B,3,68] (with `roi` in image space, like landmarks_and_pose).  return_coarse: (Lr, Lc), Lc as landmarks_and_pose gives it."""
        self._need_synergy()
        p, po = self._check_faces('param', param, (62,)), self._check_faces('pool', pool, (1280,))
        B = p.shape[0]
        if po.shape[0] != B:
            raise RuntimeError('param and pool must hold the same number of faces')
        r = self._check_faces('roi', roi, (5,)) if roi is not None else None
        if r is not None and r.shape[0] != B:
            raise RuntimeError('roi must be [B,5] (sx,sy,ex,ey,score)')
        with torch.cuda.device(self.device):
            out = torch.empty((B, 3, 68), dtype=torch.float32, device=self.device)
            coarse = torch.empty_like(out) if return_coarse else None
            abi.check(self._lib.syn_refine_landmarks(self._h, p.data_ptr(), po.data_ptr(), B, int(transform), r.data_ptr() if r is not None else None,
                                                     coarse.data_ptr() if return_coarse else None, out.data_ptr(), None, self._stream()))
        return (out, coarse) if return_coarse else out

    def refine_points(self, lmk, pool, param):
        """Lr = lmk + 0.05 MLP_for(lmk, pool, param[:,12:52], param[:,52:62]) on landmarks the caller supplies (crop space) -> [B,3,68]"""
        self._need_synergy()
        l, po, p = self._check_faces('lmk', lmk, (3, 68)), self._check_faces('pool', pool, (1280,)), self._check_faces('param', param, (62,))
        B = l.shape[0]
        if po.shape[0] != B or p.shape[0] != B:
            raise RuntimeError('lmk, pool and param must hold the same number of faces')
        with torch.cuda.device(self.device):
            out = torch.empty((B, 3, 68), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_refine_points(self._h, l.data_ptr(), po.data_ptr(), p.data_ptr(), B, out.data_ptr(), None, self._stream()))
        return out

    def landmarks_to_param(self, lmk):
        """MLP_rev (model_building.py:153): crop-space landmarks [B,3,68] -> whitened parameters [B,62]"""
        self._need_synergy()
        l = self._check_faces('lmk', lmk, (3, 68))
        with torch.cuda.device(self.device):
            out = torch.empty((l.shape[0], 62), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_landmarks_to_param(self._h, l.data_ptr(), l.shape[0], out.data_ptr(), self._stream()))
        return out

    def forward_synergy(self, input):
        """[B,3,120,120] -> dict(param, lmk, lmk_refined, param_rev): backbone, refinement and the reverse direction of the training
        graph (model_building.py:144-153), all on device with no host round trip between them; landmarks in crop space."""
        self._need_synergy()
        param, pool = self.forward_test(self._dev_f32(input), return_pool=True)
        lmk_refined, lmk = self.refine_landmarks(param, pool, return_coarse=True)
        return dict(param=param, lmk=lmk, lmk_refined=lmk_refined, param_rev=self.landmarks_to_param(lmk_refined))

    # ------------------------------------------------------------------ losses of the training graph's forward
    def get_losses(self):
        """reference model_building.py:164-165: the keys of forward's dict, in its order"""
        return LOSS_NAMES

    def wing_loss(self, pred, target, omega=10, epsilon=2):
        """reference loss_definition.py WingLoss on [B,3,n] tensors -> 0-d device tensor (syn_wing_loss; any backbone)"""
        p, t = self._dev_f32(pred), self._dev_f32(target)
        if p.dim() != 3 or p.shape[1] != 3 or p.shape[0] < 1 or p.shape[2] < 1:
            raise RuntimeError(f'pred must be [B,3,n], got {tuple(p.shape)}')
        if t.shape != p.shape:
            raise RuntimeError(f'target must have the shape of pred {tuple(p.shape)}, got {tuple(t.shape)}')
        if torch.is_grad_enabled() and (p.requires_grad or t.requires_grad):
            return _WingLossFn.apply(self, p, t, float(omega), float(epsilon))
        return self._wing_loss(p, t, float(omega), float(epsilon))

    def _wing_loss(self, p, t, omega, epsilon):
        with torch.cuda.device(self.device):
            out = torch.empty((), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_wing_loss(self._h, p.data_ptr(), t.data_ptr(), p.shape[0], p.shape[2], omega, epsilon, out.data_ptr(),
                                              self._stream()))
        return out

    def _wing_loss_backward(self, p, t, omega, epsilon, g=None):
        """syn_wing_loss_backward: the gradient of `pred` for the upstream g (0-d device tensor; None: 1); target's is its negative"""
        with torch.cuda.device(self.device):
            out = torch.empty_like(p)
            abi.check(self._lib.syn_wing_loss_backward(self._h, p.data_ptr(), t.data_ptr(), p.shape[0], p.shape[2], omega, epsilon,
                                                       g.data_ptr() if g is not None else None, out.data_ptr(), self._stream()))
        return out

    def param_loss(self, input, target, mode='normal'):
        """reference loss_definition.py ParamLoss on [B,62] tensors -> [B] device tensor (syn_param_loss; any backbone).  With an input
        that requires grad the result carries a grad_fn (syn_param_loss_backward); so does `wing_loss`."""
        if mode not in PARAM_LOSS_MODES:
            raise RuntimeError(f"mode must be 'normal' or 'only_3dmm', got {mode!r}")
        a, b = self._check_faces('input', input, (62,)), self._check_faces('target', target, (62,))
        if a.shape[0] != b.shape[0] or a.shape[0] < 1:
            raise RuntimeError('input and target must hold the same number of faces (at least one)')
        if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
            return _ParamLossFn.apply(self, a, b, PARAM_LOSS_MODES.index(mode))
        return self._param_loss(a, b, PARAM_LOSS_MODES.index(mode))

    def _param_loss(self, a, b, mode):
        with torch.cuda.device(self.device):
            out = torch.empty((a.shape[0],), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_param_loss(self._h, a.data_ptr(), b.data_ptr(), a.shape[0], mode, out.data_ptr(), self._stream()))
        return out

    def _param_loss_backward(self, a, b, mode, g=None, want_input=True, want_target=False):
        """syn_param_loss_backward -> (d_input or None, d_target or None) for the upstream g ([B] device tensor; None: ones)"""
        with torch.cuda.device(self.device):
            da = torch.empty_like(a) if want_input else None
            db = torch.empty_like(b) if want_target else None
            abi.check(self._lib.syn_param_loss_backward(self._h, a.data_ptr(), b.data_ptr(), a.shape[0], mode,
                                                        g.data_ptr() if g is not None else None, da.data_ptr() if want_input else None,
                                                        db.data_ptr() if want_target else None, self._stream()))
        return da, db

    def _losses(self, param, pool, target, meter=None):
        t = self._check_faces('target', target, (62,))
        B = param.shape[0]
        if t.shape[0] != B:
            raise RuntimeError(f'target must be [{B},62] (one row per face of the input), got {tuple(t.shape)}')
        if meter is not None and not (isinstance(meter, torch.Tensor) and meter.dtype == torch.float64 and tuple(meter.shape) == (8,)
                                      and meter.device == self.device and meter.is_contiguous()):
            raise RuntimeError(f'meter must be a contiguous float64 [8] tensor on {self.device}')
        with torch.cuda.device(self.device):
            scalars = torch.empty((2,), dtype=torch.float32, device=self.device)
            per_face = torch.empty((3, B), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_synergy_losses(self._h, param.data_ptr(), t.data_ptr(), pool.data_ptr(), B, scalars.data_ptr(),
                                                   per_face.data_ptr(), meter.data_ptr() if meter is not None else None, self._stream()))
        return dict(zip(LOSS_NAMES, (scalars[0], scalars[1], per_face[0], per_face[1], per_face[2])))

    def _losses_backward(self, param, pool, target, g_scalars=None, g_per_face=None):
        B = param.shape[0]
        with torch.cuda.device(self.device):
            d_param = torch.empty((B, 62), dtype=torch.float32, device=self.device)
            d_pool = torch.empty((B, 1280), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_synergy_losses_backward(self._h, param.data_ptr(), target.data_ptr(), pool.data_ptr(), B,
                                                            g_scalars.data_ptr() if g_scalars is not None else None,
                                                            g_per_face.data_ptr() if g_per_face is not None else None,
                                                            d_param.data_ptr(), d_pool.data_ptr(), self._stream()))
        return d_param, d_pool

    def _losses_backward_weights(self, param, pool, target, g_scalars=None, g_per_face=None):
        """syn_synergy_losses_backward_weights -> (d_param, d_pool, d_flat [syn_synergy_flat_count()])"""
        B = param.shape[0]
        with torch.cuda.device(self.device):
            d_param = torch.empty((B, 62), dtype=torch.float32, device=self.device)
            d_pool = torch.empty((B, 1280), dtype=torch.float32, device=self.device)
            d_flat = torch.empty((int(self._lib.syn_synergy_flat_count()),), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_synergy_losses_backward_weights(self._h, param.data_ptr(), target.data_ptr(), pool.data_ptr(), B,
                                                                    g_scalars.data_ptr() if g_scalars is not None else None,
                                                                    g_per_face.data_ptr() if g_per_face is not None else None,
                                                                    d_param.data_ptr(), d_pool.data_ptr(), d_flat.data_ptr(), self._stream()))
        return d_param, d_pool, d_flat

    def _head_inputs(self, param, pool, target):
        self._need_synergy()
        p, po, t = self._check_faces('param', param, (62,)), self._check_faces('pool', pool, (1280,)), self._check_faces('target', target, (62,))
        if po.shape[0] != p.shape[0] or t.shape[0] != p.shape[0] or p.shape[0] < 1:
            raise RuntimeError('param, pool and target must hold the same number of faces (at least one)')
        return p, po, t

    def _losses_train(self, param, pool, target, momentum=0.1, meter=None, batch_stats=None):
        """syn_synergy_losses_train: the dict of `_losses` with every BatchNorm of the two MLPs on the statistics of this
        batch; momentum None leaves the running statistics alone.  batch_stats: optional float32 [2, 3649] device tensor to fill."""
        t = self._check_faces('target', target, (62,))
        B = param.shape[0]
        if t.shape[0] != B:
            raise RuntimeError(f'target must be [{B},62] (one row per face of the input), got {tuple(t.shape)}')
        if B < 2:
            raise RuntimeError(f"bn='batch': Expected more than 1 value per channel when training, got input size [{B}, 12, 1]")
        if momentum is not None and not 0.0 <= float(momentum) <= 1.0:
            raise RuntimeError(f'momentum must be None (running statistics untouched) or in [0, 1], got {momentum}')
        if meter is not None and not (isinstance(meter, torch.Tensor) and meter.dtype == torch.float64 and tuple(meter.shape) == (8,)
                                      and meter.device == self.device and meter.is_contiguous()):
            raise RuntimeError(f'meter must be a contiguous float64 [8] tensor on {self.device}')
        n_bn = int(self._lib.syn_synergy_bn_channels())
        if batch_stats is not None and not (isinstance(batch_stats, torch.Tensor) and batch_stats.dtype == torch.float32
                                            and tuple(batch_stats.shape) == (2, n_bn) and batch_stats.device == self.device
                                            and batch_stats.is_contiguous()):
            raise RuntimeError(f'batch_stats must be a contiguous float32 [2,{n_bn}] tensor on {self.device}')
        with torch.cuda.device(self.device):
            scalars = torch.empty((2,), dtype=torch.float32, device=self.device)
            per_face = torch.empty((3, B), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_synergy_losses_train(self._h, param.data_ptr(), t.data_ptr(), pool.data_ptr(), B, scalars.data_ptr(),
                                                         per_face.data_ptr(), meter.data_ptr() if meter is not None else None,
                                                         batch_stats.data_ptr() if batch_stats is not None else None,
                                                         -1.0 if momentum is None else float(momentum), self._stream()))
        if momentum is not None:
            self._running_moved()
        return dict(zip(LOSS_NAMES, (scalars[0], scalars[1], per_face[0], per_face[1], per_face[2])))

    def _no_backward_under_batch_statistics(self, *tensors):
        ws = self._syn_params.values() if self._syn_params is not None else ()
        if torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.requires_grad for x in (*tensors, *ws)):
            raise RuntimeError("bn='batch': there is no backward under BatchNorm batch statistics yet (forward only); call it under "
                               "torch.no_grad() or on tensors that do not require grad -- the eval() gradients are never handed out for it")

    def loss_head(self, param, pool, target, bn='running', momentum=0.1):
        """The loss head behind any backbone: whitened param [B,62], pooled feature [B,1280], whitened target [B,62] -> the reference's
        dict of the five weighted losses (keys, order and values of `forward`).  If param or pool requires grad the tensors carry a
        grad_fn whose backward is syn_synergy_losses_backward (the head in eval() form); target gets no gradient.
        If a tensor of `synergy_parameters()` requires grad, the backward is syn_synergy_losses_backward_weights and also returns
        their gradients; parameters an optimiser changed are uploaded before the forward.
        bn='batch' (DESIGN 5.21): the reference in train() -- every BatchNorm of MLP_for / MLP_rev normalises by the statistics of this
        batch (B >= 2) and the running statistics move by `momentum` (None: untouched); forward only: anything that requires grad
        raises.  The switch is this keyword, never self.training."""
        if bn not in ('running', 'batch'):
            raise RuntimeError(f"bn must be 'running' or 'batch', got {bn!r}")
        p, po, t = self._head_inputs(param, pool, target)
        if bn == 'batch':
            self._no_backward_under_batch_statistics(p, po)
            return self._losses_train(p, po, t, momentum)
        ws = self._syn_params
        if torch.is_grad_enabled() and ws is not None and any(w.requires_grad for w in ws.values()):
            return dict(zip(LOSS_NAMES, _LossHeadWeightsFn.apply(self, p, po, t.detach(), *ws.values())))
        if torch.is_grad_enabled() and (p.requires_grad or po.requires_grad):
            return dict(zip(LOSS_NAMES, _LossHeadFn.apply(self, p, po, t.detach())))
        return self._losses(p, po, t)

    def loss_total_grad(self, param, pool, target):
        """(d_param [B,62], d_pool [B,1280]) of main_train.py:128-132's loss_total = the sum of the five losses' means"""
        p, po, t = self._head_inputs(param, pool, target)
        return self._losses_backward(p.detach(), po.detach(), t.detach())

    def forward(self, input, target, meter=None, bn='running', momentum=0.1):
        """reference model_building.py:141-157: [B,3,120,120] crops (whatever forward_test takes) and the whitened [B,62] target -> the
        dict of the five weighted losses, device tensors: the two landmark losses 0-d, the three parameter losses [B].  Forward only.
        meter: a zeroed float64 [8] device tensor the batch is added to (include/synergy_hip.h syn_synergy_losses; `validate`).
        bn='batch': the two MLPs on the statistics of this batch, as `loss_head` (the backbone stays in eval() form)."""
        if bn not in ('running', 'batch'):
            raise RuntimeError(f"bn must be 'running' or 'batch', got {bn!r}")
        self._need_synergy()
        if bn == 'batch':
            self._no_backward_under_batch_statistics(input)
        param, pool = self.forward_test(self._dev_f32(input), return_pool=True)
        if bn == 'batch':
            return self._losses_train(param, pool, target, momentum, meter)
        return self._losses(param, pool, target, meter)

    def recalibrate_synergy_bn(self, batches):
        """Re-estimates the running statistics of MLP_for / MLP_rev for the weights as they stand (after a fine-tuning run with frozen
        statistics, before synergy_state_dict() is saved): batch k of the iterable of (param, pool, target) runs `loss_head(bn='batch')`
        with momentum 1 / k -- torch's momentum=None cumulative average --, so that afterwards the running statistics are the mean of
        the batches' statistics (the variance in its unbiased form).  -> the number of batches."""
        k = 0
        with torch.no_grad():
            for param, pool, target in batches:
                k += 1
                self.loss_head(param, pool, target, bn='batch', momentum=1.0 / k)
        if k == 0:
            raise RuntimeError('recalibrate_synergy_bn: no batches')
        return k

    def losses_crops_u8(self, crops, target, meter=None, bn='running', momentum=0.1):
        """`forward` from uint8 crops [B,120,120,3] (what forward_crops_u8 takes, and what augment.TrainTransform(out='u8') gives);
        bn / momentum as `forward` has them"""
        if bn not in ('running', 'batch'):
            raise RuntimeError(f"bn must be 'running' or 'batch', got {bn!r}")
        self._need_synergy()
        param, pool = self.forward_crops_u8(crops, return_pool=True)
        if bn == 'batch':
            return self._losses_train(param, pool, target, momentum, meter)
        return self._losses(param, pool, target, meter)

    def validate(self, batches):
        """The bookkeeping of main_train.py:106-134 over an iterable of (crops or input, target) batches: every batch goes through
        `losses_crops_u8` (uint8 crops) or `forward` with ONE device-side meter, which is read once at the end -- no device-to-host
        copy inside the loop.  -> {name: average} for the five losses and 'loss_total'; each batch's mean weighs in with its size, as
        AverageMeter.update(mean, B) does."""
        self._need_synergy()
        meter = torch.zeros((8,), dtype=torch.float64, device=self.device)
        for x, target in batches:
            u8 = x.dtype == torch.uint8 if isinstance(x, torch.Tensor) else np.asarray(x).dtype == np.uint8
            (self.losses_crops_u8 if u8 else self.forward)(x, target, meter=meter)
        m = meter.cpu().numpy()
        if m[6] == 0:
            raise RuntimeError('validate: no batches')
        return {name: float(m[i] / m[6]) for i, name in enumerate(LOSS_NAMES + ('loss_total',))}

    def pose_matrix_batch(self, param):
        """Batched predict_pose(..., ret_mat=True) (utils/inference.py:146-157): [B,3,4] fp32 = [R | t3d] of parse_pose
        (:86-92), the translation column WITHOUT the ROI affine (the reference builds P before rescaling t3d)."""
        p = self._dev_f32(param)
        if p.dim() != 2 or p.shape[1] != 62:
            raise RuntimeError('length of params mismatch')
        with torch.cuda.device(self.device):
            out = torch.empty((p.shape[0], 3, 4), dtype=torch.float32, device=self.device)
            abi.check(self._lib.syn_pose_matrix(self._h, p.data_ptr(), p.shape[0], out.data_ptr(), self._stream()))
        return out

    # numpy single-face helpers with the reference's names and return types (utils/inference.py:140-157)
    def predict_sparseVert(self, param, roi_box, transform=False):
        return self._predict_vertices(param, roi_box, False, transform)

    def predict_denseVert(self, param, roi_box, transform=False):
        return self._predict_vertices(param, roi_box, True, transform)

    def _predict_vertices(self, param, roi_box, dense, transform):
        p = np.asarray(param, dtype=np.float32).reshape(1, -1)
        if p.shape[1] != 62:
            raise RuntimeError('length of params mismatch')
        roi = np.asarray(roi_box, dtype=np.float32).reshape(1, 5)
        return self.reconstruct(p, roi=roi, dense=dense, transform=transform)[0].cpu().numpy()

    def predict_pose(self, param, roi_bbox, ret_mat=False):
        p = np.asarray(param, dtype=np.float32).reshape(1, -1)
        if ret_mat:
            return self.pose_matrix_batch(p)[0].cpu().numpy()
        roi = np.asarray(roi_bbox, dtype=np.float32).reshape(1, 5)
        ang, t3d = self.predict_pose_batch(p, roi)
        return [float(v) for v in ang[0].cpu().numpy()], t3d[0].cpu().numpy()

    def crop_resize(self, frame, boxes, xofs, xcoef, yofs, ycoef, out=None):
        """crop_img + cv2.resize(INTER_LANCZOS4) of B detections of one uint8 frame [H,W,3] on the device
        (syn_crop_resize); returns uint8 crops [B,120,120,3] on the device (written into `out` when given).
        frame / tables may be numpy arrays or tensors (device tensors are used in place)."""
        fr = frame if isinstance(frame, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(frame))
        if fr.dtype != torch.uint8 or fr.dim() != 3 or fr.shape[2] != 3:
            raise RuntimeError('frame must be uint8 [H,W,3]')
        fr = fr.to(self.device).contiguous()

        def dev(a, dt):
            if isinstance(a, torch.Tensor):
                return a.to(device=self.device, dtype=dt).contiguous()
            return torch.as_tensor(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.int16: np.int16}[dt])).to(self.device)
        bx, xo, xc, yo, yc = dev(boxes, torch.int32), dev(xofs, torch.int32), dev(xcoef, torch.int16), dev(yofs, torch.int32), dev(ycoef, torch.int16)
        B = bx.shape[0]
        if (bx.dim() != 2 or bx.shape[1] != 4 or tuple(xo.shape) != (B, 120) or tuple(yo.shape) != (B, 120) or
                tuple(xc.shape) != (B, 120, 8) or tuple(yc.shape) != (B, 120, 8)):
            raise RuntimeError('crop_resize: boxes [B,4], xofs/yofs [B,120], xcoef/ycoef [B,120,8] expected')
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((B, 120, 120, 3), dtype=torch.uint8, device=self.device)
            elif tuple(out.shape) != (B, 120, 120, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
                raise RuntimeError('crop_resize: out must be a contiguous uint8 [B,120,120,3] tensor on the model device')
            abi.check(self._lib.syn_crop_resize(self._h, fr.data_ptr(), fr.shape[0], fr.shape[1], bx.data_ptr(), xo.data_ptr(),
                                                xc.data_ptr(), yo.data_ptr(), yc.data_ptr(), out.data_ptr(), B, self._stream()))
        return out

    # ---- host staging: page-locked buffers (torch's caching host allocator recycles them), so every transfer is ONE asynchronous DMA
    def _pinned_like(self, arr: np.ndarray) -> torch.Tensor:
        t = torch.empty(arr.shape, dtype=torch.from_numpy(arr[:0] if arr.ndim else arr).dtype, pin_memory=True)
        t.numpy()[...] = arr
        return t

    def _roi_and_box(self, rect):
        """The box arithmetic of get_all_outputs, verbatim in meaning (reference synergy3DMM.py:178-185): the detection list is
        aliased and MUTATED into the enlarged square ROI like the reference does; returns (roi5 floats, rounded crop box)."""
        roi_box = rect
        HCenter = (rect[1] + rect[3]) / 2
        WCenter = (rect[0] + rect[2]) / 2
        side_len = roi_box[3] - roi_box[1]
        margin = side_len * 1.2 // 2
        roi_box[0], roi_box[1], roi_box[2], roi_box[3] = WCenter - margin, HCenter - margin, WCenter + margin, HCenter + margin
        sx, sy, ex, ey = [int(round(v)) for v in roi_box[:4]]             # crop_img's rounding (utils/inference.py:98)
        if ex - sx <= 0 or ey - sy <= 0:
            raise ValueError('degenerate detection box')
        return [float(v) for v in roi_box[:5]], (sx, sy, ex, ey)

    @staticmethod
    def _chunks(counts, chunk_faces):
        """Consecutive frames -> chunks (frame_lo, frame_hi, face_lo, face_hi): every chunk holds at least chunk_faces faces (a chunk
        costs a small-batch forward of its own), the frames are never split, a call below 2 x chunk_faces faces is one chunk."""
        chunk_faces, n = max(1, int(chunk_faces)), int(sum(counts))
        chunks, f_lo, lo, acc = [], 0, 0, 0
        for fi, c in enumerate(counts):
            acc += c
            if acc >= chunk_faces and n - (lo + acc) >= chunk_faces:
                chunks.append((f_lo, fi + 1, lo, lo + acc))
                f_lo, lo, acc = fi + 1, lo + acc, 0
        chunks.append((f_lo, len(counts), lo, n))
        return chunks

    @staticmethod
    def _face_tables(rects, n):
        """_roi_and_box + the Lanczos tap tables for ALL faces of a call in array arithmetic (the per-face Python loop was 9 of the
        ~21 us of host work per face): the same IEEE double operations in the same order as the scalar code -- `//` is floor division
        on doubles, round() and numpy's rint both round halves to even -- so the results are the same bits
        (tests/test_host_cpu.py::test_face_tables_equal_the_per_face_arithmetic).  The detection lists are mutated into the ROI as before."""
        from .inference import lanczos4_tables
        flat = [r for fr in rects for r in fr]
        # the scalar statement computes in the type of the detections' elements: Python floats / float64 -> double, numpy float32 scalars
        # (what FaceBoxes returns, here and in the reference) -> float32 (NumPy 2: `np.float32 * 1.2` stays float32).  The array form
        # follows suit; anything mixed goes through the scalar statement itself (all-double arithmetic moved 1 crop box in 10^4
        # by a pixel for float32 detections)
        kinds = {type(x) for r in flat for x in r[:4]}
        if kinds <= {np.float32}:
            if int(np.__version__.split('.')[0]) < 2:
                # NumPy 1.x promotes `np.float32 scalar * 1.2` to float64 but keeps a float32 ARRAY float32: the array form would no longer
                # be the scalar statement's arithmetic -- take the scalar statement itself there
                return SynergyNet._face_tables_scalar(flat, n)
            dt = np.float32
        elif kinds <= {float, int, np.float64}:
            dt = np.float64
        else:
            return SynergyNet._face_tables_scalar(flat, n)
        d = np.array([r[:5] for r in flat], dtype=dt).reshape(n, 5)
        hc = (d[:, 1] + d[:, 3]) / 2
        wc = (d[:, 0] + d[:, 2]) / 2
        margin = np.floor_divide((d[:, 3] - d[:, 1]) * 1.2, 2)
        r4 = np.stack([wc - margin, hc - margin, wc + margin, hc + margin], axis=1)
        b4 = np.rint(r4)
        if not np.all(np.isfinite(b4)) or np.any(np.abs(b4) > 2 ** 30):
            raise ValueError('degenerate detection box')
        box = b4.astype(np.int32)
        w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        if np.any(w <= 0) or np.any(h <= 0):
            raise ValueError('degenerate detection box')
        vals = r4.tolist() if dt is np.float64 else [list(v) for v in r4]      # (float32 detections keep float32 scalars, as the scalar statement does)
        for r, v in zip(flat, vals):
            r[0], r[1], r[2], r[3] = v
        roi = np.concatenate([r4, d[:, 4:5]], axis=1).astype(np.float32)
        return SynergyNet._tap_tables(roi, box, w, h, n)

    @staticmethod
    def _face_tables_scalar(flat, n):
        """_face_tables for detections of mixed element types: the scalar statement (_roi_and_box) per face."""
        rb = [SynergyNet._roi_and_box(None, r) for r in flat]
        roi = np.array([x[0] for x in rb], dtype=np.float32).reshape(n, 5)
        box = np.array([x[1] for x in rb], dtype=np.int32).reshape(n, 4)
        return SynergyNet._tap_tables(roi, box, box[:, 2] - box[:, 0], box[:, 3] - box[:, 1], n)

    @staticmethod
    def _tap_tables(roi, box, w, h, n):
        from .inference import lanczos4_tables
        sides, inv = np.unique(np.concatenate([w, h]), return_inverse=True)
        tabs = [lanczos4_tables(int(sd)) for sd in sides]
        o_u = np.stack([t[0] for t in tabs])
        c_u = np.stack([t[1] for t in tabs])
        ofs = o_u[inv].reshape(2, n, 120).astype(np.int32, copy=False)
        coef = c_u[inv].reshape(2, n, 120, 8).astype(np.int16, copy=False)
        return roi, box, ofs, coef

    def _detector(self):
        if self.face_detector is None:
            # the reference builds FaceBoxes() on every call (:170-171); here once, on first use (HIP kernels,
            # synergynet_amd/faceboxes.py; needs FaceBoxes/weights/FaceBoxesProd.pth or model.face_detector = FaceBoxes(state_dict=...))
            from .faceboxes import FaceBoxes
            self.face_detector = FaceBoxes(device=self.device)
        return self.face_detector

    def _detect(self, frame):
        return self._detector()(frame)

    def _detect_frames(self, frames):
        """One detection list per frame: all frames in one call_batch when the detector has it (the HIP FaceBoxes: identical rows), else
        frame by frame -- a user's own detector is any callable."""
        det = self._detector()
        if hasattr(det, 'call_batch'):
            return det.call_batch(frames)
        return [det(f) for f in frames]

    def get_all_outputs_batch(self, frames, rects=None, dense=True, chunk_faces=64, refine=False):
        """get_all_outputs for a LIST of frames: every face of every frame goes through ONE backbone forward, ONE
        reconstruction and ONE download.  frames: uint8 BGR [H,W,3] arrays (sizes may differ); rects: per frame a list of
        detections [xmin,ymin,xmax,ymax,score] (mutated into the ROI like get_all_outputs does), or None -> the face detector: all frames in
        one `call_batch` when it has that method (the HIP FaceBoxes), else face_detector(frame) per frame.
        Returns a list with one (pts_res, vertices_lst, poses) triple per frame, each exactly what get_all_outputs returns
        (dense=False: vertices_lst is empty -- landmarks + pose only).  The returned arrays of a call are contiguous float32 views
        into page-locked host blocks allocated for this call and owned by the arrays (freed when the last one is dropped).
        chunk_faces: from 2 x chunk_faces faces on, the frames go through the device in chunks of at least that many faces so that the
        host staging of a chunk overlaps the device work and the downloads of the one before (same results: faces are independent;
        16 full-HD frames x 8 faces: 4.35 -> 3.53 ms per call with two chunks; chunks of 32 / 16 faces: 5.1 / 6.0 ms -- a chunk costs a
        small-batch forward of its own, ~0.4 ms).
        refine: pts_res holds the REFINED landmarks (refine_landmarks, image space) instead of the coarse ones; meshes and poses are
        unchanged.  RuntimeError when the synergy weights were not loaded."""
        if refine:
            self._need_synergy()
        from .inference import lanczos4_tables
        import time
        t_start = time.perf_counter()
        frames = list(frames)
        if rects is None:
            rects = self._detect_frames(frames)
        if len(rects) != len(frames):
            raise ValueError('rects must hold one detection list per frame')
        counts = [len(r) for r in rects]
        n = int(sum(counts))
        empty = lambda: ([], [], [])
        if n == 0:
            return [empty() for _ in frames]
        # per-face host tables: ROI (float32, as the reference's numpy arithmetic sees it), rounded box, Lanczos tap tables by crop side
        roi, box, ofs, coef = self._face_tables(rects, n)
        # Chunks of consecutive frames (>= chunk_faces faces each; one chunk below 2 x chunk_faces): while the device crops / runs /
        # downloads chunk k (downloads on a stream of their own, behind an event), the host stages chunk k + 1 into its page-locked
        # block -- the 37 MB memcpy of 16 full-HD frames and the 82 MB mesh download were one after the other before.
        chunks = self._chunks(counts, chunk_faces)
        tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.int16): torch.int16, np.dtype(np.int64): torch.int64}
        with torch.cuda.device(self.device):
            host = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
            lmk_h = host((n, 3, self._n_lmk), torch.float32)
            ang_h, t3d_h = host((n, 3), torch.float64), host((n, 3), torch.float32)
            mesh_h = host((n, 3, self._n_vert), torch.float32) if dense else None
            s_c = torch.cuda.current_stream(self.device)
            s_d = _download_stream(self.device) if len(chunks) > 1 else s_c
            for (fa, fb, lo, hi) in chunks:
                m = hi - lo
                # ONE page-locked staging block for everything of the chunk that goes up -- the frames that hold a face and the per-face
                # tables -- and one DMA (a block, a copy call and a crop launch per frame were half of the call's host time at 16 frames)
                used = [(i, np.ascontiguousarray(frames[i])) for i in range(fa, fb) if counts[i]]
                for _, fr in used:
                    if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
                        raise RuntimeError('frame must be uint8 [H,W,3]')
                slot = {i: k for k, (i, _) in enumerate(used)}
                fidx = np.repeat(np.array([slot.get(i, 0) for i in range(fa, fb)], dtype=np.int32), counts[fa:fb])
                fdim = np.array([fr.shape[:2] for _, fr in used], dtype=np.int32)
                total = 0

                def place(nbytes):
                    nonlocal total
                    at = total
                    total = (at + nbytes + 255) & ~255
                    return at
                foff = np.array([place(fr.nbytes) for _, fr in used], dtype=np.int64)
                tables = [np.ascontiguousarray(roi[lo:hi]), np.ascontiguousarray(box[lo:hi]), np.ascontiguousarray(ofs[:, lo:hi]),
                          np.ascontiguousarray(coef[:, lo:hi]), foff, fdim, fidx]
                t_at = [place(a.nbytes) for a in tables]
                stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
                sv = stage.numpy()
                for at, (_, fr) in zip(foff, used):
                    sv[at:at + fr.nbytes] = fr.reshape(-1)
                for at, a in zip(t_at, tables):
                    sv[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
                dev_blk = stage.to(self.device, non_blocking=True)
                roi_d, box_d, ofs_d, coef_d, foff_d, fdim_d, fidx_d = [dev_blk[at:at + a.nbytes].view(tdt[a.dtype]).view(a.shape) for at, a in zip(t_at, tables)]
                crops = torch.empty((m, 120, 120, 3), dtype=torch.uint8, device=self.device)
                abi.check(self._lib.syn_crop_resize_frames(self._h, dev_blk.data_ptr(), foff_d.data_ptr(), fdim_d.data_ptr(), fidx_d.data_ptr(),
                                                           box_d.data_ptr(), ofs_d[0].data_ptr(), coef_d[0].data_ptr(), ofs_d[1].data_ptr(),
                                                           coef_d[1].data_ptr(), crops.data_ptr(), m, self._stream()))
                if refine:
                    param, pool = self.forward_crops_u8(crops, return_pool=True)
                else:
                    param = self.forward_crops_u8(crops)
                lmk_d, (ang_d, t3d_d) = self.landmarks_and_pose(param, roi=roi_d, transform=True)
                if refine:
                    # the call above stays: it is where the pose comes from (the same bits as without refine).  Its coarse landmarks are
                    # replaced here; syn_refine_landmarks rebuilds Lc in crop space itself (one more launch of the ~6 us landmark kernel,
                    # next to ~70 MFLOP per face of MLP work)
                    lmk_d = self.refine_landmarks(param, pool, roi=roi_d, transform=True)
                mesh_d = None
                if dense:
                    # packed rows on the device (the kernel's guarded store path; 0.04 us per face more than pitched rows), so that the
                    # download is one contiguous DMA and every face's (3, 53215) array is a contiguous view of the host block
                    mesh_d = torch.empty((m, 3, self._n_vert), dtype=torch.float32, device=self.device)
                    self.reconstruct(param, roi=roi_d, dense=True, transform=True, out=mesh_d)
                if s_d is not s_c:
                    ev = torch.cuda.Event()
                    ev.record(s_c)
                    s_d.wait_event(ev)
                with torch.cuda.stream(s_d):
                    lmk_h[lo:hi].copy_(lmk_d, non_blocking=True)
                    ang_h[lo:hi].copy_(ang_d, non_blocking=True)
                    t3d_h[lo:hi].copy_(t3d_d, non_blocking=True)
                    if dense:
                        mesh_h[lo:hi].copy_(mesh_d, non_blocking=True)
                if s_d is not s_c:
                    for t in (lmk_d, ang_d, t3d_d, mesh_d):
                        if t is not None:
                            t.record_stream(s_d)
            t_enq = time.perf_counter()
            s_c.synchronize()
            if s_d is not s_c:
                s_d.synchronize()
            t_dev = time.perf_counter()
        lmk, ang, t3d = lmk_h.numpy(), ang_h.numpy().tolist(), t3d_h.numpy()
        mesh = mesh_h.numpy() if dense else None
        out, k = [], 0
        for c in counts:
            pts_res = [lmk[i] for i in range(k, k + c)]
            vertices_lst = [mesh[i] for i in range(k, k + c)] if dense else []
            poses = [[ang[i], t3d[i]] for i in range(k, k + c)]
            out.append((pts_res, vertices_lst, poses))
            k += c
        # where the call's wall time went: host work (tables, staging, enqueueing, result lists) vs waiting for the device + DMA
        t_end = time.perf_counter()
        self.last_timing = dict(faces=n, host_s=(t_enq - t_start) + (t_end - t_dev), device_wait_s=t_dev - t_enq)
        return out

    # ------------------------------------------------------------------ detections -> crop tables on the device
    def lanczos4_tables_device(self, sides):
        """inference.lanczos4_tables(side, 120) for n crop sides at once, on the device (syn_lanczos4_tables): sides int32 [n] (tensor or
        array, each >= 1) -> (ofs [n,120] int32, coef [n,120,8] int16) device tensors, the host function's integers.  Reads the sides
        back to refuse one below 1 (it synchronises); the per-face path, `face_tables`, does not."""
        s = sides if isinstance(sides, torch.Tensor) else torch.as_tensor(np.asarray(sides))
        if s.dim() != 1 or s.dtype.is_floating_point:
            raise RuntimeError('sides must be a vector of integers')
        s = s.to(device=self.device, dtype=torch.int32).contiguous()
        n = s.shape[0]
        with torch.cuda.device(self.device):
            ofs = torch.empty((n, 120), dtype=torch.int32, device=self.device)
            coef = torch.empty((n, 120, 8), dtype=torch.int16, device=self.device)
            abi.check(self._lib.syn_lanczos4_tables(self._h, s.data_ptr(), n, ofs.data_ptr(), coef.data_ptr(), self._stream()))
        return ofs, coef

    def face_tables(self, dets):
        """_face_tables on the device for float32 detections [n,5] (x1, y1, x2, y2, score) that are already there (syn_face_tables; a
        host array is uploaded): -> (roi [n,5] float32, box [n,4] int32, ofs [2,n,120] int32, coef [2,n,120,8] int16 -- x tables then y
        tables -- status [n] int32), device tensors with the bits _face_tables returns for lists of np.float32 scalars.  status is
        non-zero where _face_tables raises 'degenerate detection box' (that face gets box (0,0,1,1) and the taps of side 1; the
        others are unaffected); nothing synchronises, the caller reads status when it reads its results."""
        d = dets if isinstance(dets, torch.Tensor) else torch.as_tensor(np.asarray(dets))
        if d.dim() != 2 or d.shape[1] != 5 or d.dtype != torch.float32:
            raise RuntimeError('dets must be float32 [n,5] (x1, y1, x2, y2, score)')
        d = d.to(self.device).contiguous()
        n = d.shape[0]
        with torch.cuda.device(self.device):
            roi = torch.empty((n, 5), dtype=torch.float32, device=self.device)
            box = torch.empty((n, 4), dtype=torch.int32, device=self.device)
            ofs = torch.empty((2, n, 120), dtype=torch.int32, device=self.device)
            coef = torch.empty((2, n, 120, 8), dtype=torch.int16, device=self.device)
            status = torch.empty((n,), dtype=torch.int32, device=self.device)
            abi.check(self._lib.syn_face_tables(self._h, d.data_ptr(), n, roi.data_ptr(), box.data_ptr(), ofs[0].data_ptr(), coef[0].data_ptr(),
                                                ofs[1].data_ptr(), coef[1].data_ptr(), status.data_ptr(), self._stream()))
        return roi, box, ofs, coef, status

    def get_all_outputs_frames(self, frames, dense=True, refine=False, to_host=True):
        """get_all_outputs_batch(frames) with the detections kept on the device from the detector's last kernel to the crop kernel's
        first: the frames are staged ONCE, size group after size group, into one page-locked block and go up with one copy; the
        detector runs on views of that block (`detect_faces`), the only traffic to the host before the results is the N + 1 face
        counts (one synchronisation, to size the batch), the ROI / box / Lanczos tables are computed there (`face_tables`) and
        syn_crop_resize_frames crops from the same block.  No chunking (get_all_outputs_batch overlaps staging and downloads from 128
        faces on; this call does not).
        to_host=True: exactly the list of (pts_res, vertices_lst, poses) triples get_all_outputs_batch(frames) returns, same bits.
        to_host=False: a dict of device tensors for the whole call -- lmk [n,3,68], angles [n,3] float64, t3d [n,3], mesh [n,3,n_vert]
        or None, roi [n,5], face_frame [n] int32 (faces are in frame order) -- and frame_faces, the faces per frame, as a host list.
        ValueError('degenerate detection box') after the final synchronisation when any face's box is degenerate.
        A face_detector without `detect_faces` (a user's callable): get_all_outputs_batch does the work (to_host=True only)."""
        if refine:
            self._need_synergy()
        det = self._detector()
        if not hasattr(det, 'detect_faces'):
            if not to_host:
                raise RuntimeError('get_all_outputs_frames(to_host=False) needs a face detector with detect_faces (the HIP FaceBoxes)')
            return self.get_all_outputs_batch(frames, dense=dense, refine=refine)
        import time
        from .faceboxes import group_by_size
        t_start = time.perf_counter()
        frames = [np.ascontiguousarray(f) for f in frames]
        for fr in frames:
            if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
                raise RuntimeError('frame must be uint8 [H,W,3]')
        N = len(frames)
        empty = lambda: ([], [], [])
        if N == 0:
            return [] if to_host else self._frames_result_device(0, dense, [])
        # ONE page-locked block: the frames, each size group contiguous (one [m,H,W,3] view for the detector), then where each INPUT
        # frame lies (byte offset, height and width: the crop kernel's frame tables)
        total = 0

        def place(nbytes):
            nonlocal total
            at = total
            total = (at + nbytes + 255) & ~255
            return at
        foff = np.zeros(N, dtype=np.int64)
        for (h, w), pos in group_by_size([f.shape for f in frames]):
            at = place(len(pos) * h * w * 3)
            foff[pos] = at + np.arange(len(pos), dtype=np.int64) * (h * w * 3)
        fdim = np.array([fr.shape[:2] for fr in frames], dtype=np.int32)
        t_at = [place(foff.nbytes), place(fdim.nbytes)]
        with torch.cuda.device(self.device):
            stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            sv = stage.numpy()
            for at, fr in zip(foff, frames):
                sv[at:at + fr.nbytes] = fr.reshape(-1)
            for at, a in zip(t_at, (foff, fdim)):
                sv[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
            dev_blk = stage.to(self.device, non_blocking=True)
            foff_d = dev_blk[t_at[0]:t_at[0] + foff.nbytes].view(torch.int64)
            fdim_d = dev_blk[t_at[1]:t_at[1] + fdim.nbytes].view(torch.int32)
            views = [dev_blk[at:at + fr.nbytes].view(fr.shape) for at, fr in zip(foff.tolist(), frames)]
            rows, face_frame, frame_faces = det.detect_faces(views)
            ff_h = torch.empty((N + 1,), dtype=torch.int32, pin_memory=True)
            ff_h.copy_(frame_faces, non_blocking=True)
            s_c = torch.cuda.current_stream(self.device)
            t_enq0 = time.perf_counter()
            s_c.synchronize()
            t_dev0 = time.perf_counter()
            counts = ff_h[:N].tolist()
            n = int(ff_h[N])
            if n == 0:
                self.last_timing = dict(faces=0, host_s=(t_enq0 - t_start) + (time.perf_counter() - t_dev0), device_wait_s=t_dev0 - t_enq0)
                return [empty() for _ in frames] if to_host else self._frames_result_device(N, dense, counts)
            face_frame = face_frame[:n]
            roi_d, box_d, ofs_d, coef_d, status_d = self.face_tables(rows[:n])
            crops = torch.empty((n, 120, 120, 3), dtype=torch.uint8, device=self.device)
            abi.check(self._lib.syn_crop_resize_frames(self._h, dev_blk.data_ptr(), foff_d.data_ptr(), fdim_d.data_ptr(), face_frame.data_ptr(),
                                                       box_d.data_ptr(), ofs_d[0].data_ptr(), coef_d[0].data_ptr(), ofs_d[1].data_ptr(),
                                                       coef_d[1].data_ptr(), crops.data_ptr(), n, self._stream()))
            if refine:
                param, pool = self.forward_crops_u8(crops, return_pool=True)
            else:
                param = self.forward_crops_u8(crops)
            lmk_d, (ang_d, t3d_d) = self.landmarks_and_pose(param, roi=roi_d, transform=True)
            if refine:          # as in get_all_outputs_batch: the pose comes from the call above, the landmarks are replaced
                lmk_d = self.refine_landmarks(param, pool, roi=roi_d, transform=True)
            mesh_d = None
            if dense:
                mesh_d = torch.empty((n, 3, self._n_vert), dtype=torch.float32, device=self.device)
                self.reconstruct(param, roi=roi_d, dense=True, transform=True, out=mesh_d)
            host = lambda t: torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            status_h = host(status_d)
            status_h.copy_(status_d, non_blocking=True)
            if to_host:
                lmk_h, ang_h, t3d_h = host(lmk_d), host(ang_d), host(t3d_d)
                mesh_h = host(mesh_d) if dense else None
                lmk_h.copy_(lmk_d, non_blocking=True)
                ang_h.copy_(ang_d, non_blocking=True)
                t3d_h.copy_(t3d_d, non_blocking=True)
                if dense:
                    mesh_h.copy_(mesh_d, non_blocking=True)
            t_enq = time.perf_counter()
            s_c.synchronize()
            t_dev = time.perf_counter()
        if status_h.numpy().any():
            raise ValueError('degenerate detection box')
        if to_host:
            lmk, ang, t3d = lmk_h.numpy(), ang_h.numpy().tolist(), t3d_h.numpy()
            mesh = mesh_h.numpy() if dense else None
            out, k = [], 0
            for c in counts:
                pts_res = [lmk[i] for i in range(k, k + c)]
                vertices_lst = [mesh[i] for i in range(k, k + c)] if dense else []
                poses = [[ang[i], t3d[i]] for i in range(k, k + c)]
                out.append((pts_res, vertices_lst, poses))
                k += c
        else:
            out = dict(lmk=lmk_d, angles=ang_d, t3d=t3d_d, mesh=mesh_d, roi=roi_d, face_frame=face_frame, frame_faces=counts)
        t_end = time.perf_counter()
        self.last_timing = dict(faces=n, host_s=(t_enq0 - t_start) + (t_enq - t_dev0) + (t_end - t_dev),
                                device_wait_s=(t_dev0 - t_enq0) + (t_dev - t_enq))
        return out

    def _frames_result_device(self, N, dense, counts):
        """get_all_outputs_frames(to_host=False) of a call without a face: empty tensors of the right shapes, no launch."""
        e = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=self.device)
        return dict(lmk=e((0, 3, self._n_lmk)), angles=e((0, 3), torch.float64), t3d=e((0, 3)), mesh=e((0, 3, self._n_vert)) if dense else None,
                    roi=e((0, 5)), face_frame=e((0,), torch.int32), frame_faces=list(counts))

    def get_all_outputs(self, input, rects=None, refine=False):
        """reference synergy3DMM.py:167-207: BGR uint8 image [H,W,3] -> (list of (3,68) landmarks,
        list of (3,53215) meshes, list of [angles_deg, translation]) with one entry per face.

        All faces of the image go through ONE batched launch chain instead of the reference's
        per-face loop (get_all_outputs_batch with one frame).  `rects` = detections [[xmin,ymin,xmax,ymax,score], ...];
        when omitted the `face_detector(image)` is called -- by default the HIP FaceBoxes of synergynet_amd/faceboxes.py (the
        reference constructs FaceBoxes here, :170-171)."""
        if rects is None:
            rects = self._detect(input)
        return self.get_all_outputs_batch([input], [rects], refine=refine)[0]
