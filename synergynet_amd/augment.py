"""Train-time augmentation on the device: the reference's training transform, main_train.py:199-208

    Compose_GT([ColorJitter(0.4, 0.4, 0.4), ToTensor(), CenterCrop(5), Normalize(mean=127.5, std=128)])

on a uint8 set that lives on the device, one launch per batch (syn_train_transform_u8), bit for bit what utils/ddfa.py and PIL produce for
the same draws.  The random draws stay on the host -- a few numbers per face -- and follow the reference's order, so a seeded
single-worker loop of the reference and `draw_records` choose the same factors, orders and masks.

  draw_records(B, ...)        the per-face records (factors, order of the steps, mask kind) as a numpy structured array
  TrainTransform(model, ...)  (crops_u8, index=None, records=None, out='f32' | 'u8' | 'both') -> device tensors
  train_batches(...)          (input, target[:, :62].float()) per batch over torch.randperm(N): this library's own order, not DataLoader's

Out of scope: hue (the reference trains with hue 0), file decoding, DataLoader's sampling order.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import abi

RECORD_DTYPE = np.dtype([('src_index', '<i4'), ('factor', '<f4', (3,)), ('op', 'u1', (3,)), ('mask', 'u1')])   # syn_train_record, 20 bytes
OP_SKIP, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION = 0, 1, 2, 3
assert RECORD_DTYPE.itemsize == 20


def draw_records(B, brightness=0.4, contrast=0.4, saturation=0.4, prob=0.01, np_random=np.random, py_random=random):
    """B records drawn as the reference draws per sample (utils/ddfa.py ColorJitter.get_params, then CenterCrop.get_params / __call__):
    one np_random.uniform(max(0, 1 - a), 1 + a) per enabled step in the order brightness, contrast, saturation; one np_random.shuffle of
    the list of enabled steps; py_random.random(); py_random.randint(1, 7) only when that draw was below `prob`.  src_index = 0 .. B - 1."""
    rec = np.zeros((int(B),), dtype=RECORD_DTYPE)
    rec['src_index'] = np.arange(int(B), dtype=np.int32)
    for i in range(int(B)):
        steps = []
        for op, a in ((OP_BRIGHTNESS, brightness), (OP_CONTRAST, contrast), (OP_SATURATION, saturation)):
            if a > 0:
                steps.append((op, np_random.uniform(max(0, 1 - a), 1 + a)))
        order = list(range(len(steps)))
        np_random.shuffle(order)
        for j, k in enumerate(order):
            rec['op'][i, j], rec['factor'][i, j] = steps[k][0], np.float32(steps[k][1])
        if py_random.random() < prob:
            rec['mask'][i] = py_random.randint(1, 7)
    return rec


def check_records(records, n_src):
    """The host-side validation before an upload: the kernel turns a bad record into an all-zero face, this names it instead."""
    r = np.ascontiguousarray(records)
    if r.dtype != RECORD_DTYPE or r.ndim != 1 or r.shape[0] < 1:
        raise ValueError('records must be a non-empty 1-d array of augment.RECORD_DTYPE')
    if (r['op'] > 3).any():
        raise ValueError('records: op must be 0 (skip), 1 (brightness), 2 (contrast) or 3 (saturation)')
    if (r['mask'] > 7).any():
        raise ValueError('records: mask must be 0..7')
    if not np.isfinite(r['factor']).all():
        raise ValueError('records: factors must be finite')
    if ((r['src_index'] < 0) | (r['src_index'] >= n_src)).any():
        raise ValueError(f'records: src_index must lie in [0, {n_src})')
    return r


class TrainTransform:
    """ColorJitter(brightness, contrast, saturation) -> ToTensor -> CenterCrop(margin, prob, mode='train') -> Normalize(mean, std) of the
    reference on a resident uint8 set [N,H,W,3] (keep it on the model's device: anything else is uploaded on every call).

        t = TrainTransform(model)
        x = t(crops_u8, index=idx)                 # [B,3,H,W] float32, B = len(idx) faces gathered by idx (default: all N in order)
        u = t(crops_u8, index=idx, out='u8')       # [B,H,W,3] uint8: the jittered, cropped, masked bytes for losses_crops_u8
        x, u = t(crops_u8, records=r, out='both')  # records of draw_records / RECORD_DTYPE instead of fresh draws

    Fresh draws come from `np_random` / `py_random` (default: the global numpy and python generators, as in the reference)."""

    def __init__(self, model, brightness=0.4, contrast=0.4, saturation=0.4, hue=0, margin=5, prob=0.01, mean=127.5, std=128,
                 np_random=np.random, py_random=random):
        if hue > 0:
            raise NotImplementedError(f'TrainTransform: hue={hue} is not supported (the reference trains with hue 0; the HSV path is not built)')
        if min(brightness, contrast, saturation) < 0 or hue < 0:
            raise ValueError('TrainTransform: brightness, contrast, saturation and hue must not be negative')
        if margin < 0:
            raise ValueError('TrainTransform: margin must not be negative')
        if not np.isfinite(mean) or not np.isfinite(std) or std == 0:
            raise ValueError('TrainTransform: mean must be finite, std finite and not 0')
        self.model = model
        self.brightness, self.contrast, self.saturation = brightness, contrast, saturation
        self.margin, self.prob, self.mean, self.std = int(margin), prob, float(mean), float(std)
        self.np_random, self.py_random = np_random, py_random

    def draw(self, B):
        return draw_records(B, self.brightness, self.contrast, self.saturation, self.prob, self.np_random, self.py_random)

    def __call__(self, crops_u8, index=None, records=None, out='f32'):
        if out not in ('f32', 'u8', 'both'):
            raise ValueError(f"out must be 'f32', 'u8' or 'both', got {out!r}")
        m = self.model
        x = crops_u8 if isinstance(crops_u8, torch.Tensor) else torch.as_tensor(np.asarray(crops_u8))
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or min(x.shape) < 1:
            raise ValueError('expected uint8 crops [N,H,W,3]')
        N, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        if 3 * H * W > abi.SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES:
            raise ValueError(f'a face of {3 * H * W} bytes does not fit one workgroup: at most {abi.SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES}')
        if index is not None:
            index = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index).astype(np.int64).reshape(-1)
        if records is None:
            records = self.draw(N if index is None else len(index))
        else:
            records = np.array(records, dtype=RECORD_DTYPE, copy=True)
        if index is not None:
            if len(index) != len(records):
                raise ValueError(f'index names {len(index)} faces, records {len(records)}')
            if ((index < 0) | (index >= N)).any():
                raise ValueError(f'index must lie in [0, {N})')
            records['src_index'] = index.astype(np.int32)
        records = check_records(records, N)
        B = records.shape[0]
        x = x.to(m.device).contiguous()
        with torch.cuda.device(m.device):
            rec = torch.from_numpy(records.view(np.uint8).reshape(B, RECORD_DTYPE.itemsize)).to(m.device)
            f32 = torch.empty((B, 3, H, W), dtype=torch.float32, device=m.device) if out != 'u8' else None
            u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=m.device) if out != 'f32' else None
            abi.check(m._lib.syn_train_transform_u8(m._h, x.data_ptr(), N, H, W, rec.data_ptr(), B, self.margin, self.mean, self.std,
                                                    f32.data_ptr() if f32 is not None else None,
                                                    u8.data_ptr() if u8 is not None else None, m._stream()))
        return f32 if out == 'f32' else u8 if out == 'u8' else (f32, u8)


def train_batches(model, crops_u8, targets, batch_size, transform, generator=None, drop_last=True, out='f32'):
    """One epoch: yields (input, target[:, :62].float()) on the model's device, `batch_size` faces each, in the order of
    torch.randperm(N, generator=generator) -- this library's own order, not claimed to be DataLoader's.  crops_u8 [N,H,W,3] uint8 and
    targets [N,>=62] are made resident once; every batch is one `transform` launch plus one gather of the targets.  drop_last as
    DataLoader: a last batch of fewer than batch_size faces is dropped (True) or yielded short (False)."""
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1')
    x = crops_u8 if isinstance(crops_u8, torch.Tensor) else torch.as_tensor(np.asarray(crops_u8))
    t = targets if isinstance(targets, torch.Tensor) else torch.as_tensor(np.asarray(targets))
    if t.dim() != 2 or t.shape[0] != x.shape[0] or t.shape[1] < 62:
        raise ValueError(f'targets must be [{x.shape[0]},>=62], got {tuple(t.shape)}')
    x, t = x.to(model.device).contiguous(), t.to(model.device)
    N = x.shape[0]
    perm = torch.randperm(N, generator=generator)
    for i in range(0, N, batch_size):
        idx = perm[i:i + batch_size]
        if len(idx) < batch_size and drop_last:
            return
        yield transform(x, index=idx, out=out), t[idx.to(model.device)][:, :62].float()
