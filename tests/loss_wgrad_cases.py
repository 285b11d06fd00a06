"""Shared by tests/test_loss_wgrad_cpu.py, tests/test_gpu_loss_wgrad.py and tests/golden/make_loss_wgrad_golden.py: the weight gradients
of the loss head from the torch restatement of tests/loss_grad_cases.py -- its `sd` tensors set to require grad --, the
wrong variants the bite tests hold against the recording, the face selection and the plain SGD steps.  CPU only."""
import os

import numpy as np
import torch

import loss_cases as lc
import loss_grad_cases as lg

GOLDEN = os.path.join(lg.HERE, 'golden', 'loss_wgrad_golden.npz')
TOL = lc.TOL                            # GPU bar: 1e-4 x max |g| of the tensor
CPU_BAR = lg.CPU_BAR                    # 1e-5 x max |g|
WHOLE_MAX = 4096                        # tensors up to this size are recorded whole
SAMPLE = 499                            # larger ones: every SAMPLE-th element (61 would put the fixture at 0.9 MB: 28 000 elements of
#                                         small tensors per loss are recorded whole, which alone is 450 KB of the 512 KB the fixture may have)
TIE_SAMPLE = 61
RECORDED = ('total', 'loss_LMK_pointNet', 'loss_Param_S2', 'loss_Param_S1S2')
ZERO_LOSSES = ('loss_LMK_f0', 'loss_Param_In')          # neither sees an MLP: every weight gradient is exactly 0
TIE_KEYS = ('forwardDirection.conv5.weight', 'forwardDirection.conv1.weight')
ORDERS = 3                              # random channel orders beside the native one (select_wgrad_faces)
SGD_STEPS, SGD_LR = 3, 1e-3


def layers():
    from synergynet_amd import synth
    return synth.synergy_layers()


def learnable_keys():
    return [k for k, _ in layers() if 'running_' not in k]


def flat_slices():
    """{key: (offset, shape)} of the FLAT layout of syn_load_synergy"""
    out, at = {}, 0
    for k, shape in layers():
        out[k] = (at, shape)
        at += int(np.prod(shape))
    return out


def recorded_part(a, sample=SAMPLE):
    a = np.asarray(a).reshape(-1)
    return a if a.size <= WHOLE_MAX else a[::sample]


def fixture_key(name, key):
    return f'w|{name}|{key}'


class WHead(lg.Head):
    """lg.Head whose learnable tensors require grad.  Wrong variants: pad_rows -- the 12 clamped copies of point 67 that pad a face's 68
    points to five tiles of 16 are COUNTED in every weight reduction over points (the values and the data gradients are unchanged);
    no_mean_term -- d gamma without the (bias - mean) s term."""

    def __init__(self, pack, sd, dtype=torch.float64, perm_seed=None, pad_rows=False, no_mean_term=False):
        super().__init__(pack, sd, dtype, perm_seed)
        self.pad_rows, self.no_mean_term = pad_rows, no_mean_term
        self.keys = learnable_keys()
        for k in self.keys:                                  # a copy: lg.Head's fp32 tensors share the caller's arrays, and sgd() writes
            self.sd[k] = self.sd[k].clone().requires_grad_(True)

    def _affine(self, s, prefix, conv, bn, x, order):
        W = s[f'{prefix}{conv}.weight'][:, :, 0]
        if order is not None:
            W, x = W[:, order].contiguous(), x[:, order].contiguous()
        inv = s[f'{prefix}{bn}.weight'] / torch.sqrt(s[f'{prefix}{bn}.running_var'] + 1e-5)
        off = s[f'{prefix}{conv}.bias'] - s[f'{prefix}{bn}.running_mean']
        y = torch.einsum('oi,bip->bop', W, x) * inv[None, :, None]
        return y + (off * (inv.detach() if self.no_mean_term else inv) + s[f'{prefix}{bn}.bias'])[None, :, None]

    def _layer(self, prefix, conv, bn, x):
        order = None if self.perm is None else torch.from_numpy(self.perm.permutation(x.shape[1]))
        y = self._affine(self.sd, prefix, conv, bn, x, order)
        if self.pad_rows and x.shape[2] == 68:
            frozen = {k: v.detach() for k, v in self.sd.items()}
            y_x, y_p = self._affine(frozen, prefix, conv, bn, x, order), self._affine(self.sd, prefix, conv, bn, x.detach(), order)
            w = torch.ones(68, dtype=self.dtype)
            w[67] = 13.0
            y = y_x + (y_p - y_p.detach()) * w
        if self.record is not None:
            self.record.append((prefix + conv, y.detach()))
        return torch.relu(y)

    def _grads(self, scalar, retain=False):
        g = torch.autograd.grad(scalar, [self.sd[k] for k in self.keys], retain_graph=retain, allow_unused=True)
        return {k: (np.zeros(tuple(self.sd[k].shape)) if x is None else x.numpy()) for k, x in zip(self.keys, g)}

    def wvjp(self, param, pool, target, g_scalars, g_per_face, **kw):
        """numpy inputs and upstream gradients -> {key: d sum_i <g_i, loss_i> / d tensor}"""
        t = lambda a: lg._t(a, self.dtype)
        L = self.losses(t(param), t(pool), t(target), **kw)
        gs, gp = t(g_scalars), t(g_per_face)
        return self._grads(gs[0] * L[0] + gs[1] * L[1] + sum((gp[i] * L[2 + i]).sum() for i in range(3)))

    def wgrads(self, param, pool, target, names=RECORDED, **kw):
        """{loss name: {key: gradient of the loss's .mean()}}; 'total' is the sum of the five means"""
        t = lambda a: lg._t(a, self.dtype)
        means = [v.mean() for v in self.losses(t(param), t(pool), t(target), **kw)]
        scal = dict(zip(lc.LOSS_NAMES + ('total',), means + [sum(means)]))
        return {n: self._grads(scal[n], retain=True) if scal[n].requires_grad else {k: np.zeros(tuple(self.sd[k].shape)) for k in self.keys}
                for n in names}

    def sgd(self, param, pool, target, steps=SGD_STEPS, lr=SGD_LR):
        """plain SGD on the sum of the five means -> [steps][5] float64: the five means after each step.  Changes self.sd."""
        t = lambda a: lg._t(a, self.dtype)
        out = []
        for _ in range(steps):
            g = self._grads(sum(v.mean() for v in self.losses(t(param), t(pool), t(target))))
            with torch.no_grad():
                for k in self.keys:
                    self.sd[k] -= lr * torch.from_numpy(g[k]).to(self.dtype)
                out.append([float(v.mean()) for v in self.losses(t(param), t(pool), t(target))])
        return np.array(out)


def total_upstream(B):
    """the NULL / NULL call: 1 for the scalars, 1 / B per face"""
    return np.ones(2, dtype=np.float32), np.full((3, B), np.float32(1.0) / np.float32(B), dtype=np.float32)


def worst_rel(got, want, keys=None):
    """(max over tensors of max |got - want| / max |want|, its key); a tensor whose expected maximum is 0 must be exactly 0"""
    worst, at = 0.0, ''
    for k in (keys or want):
        w = np.asarray(want[k], dtype=np.float64)
        g = np.asarray(got[k], dtype=np.float64).reshape(w.shape)
        if not np.any(w[np.isfinite(w)] != 0):
            assert not np.any(g[np.isfinite(w)] != 0), (k, 'expected exactly 0')
            continue
        r = lg.rel_to_max(g, w)
        if r > worst:
            worst, at = r, k
    return worst, at


def select_wgrad_faces(pack, sd, batch_faces):
    """the batch_faces whose own weight gradients (upstream 1 for all five losses) from the fp32 restatement, in the native order and in
    ORDERS random channel orders, meet float64 within CPU_BAR x max |g| of every tensor -> (indices into the candidates, {rejected: why})"""
    param, pool, target = lg.candidate_inputs()
    h64 = WHead(pack, sd)
    h32 = [WHead(pack, sd, torch.float32, perm_seed=s if s else None) for s in range(ORDERS + 1)]
    gs, gp = np.ones(2, dtype=np.float32), np.ones((3, 1), dtype=np.float32)
    chosen, rejected = [], {}
    for b in (int(x) for x in np.asarray(batch_faces)):
        one = (param[b:b + 1], pool[b:b + 1], target[b:b + 1], gs, gp)
        want = h64.wvjp(*one)
        worst = max(worst_rel(h.wvjp(*one), want) for h in h32)
        if worst[0] > CPU_BAR:
            rejected[b] = '%.1e on %s' % worst
        else:
            chosen.append(b)
    return np.array(chosen), rejected


def wgrad_inputs(faces, B):
    param, pool, target = lg.candidate_inputs()
    f = np.asarray(faces)[:B]
    return param[f], pool[f], target[f]


def split_flat(flat):
    """flat [syn_synergy_flat_count()] -> {key: array in the reference's shape}, running statistics included"""
    return {k: np.asarray(flat[at:at + int(np.prod(shape))]).reshape(shape) for k, (at, shape) in flat_slices().items()}
