"""Shared by tests/test_loss_train_cpu.py, tests/test_gpu_loss_train.py and tests/golden/make_loss_train_golden.py: a torch-CPU restatement
(float64 unless a dtype is asked for) of the loss head with every BatchNorm1d of MLP_for / MLP_rev in train() -- batch statistics for the
normalisation, the running update with the unbiased variance -- written from the formulas of DESIGN 5.21 on top of the eval() Head of
tests/loss_grad_cases.py, with the wrong variants the bite tests hold against the recording, the edge state and the fixture's keys."""
import os

import numpy as np
import torch

import loss_cases as lc
import loss_grad_cases as lg

GOLDEN = os.path.join(lg.HERE, 'golden', 'loss_train_golden.npz')
TOL = lc.TOL                            # GPU bar: losses relative, statistics relative to the max of their tensor
CPU_BAR = lg.CPU_BAR                    # restatement against the recording, fp32 against fp64 in the generator
BATCHES = (2, 3, 5, 17)                 # recorded: the first B of lg.candidate_inputs()
STATES = ('plain', 'edge')
MOMENTUM = 0.1                          # the reference's BatchNorm1d default
CALLS = 3                               # running statistics are recorded after one and after CALLS calls on the same batch
EPS = 1e-5
BN_CHANNELS = 3649
WRONG = ('norm_unbiased', 'running_biased', 'heads_n68', 'max_before_bn', 'conv6_point_stats')
# At B = 2 a head of MLP_rev normalises two values d apart to +-(d / 2) / sqrt(d d / 4 + 1e-5): a channel whose two pre-activations lie
# within ~0.03 of each other is not saturated and amplifies an fp32 rounding of z by up to gamma / (2 sqrt(1e-5)) = 158 gamma.  Which
# channels those are depends on which gammas the edge state flips; the seed is the first of 977.. for which the REFERENCE in fp32 meets
# the reference in float64 within CPU_BAR on S2 at every recorded batch (977 and 978 miss at B = 2 by 1.5e-4 and 8.4e-5 on one channel
# each; their losses and statistics agree like the others').  The generator asserts it; nothing of the library enters the choice.
SEED_EDGE = 979


def bn_order():
    """[(state_dict prefix of the BatchNorm, channels)] in the FLAT layout's order: forwardDirection.bn1..bn9, reverseDirection.bn1..bn5,
    bn6_1..bn6_3 -- the order of batch_stats"""
    from synergynet_amd import synth
    return [(p + bn, cout) for p, table in zip(synth.SYNERGY_PREFIXES, (synth.SYNERGY_FOR, synth.SYNERGY_REV)) for _, bn, _, cout in table]


def bn_offsets():
    out, at = {}, 0
    for name, n in bn_order():
        out[name] = (at, n)
        at += n
    assert at == BN_CHANNELS
    return out


def recorded_channels():
    """indices into the 3649 channels that the fixture keeps: every BatchNorm whole up to 256 channels, every 2nd channel of bn6 (512),
    every 16th of the two bn5 (1024) -- a statistic is per channel, so a sample checks the same arithmetic at a sixth of the bytes"""
    idx = []
    for name, (at, n) in bn_offsets().items():
        step = 1 if n <= 256 else 2 if n <= 512 else 16
        idx.append(at + np.arange(0, n, step))
    return np.concatenate(idx)


def edge_state(sd):
    """a copy of the state with one eighth (at least one) of every BatchNorm's gamma negated and one sixteenth (at least one) set to 0"""
    rng = np.random.default_rng(SEED_EDGE)
    out = dict(sd)
    for name, n in bn_order():
        g = np.array(sd[name + '.weight'], dtype=np.float32).copy()
        perm = rng.permutation(n)
        n_neg, n_zero = max(1, n // 8), max(1, n // 16)
        g[perm[:n_neg]] *= -1
        g[perm[n_neg:n_neg + n_zero]] = 0
        out[name + '.weight'] = g
    return out


def state_of(sd, which):
    return edge_state(sd) if which == 'edge' else dict(sd)


def inputs(B):
    param, pool, target = lg.candidate_inputs()
    return param[:B], pool[:B], target[:B]


def degenerate_inputs():
    """two identical faces: every head channel of MLP_rev has variance exactly 0"""
    param, pool, target = inputs(1)
    return np.repeat(param, 2, 0), np.repeat(pool, 2, 0), np.repeat(target, 2, 0)


class TrainHead(lg.Head):
    """lg.Head with _layer normalising by the statistics of the batch.  `momentum` None leaves the running statistics alone; otherwise
    self.sd's running_* tensors move with every call.  `wrong`: one of WRONG."""

    def __init__(self, pack, sd, dtype=torch.float64, momentum=MOMENTUM, wrong=None):
        super().__init__(pack, sd, dtype)
        assert wrong is None or wrong in WRONG
        self.momentum, self.wrong = momentum, wrong
        self.stats = None

    def _layer(self, prefix, conv, bn, x, pool_first=False):
        s = self.sd
        W = s[f'{prefix}{conv}.weight'][:, :, 0]
        bias = s[f'{prefix}{conv}.bias'][None, :, None]
        z = torch.einsum('oi,bip->bop', W, x) + bias
        zs = z
        if self.wrong == 'conv6_point_stats' and conv == 'conv6':
            zs = torch.einsum('oi,bip->bop', W[:, :64], x[:, :64]) + bias
        n = zs.shape[0] * zs.shape[2]
        mean, var = zs.mean((0, 2)), zs.var((0, 2), unbiased=False)
        nvar = var * n / (n - 1) if self.wrong == 'norm_unbiased' else var
        if self.stats is not None:
            self.stats.append((prefix + bn, mean.detach(), var.detach()))
        if self.momentum is not None:
            m = self.momentum
            nr = 68 * zs.shape[0] if (self.wrong == 'heads_n68' and 'conv6_' in conv) else n
            rvar = var if self.wrong == 'running_biased' else var * nr / (nr - 1)
            s[f'{prefix}{bn}.running_mean'] = (1 - m) * s[f'{prefix}{bn}.running_mean'] + m * mean.detach()
            s[f'{prefix}{bn}.running_var'] = (1 - m) * s[f'{prefix}{bn}.running_var'] + m * rvar.detach()
        if pool_first:                                                              # the wrong variant: the max before BatchNorm
            z = z.max(2, keepdim=True).values
        y = (z - mean[None, :, None]) / torch.sqrt(nvar + EPS)[None, :, None] * s[f'{prefix}{bn}.weight'][None, :, None] + s[f'{prefix}{bn}.bias'][None, :, None]
        return torch.relu(y)

    def _trunk(self, prefix, x, max_last):
        pf = None
        for i in range(1, 5):
            x = self._layer(prefix, f'conv{i}', f'bn{i}', x)
            if i == 2:
                pf = x
        if self.wrong == 'max_before_bn':
            return pf, self._layer(prefix, 'conv5', 'bn5', x, pool_first=True)
        return pf, self._max(self._layer(prefix, 'conv5', 'bn5', x))

    def forward(self, param, pool, target):
        """numpy inputs -> dict: the five losses (numpy, LOSS_NAMES), 'S2' [B,62], 'Lr' [B,3,68], 'mean' / 'var' [3649] of this call"""
        p, po, t = (lg._t(a, self.dtype) for a in (param, pool, target))
        self.stats = []
        with torch.no_grad():
            Lc, Lg = self.landmarks(p), self.landmarks(t)
            Lr = Lc + 0.05 * self.mlp_for(Lc, po, p)
            s2 = self.mlp_rev(Lr)
            W = lc.WEIGHTS
            losses = (W[0] * lg.wing(Lc, Lg), W[1] * lg.wing(Lr, Lg), W[2] * lg.param_loss(p, t), W[3] * lg.param_loss(s2, t, 'only_3dmm'),
                      W[4] * lg.param_loss(s2, p, 'only_3dmm'))
        assert [n for n, _, _ in self.stats] == [n for n, _ in bn_order()]
        out = {k: v.numpy() for k, v in zip(lc.LOSS_NAMES, losses)}
        out.update(S2=s2.numpy(), Lr=Lr.numpy(), mean=torch.cat([m for _, m, _ in self.stats]).numpy(),
                   var=torch.cat([v for _, _, v in self.stats]).numpy())
        self.stats = None
        return out

    def running(self):
        """-> (running_mean [3649], running_var [3649]) as they stand"""
        return (torch.cat([self.sd[n + '.running_mean'] for n, _ in bn_order()]).numpy(),
                torch.cat([self.sd[n + '.running_var'] for n, _ in bn_order()]).numpy())


def running_of_flat(flat):
    """the same two vectors from a flat state (syn_export_synergy_flat)"""
    import loss_wgrad_cases as lw
    where = lw.flat_slices()
    flat = np.asarray(flat)
    cut = lambda k: flat[where[k][0]:where[k][0] + int(np.prod(where[k][1]))]
    return (np.concatenate([cut(n + '.running_mean') for n, _ in bn_order()]), np.concatenate([cut(n + '.running_var') for n, _ in bn_order()]))


def case_key(state, B, what):
    return f'{state}|B{B}|{what}'


RECORDED_FIELDS = lc.LOSS_NAMES + ('S2', 'Lr', 'mean', 'var', 'run1_mean', 'run1_var', 'run3_mean', 'run3_var')
PER_CHANNEL = ('mean', 'var', 'run1_mean', 'run1_var', 'run3_mean', 'run3_var')


def run_case(head, B):
    """CALLS calls of `head` on the first B candidates -> the fields of the fixture (whole vectors)"""
    out = None
    for call in range(1, CALLS + 1):
        r = head.forward(*inputs(B))
        if call == 1:
            out = r
        if call in (1, CALLS):
            out[f'run{call}_mean'], out[f'run{call}_var'] = head.running()
    return out


def rel(got, want, field, channels=None):
    """losses: the worst relative error of an element; S2 / Lr: relative to the max of the tensor; the per-channel fields: per BatchNorm,
    relative to the max of THAT BatchNorm's tensor (a BatchNorm with a variance of 1e-30 everywhere, the degenerate heads, is held to
    1e-30).  channels: the channel index of every element when the vectors are samples (recorded_channels()), else they are whole."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if field in lc.LOSS_NAMES:                                                      # a 0-d loss may come as [1]
        got, want = got.reshape(-1), want.reshape(-1)
    assert got.shape == want.shape, (field, got.shape, want.shape)
    if field in lc.LOSS_NAMES:
        return float((np.abs(got - want) / np.abs(want)).max())
    if field not in PER_CHANNEL:
        return float(np.abs(got - want).max() / np.abs(want).max())
    ch = np.arange(BN_CHANNELS) if channels is None else np.asarray(channels)
    e = 0.0
    for at, n in bn_offsets().values():
        m = (ch >= at) & (ch < at + n)
        e = max(e, float(np.abs(got[m] - want[m]).max() / max(np.abs(want[m]).max(), 1e-300)))
    return e


def worst(got, want, fields=RECORDED_FIELDS, channels=None):
    """-> (worst rel, field) over the fields.  channels: `want` holds these channels of the per-channel fields (the fixture), `got` is whole"""
    w = (0.0, '')
    for f in fields:
        g = got[f]
        if channels is not None and f in PER_CHANNEL:
            g = np.asarray(g)[channels]
        e = rel(g, want[f], f, channels)
        if not e <= w[0]:
            w = (e, f)
    return w


def recorded(gold, state, B):
    return {f: gold[case_key(state, B, f)] for f in RECORDED_FIELDS}
