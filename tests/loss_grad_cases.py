"""Shared by tests/test_loss_grad_cpu.py, tests/test_gpu_loss_grad.py and tests/golden/make_loss_grad_golden.py: a torch-CPU restatement
(autograd; float64 unless a dtype is asked for) of the reference's WingLoss, ParamLoss and of the whole loss head of
model_building.py:141-157 -- landmark reconstruction, MLP_for, MLP_rev in eval() form, the five weighted losses -- written from the
formulas and from synth's state, with the wrong variants the bite tests hold against the recording, and the input builders.
The inputs of the module-level cases are those of tests/loss_cases.py."""
import os

import numpy as np
import torch

import loss_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'loss_grad_golden.npz')

TOL = lc.TOL                            # GPU bar: 1e-4 x max |g| of the tensor
CPU_BAR = 1e-5                          # restatement against the recording, and fp32 against fp64 in the generator: x max |g|
FULL_MAX_B = 3                          # module gradients are recorded whole up to this batch, every SAMPLE-th element above it
SAMPLE = 61
TIE_ROW = (1.0, 3.0, 3.0, 0.0)          # torch's MaxPool1d sends the gradient of a tie to the FIRST maximum: index 1


def recorded_part(grad, B):
    g = np.asarray(grad).reshape(-1)
    return g if B <= FULL_MAX_B else g[::SAMPLE]


def param_grad_keys():
    return [f'param_B{B}_{mode}' + ('_same' if same else '') for B in lc.PARAM_B for mode in ('normal', 'only_3dmm') for same in (False, True)]


def param_grad_upstream(B):
    """a non-uniform upstream gradient per face (exact in fp32)"""
    return ((np.arange(B) % 7 + 1) / 8.0).astype(np.float32)


def identical_face():
    """3 faces, the middle one's input equals its target: ParamLoss 'normal' is 0 there and torch's gradient is NaN for that row"""
    a, b = lc.param_inputs(3)
    b = b.copy()
    b[1] = a[1]
    return a, b


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---- the two modules ----
def wing(pred, target, omega=lc.OMEGA, epsilon=lc.EPSILON, count_nan=False):
    """torch tensors [B,3,n] -> 0-d loss; count_nan: the wrong variant (every element counted in n)"""
    d = (target - pred).abs()
    lo, hi = d < omega, d >= omega
    C = omega - omega * float(np.log(1.0 + omega / epsilon))
    total = (omega * torch.log(1 + d[lo] / epsilon)).sum() + (d[hi] - C).sum()
    n = d.numel() if count_nan else int(lo.sum() + hi.sum())
    return total / n


def param_loss(a, b, mode='normal', aligned=False):
    if mode == 'normal':
        return torch.sqrt(((a[:, :12] - b[:, :12]) ** 2).mean(1) + ((a[:, 12:62] - b[:, 12:62]) ** 2).mean(1))
    lhs = a[:, 12:62] if aligned else a[:, :50]               # aligned: the wrong variant
    return torch.sqrt(((lhs - b[:, 12:62]) ** 2).mean(1))


def wing_grad(pred, target, g=1.0, dtype=torch.float64, **kw):
    """numpy [B,3,n] -> d (g x loss) / d pred as numpy, by autograd"""
    p, t = _t(pred, dtype).requires_grad_(True), _t(target, dtype)
    (wing(p, t, **kw) * g).backward()
    return p.grad.numpy()


def param_grad(a, b, mode, g=None, dtype=torch.float64, **kw):
    """-> (d input, d target) of sum_b g[b] loss[b] (g None: ones)"""
    x, y = _t(a, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)
    w = torch.ones(x.shape[0], dtype=dtype) if g is None else _t(g, dtype)
    (param_loss(x, y, mode, **kw) * w).sum().backward()
    return x.grad.numpy(), y.grad.numpy()


# ---- the loss head ----
class Head:
    """The head in eval() form from synth.make_3dmm's pack and synth.make_synergy_state's dict.  max_last / drop_s1s2_param / aligned /
    count_nan are the wrong variants."""

    def __init__(self, pack, sd, dtype=torch.float64, perm_seed=None):
        self.dtype = dtype
        self.perm = None if perm_seed is None else np.random.default_rng(perm_seed)      # sum every layer's channels in a random order
        self.record = None                                                              # a list: receives (layer name, pre-activations)
        kp = np.asarray(pack['keypoints'])
        u = np.asarray(pack['u_shp'], dtype=np.float64) + np.asarray(pack['u_exp'], dtype=np.float64)
        self.u_base, self.w_shp_base, self.w_exp_base = _t(u[kp], dtype), _t(pack['w_shp'][kp], dtype), _t(pack['w_exp'][kp], dtype)
        self.mean, self.std = _t(np.asarray(pack['param_mean'])[:62], dtype), _t(np.asarray(pack['param_std'])[:62], dtype)
        self.sd = {k: _t(v, dtype) for k, v in sd.items()}

    def landmarks(self, param):
        p_ = param * self.std + self.mean
        P = p_[:, :12].reshape(-1, 3, 4)
        p, offset = P[:, :, :3], P[:, :, 3:]
        V = self.u_base + self.w_shp_base @ p_[:, 12:52, None] + self.w_exp_base @ p_[:, 52:62, None]
        v = p @ V.reshape(-1, 68, 3).transpose(1, 2) + offset
        return torch.cat([v[:, :1], 121.0 - v[:, 1:2], v[:, 2:]], 1)                  # transform = 1: row 1 flipped

    def _layer(self, prefix, conv, bn, x):
        s = self.sd
        W = s[f'{prefix}{conv}.weight'][:, :, 0]
        if self.perm is not None:
            order = torch.from_numpy(self.perm.permutation(W.shape[1]))
            W, x = W[:, order].contiguous(), x[:, order].contiguous()
        y = torch.einsum('oi,bip->bop', W, x) + s[f'{prefix}{conv}.bias'][None, :, None]
        inv = s[f'{prefix}{bn}.weight'] / torch.sqrt(s[f'{prefix}{bn}.running_var'] + 1e-5)
        y = (y - s[f'{prefix}{bn}.running_mean'][None, :, None]) * inv[None, :, None] + s[f'{prefix}{bn}.bias'][None, :, None]
        if self.record is not None:
            self.record.append((prefix + conv, y.detach()))
        return torch.relu(y)

    @staticmethod
    def _max(x, last=False):
        if not last:
            return torch.nn.functional.max_pool1d(x, x.shape[2])
        idx = x.shape[2] - 1 - torch.flip(x, [2]).argmax(2, keepdim=True)             # the LAST maximum: the wrong routing of a tie
        return torch.gather(x, 2, idx)

    def _trunk(self, prefix, x, max_last):
        pf = None
        for i in range(1, 6):
            x = self._layer(prefix, f'conv{i}', f'bn{i}', x)
            if i == 2:
                pf = x
        return pf, self._max(x, max_last)

    def mlp_for(self, lmk, pool, param, max_last=False):
        pf, gf = self._trunk('forwardDirection.', lmk, max_last)
        n = lmk.shape[2]
        rep = lambda v: v[:, :, None].expand(-1, -1, n)
        x = torch.cat([pf, gf.expand(-1, -1, n), rep(pool), rep(param[:, 12:52]), rep(param[:, 52:62])], 1)
        for i in range(6, 10):
            x = self._layer('forwardDirection.', f'conv{i}', f'bn{i}', x)
        return x

    def mlp_rev(self, lmk, max_last=False):
        _, gf = self._trunk('reverseDirection.', lmk, max_last)
        return torch.cat([self._layer('reverseDirection.', f'conv6_{i}', f'bn6_{i}', gf) for i in (1, 2, 3)], 1)[:, :, 0]

    def losses(self, param, pool, target, max_last=False, drop_s1s2_param=False, aligned=False, count_nan=False):
        """tensors -> the five weighted losses in LOSS_NAMES order"""
        Lc, Lg = self.landmarks(param), self.landmarks(target)
        Lr = Lc + 0.05 * self.mlp_for(Lc, pool, param, max_last)
        s2 = self.mlp_rev(Lr, max_last)
        W = lc.WEIGHTS
        return (W[0] * wing(Lc, Lg, count_nan=count_nan), W[1] * wing(Lr, Lg, count_nan=count_nan), W[2] * param_loss(param, target),
                W[3] * param_loss(s2, target, 'only_3dmm', aligned),
                W[4] * param_loss(s2, param.detach() if drop_s1s2_param else param, 'only_3dmm', aligned))

    def vjp(self, param, pool, target, g_scalars, g_per_face, **kw):
        """numpy inputs and upstream gradients -> (d param, d pool) of sum_i <g_i, loss_i>"""
        p, po = _t(param, self.dtype).requires_grad_(True), _t(pool, self.dtype).requires_grad_(True)
        L = self.losses(p, po, _t(target, self.dtype), **kw)
        gs, gp = _t(g_scalars, self.dtype), _t(g_per_face, self.dtype)
        total = gs[0] * L[0] + gs[1] * L[1] + sum((gp[i] * L[2 + i]).sum() for i in range(3))
        gpar, gpool = torch.autograd.grad(total, (p, po))
        return gpar.numpy(), gpool.numpy()

    def grads(self, param, pool, target, **kw):
        """numpy inputs -> {name: (d param, d pool)} for each loss's .mean() and 'total' (their sum), numpy"""
        out = {}
        p, po = _t(param, self.dtype).requires_grad_(True), _t(pool, self.dtype).requires_grad_(True)
        losses = self.losses(p, po, _t(target, self.dtype), **kw)
        means = [v.mean() for v in losses]
        zero = lambda g, like: np.zeros(like.shape) if g is None else g.numpy()
        for name, m in zip(lc.LOSS_NAMES + ('total',), means + [sum(means)]):
            gp, gpo = torch.autograd.grad(m, (p, po), retain_graph=True, allow_unused=True)
            out[name] = (zero(gp, p), zero(gpo, po))
        return out


def graph_inputs():
    from synergynet_amd import synth
    pool = np.abs(np.random.default_rng(lc.SEED_GRAPH_POOL).standard_normal((5, 1280))).astype(np.float32)
    return synth.make_params(5, lc.SEED_GRAPH_PARAM), pool, synth.make_params(5, lc.SEED_GRAPH_TARGET)


SEED_BATCH_PARAM, SEED_BATCH_TARGET, SEED_BATCH_POOL = 271, 273, 275
BATCH_SIZES = (1, 3, 4, 5, 9, 17, 37)   # 68 B is a multiple of 32 only where 8 divides B: for none of these; 17 = 16 + 1 faces
CANDIDATES = 64
# A gradient is a discontinuous function of the inputs at every ReLU and arg-max, so a face can be held to 1e-4 only if no correct fp32
# evaluation can land on the other side of one that matters.  Two conditions, both on the CPU and neither looking at the library:
#  * the 204 units of MLP_for's last ReLU and the 62 of MLP_rev's heads each gate a whole coordinate's / parameter's gradient: their
#    float64 pre-activations must stay GATE_MARGIN x the layer's largest away from 0.  An fp32 chain of 9 layers of up to 2354-term
#    sums is off by about 9 sqrt(2354) 2^-24 = 2.6e-5 of the layer's scale; 1e-4 leaves a factor of four;
#  * the wide layers (1e5 units per face) always hold units within 1e-6 of 0; there the fp32 restatement is run with every layer's
#    channels summed in ORDERS random orders, and each run's gradient must meet the float64 one within CPU_BAR.
GATE_MARGIN = 1e-4
ORDERS = 5


def candidate_inputs():
    from synergynet_amd import synth
    pool = np.abs(np.random.default_rng(SEED_BATCH_POOL).standard_normal((CANDIDATES, 1280))).astype(np.float32)
    return synth.make_params(CANDIDATES, SEED_BATCH_PARAM), pool, synth.make_params(CANDIDATES, SEED_BATCH_TARGET)


def batch_inputs(faces, B=37):
    """(param, pool, target) of the batch-shape tests: the first B of the fixture's batch_faces (select_batch_faces chose them)"""
    param, pool, target = candidate_inputs()
    f = np.asarray(faces)[:B]
    return param[f], pool[f], target[f]


def select_batch_faces(pack, sd, count=37):
    """the first `count` candidates that meet the two conditions above -> (indices, {rejected index: reason})"""
    param, pool, target = candidate_inputs()
    h64 = Head(pack, sd)
    h64.record = []
    with torch.no_grad():
        h64.losses(_t(param, torch.float64), _t(pool, torch.float64), _t(target, torch.float64))
    gate = np.full(CANDIDATES, np.inf)
    for name, y in h64.record:
        if name.endswith('conv9') or 'conv6_' in name:
            a = y.abs().reshape(CANDIDATES, -1)
            gate = np.minimum(gate, (a.min(1).values / a.max(1).values).numpy())
    h64.record = None
    gs, gp = np.ones(2, dtype=np.float32), np.ones((3, 1), dtype=np.float32)
    chosen, rejected = [], {}
    for b in range(CANDIDATES):
        if len(chosen) == count:
            break
        if gate[b] < GATE_MARGIN:
            rejected[b] = 'gate margin %.1e' % gate[b]
            continue
        one = (param[b:b + 1], pool[b:b + 1], target[b:b + 1], gs, gp)
        want = h64.vjp(*one)
        worst = 0.0
        for seed in range(ORDERS + 1):
            got = Head(pack, sd, torch.float32, perm_seed=seed if seed else None).vjp(*one)
            worst = max(worst, rel_to_max(got[0], want[0]), rel_to_max(got[1], want[1]))
        if worst > CPU_BAR:
            rejected[b] = 'summation order moves the gradient by %.1e' % worst
            continue
        chosen.append(b)
    assert len(chosen) == count
    return np.array(chosen), rejected


def head_upstream(B, seed=9):
    """random upstream gradients per loss and per face: (g_scalars [2], g_per_face [3][B]) float32"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, 2).astype(np.float32), rng.uniform(-1, 1, (3, B)).astype(np.float32)


def tie_case(pack, sd, faces):
    """A max-pool tie that shows in d param, through the public entry: -> (pack, synergy state, param, pool, target).
    The landmarks of largest and of smallest z each get a neighbour that takes its z from their vertex and keeps its own x and y; the pose's third row is (0, 0, s) exactly (its mean and
    the faces' whitened entries 8 and 9 are 0), so the two landmarks have the same crop-space z bit for bit in any precision; MLP_for's
    conv1 reads z alone, so its activations tie at the two points in every channel of every layer.  The first maximum is the
    lower index (torch's MaxPool1d); routing to the other instead moves d p[2, 0:2] = sum_points d Lc_z V_xy, because the two points differ in V_xy."""
    pack = dict(pack)
    kp = np.array(pack['keypoints']).copy()                   # flat indices [3k, 3k+1, 3k+2] per landmark
    u = (np.asarray(pack['u_shp'], dtype=np.float64) + np.asarray(pack['u_exp'], dtype=np.float64)).reshape(-1)
    hi, lo = int(np.argmax(u[kp[2::3]])), int(np.argmin(u[kp[2::3]]))     # the extreme z: these points win the channels that grow / fall with z
    for a in (hi, lo):
        b = a + 1 if a + 1 not in (hi, lo) and a + 1 < 68 else a - 1
        kp[3 * b + 2] = kp[3 * a + 2]
    mean = np.array(pack['param_mean']).copy()
    mean[8:10] = 0
    pack.update(keypoints=kp, param_mean=mean)
    sd = dict(sd)
    w = np.array(sd['forwardDirection.conv1.weight']).copy()
    w[:, 0:2] = 0
    sd['forwardDirection.conv1.weight'] = w
    param, pool, target = batch_inputs(np.asarray(faces)[[0, 1, 3, 4]], 4)
    param = param.copy()
    param[:, 8:10] = 0
    return pack, sd, param, pool, target


def rel_to_max(got, want):
    """max |got - want| / max |want| over the finite entries of want"""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    return float(np.abs(got[fin] - want[fin]).max() / max(np.abs(want[fin]).max(), 1e-30))


def same_classes(got, want):
    """NaN at the same positions, infinities equal, everything else finite"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
                and np.array_equal(got[np.isinf(want)], want[np.isinf(want)]))
