"""Shared by the synergy tests and tests/golden/make_synergy_golden.py: the numpy definition of MLP_for / MLP_rev written from the
FOLDED form (include/synergy_hip.h: per layer W [out][in], scale, shift, y = relu(scale * (W x) + shift)), the fixture's case
names and the batch sizes the GPU tests walk.  float64 throughout: the definition is the yardstick, not the thing measured."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'synergy_golden.npz')

N_PTS, N_GLOBAL, N_POOL = 68, 1024, 1280
CASES = ('a', 'b', 'c', 'd')          # a: 5 ordinary faces; b: one cold face; c: [ordinary, all-zero landmarks]; d: zero pool and codes
# below one 4-face group, a full group, a group + 1, several workgroups with a ragged tail
BATCH_SIZES = (1, 3, 4, 5, 37)
BAR = 1e-4                             # the project bar, on conftest's rel_l2 and rel_max
PAD_POINTS = 12                        # all-zero input points appended by the padding condition of case b
PAD_MIN_CHANNELS = 64

TRUNK = [(3, 64), (64, 64), (64, 64), (64, 128), (128, 1024)]
FOR_TAIL = [(512, 256), (256, 128), (128, 3)]
FACE_K = N_GLOBAL + N_POOL + 40 + 10   # global | pool | shape | expr


def parse_folded(folded):
    """The folded float array -> {'for': [...], 'rev': [...]}: lists of layers (W [out,in], scale, shift); conv6 of MLP_for is
    (Wpoint [512,64], Wface [512,2354], scale, shift), MLP_rev's last layer the concatenated heads [62,1024]."""
    f = np.asarray(folded, dtype=np.float64)
    at = [0]

    def take(*shape):
        n = int(np.prod(shape))
        a = f[at[0]:at[0] + n].reshape(shape)
        at[0] += n
        return a

    def layer(cin, cout):
        return take(cout, cin), take(cout), take(cout)
    out = {'for': [layer(*s) for s in TRUNK]}
    out['for'].append((take(512, 64), take(512, FACE_K), take(512), take(512)))
    out['for'] += [layer(*s) for s in FOR_TAIL]
    out['rev'] = [layer(*s) for s in TRUNK] + [layer(1024, 62)]
    assert at[0] == f.size, (at[0], f.size)
    return out


def _act(x, W, scale, shift):
    """x [B,P,in] -> relu(scale * (W x) + shift) [B,P,out]"""
    return np.maximum((x @ W.T) * scale + shift, 0.0)


def trunk(layers, lmk, pad_points=0):
    """conv1..conv5 + max over the points: lmk [B,3,P] -> (conv2's output [B,P,64], global feature [B,1024]).  pad_points: that many
    all-zero input points appended before the max -- what a kernel computes if its padding rows take part."""
    x = np.transpose(np.asarray(lmk, dtype=np.float64), (0, 2, 1))
    if pad_points:
        x = np.concatenate([x, np.zeros((x.shape[0], pad_points, 3))], axis=1)
    pf = None
    for i, L in enumerate(layers[:5]):
        x = _act(x, *L)
        if i == 1:
            pf = x
    return pf, x.max(axis=1)


def mlp_for(F, lmk, pool, param):
    """-> (residual [B,3,P], global_features [B,1024]); codes = the whitened param[:,12:52] | param[:,52:62]"""
    L = F['for']
    pf, gf = trunk(L, lmk)
    face = np.concatenate([gf, np.asarray(pool, dtype=np.float64), np.asarray(param, dtype=np.float64)[:, 12:62]], axis=1)
    Wp, Wf, scale, shift = L[5]
    x = np.maximum((pf @ Wp.T + (face @ Wf.T)[:, None, :]) * scale + shift, 0.0)
    for lay in L[6:]:
        x = _act(x, *lay)
    return np.transpose(x, (0, 2, 1)), gf


def mlp_rev(F, lmk):
    L = F['rev']
    _, gf = trunk(L, lmk)
    return _act(gf[:, None, :], *L[5])[:, 0, :]


def refine(F, lmk, pool, param):
    res, gf = mlp_for(F, lmk, pool, param)
    return np.asarray(lmk, dtype=np.float64) + 0.05 * res, res, gf


def roi_affine(lmk, roi):
    """_predict_vertices' ROI affine on [B,3,P] crop-space points"""
    roi = np.asarray(roi, dtype=np.float64)
    sx, sy = (roi[:, 2] - roi[:, 0]) / 120.0, (roi[:, 3] - roi[:, 1]) / 120.0
    out = np.array(lmk, dtype=np.float64)
    out[:, 0] = out[:, 0] * sx[:, None] + roi[:, 0, None]
    out[:, 1] = out[:, 1] * sy[:, None] + roi[:, 1, None]
    out[:, 2] = out[:, 2] * ((sx + sy) / 2)[:, None]
    return out


def winners(lmk, layers):
    """per face the number of distinct points that win at least one channel of the max-pool"""
    x = np.transpose(np.asarray(lmk, dtype=np.float64), (0, 2, 1))
    for L in layers[:5]:
        x = _act(x, *L)
    return [len(set(np.argmax(f, axis=0).tolist())) for f in x]


def folded_from_seed(seed):
    """syn_fold_synergy_host on synth.make_synergy_state(seed) (device-free)"""
    import ctypes as C
    from synergynet_amd import abi, synth
    lib = abi.lib()
    flat = synth.flatten_synergy(synth.make_synergy_state(seed))
    folded = np.empty(lib.syn_synergy_folded_count(), dtype=np.float32)
    abi.check(lib.syn_fold_synergy_host(flat.ctypes.data_as(C.c_void_p), flat.size, folded.ctypes.data_as(C.c_void_p), folded.size))
    return folded


def fold_numpy(sd):
    """The same fold in numpy (float64), straight from a state_dict: what the generator checks its conditions with."""
    from synergynet_amd import synth
    parts = []

    def fold(prefix, conv, bn):
        W = np.asarray(sd[f'{prefix}{conv}.weight'], dtype=np.float64)[:, :, 0]
        g, b, m, v = (np.asarray(sd[f'{prefix}{bn}.{t}'], dtype=np.float64) for t in ('weight', 'bias', 'running_mean', 'running_var'))
        scale = g / np.sqrt(v + 1e-5)
        return W, scale, (np.asarray(sd[f'{prefix}{conv}.bias'], dtype=np.float64) - m) * scale + b
    pf, pr = synth.SYNERGY_PREFIXES
    for i, (conv, bn, _, _) in enumerate(synth.SYNERGY_FOR):
        W, sc, sh = fold(pf, conv, bn)
        parts += [W[:, :64], W[:, 64:], sc, sh] if i == 5 else [W, sc, sh]
    for conv, bn, _, _ in synth.SYNERGY_REV[:5]:
        parts += list(fold(pr, conv, bn))
    heads = [fold(pr, conv, bn) for conv, bn, _, _ in synth.SYNERGY_REV[5:]]
    parts += [np.concatenate([h[k] for h in heads], axis=0) for k in range(3)]
    return np.concatenate([p.reshape(-1) for p in parts])
