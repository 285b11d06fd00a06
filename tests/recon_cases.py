"""Shared by tests/test_recon_cases_cpu.py and tests/test_gpu_recon_edges.py: 3DMM packs of any vertex / landmark count, a float64
statement of the reconstruction they are held to, the case tables, and a plain-Python restatement of the launcher's choice of store
schedule (so the CPU test can assert that the tables reach every schedule they name).  float64 after the float32 inputs: the
definition is the yardstick, not the thing measured."""
import functools
from collections import namedtuple

import numpy as np

from test_gpu_numerics import per_face_err          # per face: max |diff| / max |want|          # noqa: F401  (re-exported)

BAR = 2e-6                  # the project's reconstruction bar on per_face_err (tests/test_gpu_numerics.py)
REF_BAR = 5e-7              # float64 reference vs the float32 oracle on the same inputs: a quarter of BAR, three quarters are the kernel's

# 4256 = 19 * 224 (whole PK windows); 4479: n mod 32 = 31; 4485: n mod 32 = 5 and the last PK window starts past the end for most rows
VERTEX_COUNTS = (1, 31, 32, 33, 127, 128, 129, 1023, 1024, 4095, 4096, 4097, 4112, 4256, 4257, 4479, 4485)
LANDMARK_COUNTS = (1, 31, 32, 33, 68, 255, 256, 257, 300)
LMK_N_VERT = 4485
BATCH_SIZES = (1, 31, 32, 33, 65)
FULL_N_VERT = 53215
# (n_vert, layout name, B): several face tiles per workgroup and a ragged last face tile (test_recon_cases_cpu.py holds them to that)
LARGE_B_CASES = ((4097, 'default', 1701), (4485, 'packed', 1445), (FULL_N_VERT, 'packed', 161))
PARENT_N_VERT = 4608        # the parent pack the small ones are cut from
N_DEFAULT_LMK = 68
LOCK_S = 2.0 ** -11         # gimbal-lock rows: every norm, quotient and cross product is exact
LOCK_LANES = (0, 31, 63)
LOCK_B = 70
LOCK_N_VERT = 129


def roundup128(n):
    return (n + 127) // 128 * 128


# ------------------------------------------------------------------------------------------------ packs
@functools.lru_cache(maxsize=4)
def _parent(seed):
    from synergynet_amd import synth
    return synth.make_3dmm(seed, n_vert=PARENT_N_VERT)


def flat_keypoints(vertices):
    """vertex indices -> the reference's flat [3k, 3k+1, 3k+2] form (utils/io.py:78-81)"""
    v = np.asarray(vertices, dtype=np.int64).reshape(-1)
    return np.stack([3 * v, 3 * v + 1, 3 * v + 2], axis=1).reshape(-1)


def default_keypoints(n_vert, seed=0):
    """min(68, n_vert) distinct vertices, sorted (what synth.make_3dmm draws)"""
    rng = np.random.default_rng(1000 + seed)
    return np.sort(rng.choice(n_vert, min(N_DEFAULT_LMK, n_vert), replace=False))


def landmark_vertices(n_lmk, n_vert=LMK_N_VERT, seed=0):
    """n_lmk vertex indices; from three on: unsorted, vertex 0 and vertex n_vert - 1 among them, one vertex twice"""
    rng = np.random.default_rng(2000 + 7 * n_lmk + seed)
    if n_lmk < 3:
        return rng.choice(n_vert, n_lmk, replace=False).astype(np.int64)
    inner = rng.choice(np.arange(1, n_vert - 1), n_lmk - 3, replace=False)
    v = np.concatenate([[0, n_vert - 1], inner]).astype(np.int64)
    v = np.concatenate([v, v[rng.integers(0, v.size, 1)]])               # the duplicate
    v = v[rng.permutation(v.size)]
    if np.all(np.diff(v) >= 0):                                          # (n_lmk = 3 can come out sorted)
        v = v[::-1].copy()
    return v


def small_pack(n_vert, keypoints=None, seed=4321, param_mean=None, param_std=None):
    """The first n_vert vertices of a synth.make_3dmm parent: rows of w_shp / w_exp / u_shp / u_exp sliced, `tri` replaced by indices
    that stay in range, `keypoints` (VERTEX indices; default: default_keypoints) expanded to the flat form.  param_mean / param_std:
    replacements for the 12 pose entries."""
    assert 1 <= n_vert <= PARENT_N_VERT
    p = _parent(seed)
    out = {k: np.array(p[k][:3 * n_vert], copy=True) for k in ('w_shp', 'w_exp', 'u_shp', 'u_exp')}
    out['param_mean'], out['param_std'] = np.array(p['param_mean'], copy=True), np.array(p['param_std'], copy=True)
    if param_mean is not None:
        out['param_mean'][:12] = np.asarray(param_mean, dtype=np.float32)
    if param_std is not None:
        out['param_std'][:12] = np.asarray(param_std, dtype=np.float32)
    kv = default_keypoints(n_vert, seed) if keypoints is None else np.asarray(keypoints, dtype=np.int64)
    assert kv.size >= 1 and kv.min() >= 0 and kv.max() < n_vert
    out['keypoints'] = flat_keypoints(kv)
    rng = np.random.default_rng(seed + n_vert)
    out['tri'] = (rng.integers(0, n_vert, size=(3, max(1, 2 * n_vert))) + 1).astype(np.int32)      # 1-based like the reference's
    return out


def landmark_pack(n_lmk):
    return small_pack(LMK_N_VERT, keypoints=landmark_vertices(n_lmk))


def lock_pack():
    """pose entries de-whiten exactly: param_mean = 0, param_std = 1"""
    return small_pack(LOCK_N_VERT, param_mean=np.zeros(12), param_std=np.ones(12))


# ------------------------------------------------------------------------------------------------ inputs
def inputs(n, B, tag=0):
    """(param [B,62], roi [B,5]) float32 of a case; every batch size of one vertex / landmark count has its own draw"""
    from synergynet_amd import synth
    seed = 10007 * tag + 31 * n + B
    return synth.make_params(B, seed=seed, scale=1.3), synth.make_rois(B, seed=seed + 1)


def lock_rows(sign):
    """the 12 pose entries of a face with R[2,0] == sign (+1 | -1); the third row never enters R"""
    s = np.float32(LOCK_S)
    r1, r2 = ((0, s, 0), (0, 0, s)) if sign > 0 else ((0, 0, s), (0, s, 0))
    return np.array([*r1, 61.0, *r2, 58.5, 3e-4, -2e-4, 4e-4, -40.0], dtype=np.float32)


def lock_inputs(sign=0):
    """LOCK_B faces on lock_pack(): ordinary poses (the parent's statistics, written de-whitened since mean = 0 and std = 1 here);
    sign != 0 puts a locked face at LOCK_LANES."""
    param, roi = inputs(LOCK_N_VERT, LOCK_B, tag=3)
    p = _parent(4321)
    rng = np.random.default_rng(77)
    param[:, :12] = (p['param_mean'][:12] + rng.standard_normal((LOCK_B, 12)) * p['param_std'][:12]).astype(np.float32)
    if sign:
        param[list(LOCK_LANES), :12] = lock_rows(sign)
    return param, roi


# ------------------------------------------------------------------------------------------------ the float64 reference
def reference(pack, param, roi=None, dense=True, transform=True):
    """reconstruct_vertex_62 (synergy3DMM.py:116-149) + the ROI affine of _predict_vertices (utils/inference.py:127-138), float64
    from the float32 inputs on (param, param_mean / param_std, w_shp, w_exp, u = u_shp + u_exp as the pack loader adds it in
    float32, keypoints, roi): de-whitening, contraction, pose matrix, flip, affine -> [B,3,n] float64"""
    from oracle import recon_numpy
    b = recon_numpy.Basis(pack)
    f8 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    param = np.asarray(param, dtype=np.float32)
    assert param.ndim == 2 and param.shape[1] == 62
    pr = f8(param) * f8(b.param_std[:62]) + f8(b.param_mean[:62])
    p_ = pr[:, :12].reshape(-1, 3, 4)
    P, offset = p_[:, :, :3], p_[:, :, 3:4]
    alpha = pr[:, 12:62]
    if dense:
        w, u = np.concatenate([f8(b.w_shp), f8(b.w_exp)], axis=1), f8(b.u)
    else:
        w, u = np.concatenate([f8(b.w_shp_base), f8(b.w_exp_base)], axis=1), f8(b.u_base)
    s = alpha @ w.T + u.reshape(1, -1)                                     # [B,3n], xyz interleaved
    v = s.reshape(param.shape[0], -1, 3).transpose(0, 2, 1)
    vertex = P @ v + offset
    if transform:
        vertex[:, 1, :] = 121.0 - vertex[:, 1, :]
    if roi is not None:
        r = f8(roi)
        sx, sy = (r[:, 2] - r[:, 0]) / 120.0, (r[:, 3] - r[:, 1]) / 120.0
        vertex[:, 0, :] = vertex[:, 0, :] * sx[:, None] + r[:, 0, None]
        vertex[:, 1, :] = vertex[:, 1, :] * sy[:, None] + r[:, 1, None]
        vertex[:, 2, :] *= ((sx + sy) / 2)[:, None]
    return vertex


def oracle(pack, param, roi=None, dense=True, transform=True):
    """the float32 oracle on the same inputs: the batched method without a ROI, the per-face one with"""
    from oracle import recon_numpy
    b = recon_numpy.Basis(pack)
    param = np.asarray(param, dtype=np.float32)
    if roi is None:
        return recon_numpy.reconstruct_vertex_62(b, param, dense=dense, transform=transform)
    return np.stack([recon_numpy.predict_vertices(b, param[i], roi[i], dense, transform) for i in range(param.shape[0])])


UNIT_ROI = np.array([0, 0, 120, 120, 1], dtype=np.float32)       # predict_pose's affine with this box is t * 1 + 0


def reference_pose(pack, param, roi=None):
    """oracle.recon_numpy.predict_pose, unchanged, face by face -> (angles [B,3] float64 degrees, t3d [B,3] float32)"""
    from oracle import recon_numpy
    b = recon_numpy.Basis(pack)
    param = np.asarray(param, dtype=np.float32)
    res = [recon_numpy.predict_pose(b, param[i], UNIT_ROI if roi is None else roi[i]) for i in range(param.shape[0])]
    return np.array([r[0] for r in res], dtype=np.float64), np.stack([r[1] for r in res]).astype(np.float32)


def rotation_f32(pack, param_row):
    """the float32 matrix R the reference hands to matrix2angle_corr for one face (P2sRt on the de-whitened float32 parameters)"""
    from oracle import recon_numpy
    b = recon_numpy.Basis(pack)
    p = np.asarray(param_row, dtype=np.float32) * b.param_std[:62] + b.param_mean[:62]
    return recon_numpy.P2sRt(p[:12].reshape(3, -1))[1]


# ------------------------------------------------------------------------------------------------ layouts and the launcher's choice
# name -> (pitch(n), pad_writable, floats past a 128-byte boundary); None where the layout does not exist for that n
Layout = namedtuple('Layout', 'name pitch pad_writable offset')


def default_layout(n):
    """what SynergyNet.empty_vertices allocates for a dense mesh"""
    pitch = roundup128(n) if n >= 1024 else n
    return Layout('default', pitch, int(pitch > n), 0)


def layouts(n):
    """the output layouts of issue item 2 for n vertices, (a) .. (g)"""
    out = [Layout('packed', n, 0, 0),                                        # (a)
           Layout('packed+pad_writable', n, 1, 0),                           # (b)
           Layout('packed+1', n, 0, 1), Layout('packed+4', n, 0, 4), Layout('packed+16', n, 0, 16),      # (c)
           Layout('pitch n+5', n + 5, 0, 0),                                 # (d)
           Layout('pitch roundup128, pad_writable', roundup128(n), 1, 0)]    # (e)
    if roundup128(n) - 1 >= n:
        out.append(Layout('pitch roundup128-1, pad_writable', roundup128(n) - 1, 1, 0))      # (f)
    out.append(Layout('pitch roundup128+128', roundup128(n) + 128, 0, 0))    # (g)
    return out


def layout_by_name(n, name):
    return default_layout(n) if name == 'default' else [l for l in layouts(n) if l.name == name][0]


Path = namedtuple('Path', 'kind per ragged tail_per')
WG_TARGET, PK_WINDOW, PK_MIN_VERT = 1664, 224, 4096


def expected_path(n, pitch, pad_writable, aligned128, B):
    """MIRRORS launch_reconstruct_f16 (synergynet_amd/csrc/recon_kernels.hip) at its default knobs -- keep the two in step.
    kind: the store schedule of the WHOLE 32-face tiles ('FAST' | 'PK' | 'guarded'; with FAST and B < 32 there is none: the one
    ragged tile runs guarded and that is reported); per: face tiles a workgroup of that launch walks; ragged: a ragged last face tile
    exists (under FAST it runs in a guarded launch of its own, tail_per tiles per workgroup -- always 1; else inside the same launch)."""
    nvp = (n + 31) // 32 * 32
    n_tiles, n_ftiles = nvp // 32, (B + 31) // 32
    fast_groups = (n_tiles + 3) // 4
    fast_ok = bool(pad_writable) and pitch >= fast_groups * 128
    pk = (not fast_ok) and pitch == n and n >= PK_MIN_VERT and bool(aligned128)
    n_groups = (n + PK_WINDOW - 1) // PK_WINDOW if pk else fast_groups

    def per_of(nft):
        target = WG_TARGET // 2 if pk else WG_TARGET
        n_split = max(1, (target + n_groups - 1) // n_groups)
        n_split = min(n_split, nft)
        return (nft + n_split - 1) // n_split
    ragged = B % 32 != 0
    if fast_ok:
        if B // 32 == 0:
            return Path('guarded', per_of(1), ragged, 1)
        return Path('FAST', per_of(B // 32), ragged, per_of(1) if ragged else 0)
    return Path('PK' if pk else 'guarded', per_of(n_ftiles), ragged, 0)
