"""Shared by tests/test_loss_cpu.py, tests/test_gpu_losses.py and tests/golden/make_loss_golden.py: the float64 restatement of the
reference's WingLoss / ParamLoss / SynergyNet.forward losses / CenterCrop / AverageMeter bookkeeping, written from the formulas alone
(DESIGN 5.17), the deterministic inputs of the module-level cases (too large to store: rebuilt from integers, their checksums are in the
fixture) and the wrong variants the bite tests hold against the recording.  float64 throughout: the definition is the yardstick."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'loss_golden.npz')

TOL = 1e-4                              # the project bar (TOL of tests/test_gpu_parity.py)
CPU_BAR = 1e-5                          # restatement against the recording
OMEGA, EPSILON = 10.0, 2.0
LOSS_NAMES = ('loss_LMK_f0', 'loss_LMK_pointNet', 'loss_Param_In', 'loss_Param_S2', 'loss_Param_S1S2')
WEIGHTS = (0.05, 0.05, 0.02, 0.02, 0.001)
WING_LIPSCHITZ = OMEGA / EPSILON        # d/d delta of omega log(1 + delta / epsilon) at 0; the linear branch has slope 1
PARAM_LIPSCHITZ = 2.0 ** 0.5            # sqrt(mean_a + mean_b) of differences moved by at most e moves by at most sqrt(2) e

WING_B, WING_N = (1, 3, 257, 1025), (68, 1)
# variant -> the (B, n) it is recorded at; 'plain' at every shape
WING_VARIANTS = {'nan': (3, 68), 'inf': (3, 68), 'allnan': (3, 1), 'small': (257, 68)}
PARAM_B = (1, 3, 257)
CROP_MARGINS = (5, 0, 59, 60)
SEED_GRAPH_PARAM, SEED_GRAPH_TARGET, SEED_GRAPH_POOL, SEED_SYN = 171, 173, 175, 8643


def wing_case_names():
    return [f'wing_B{B}_n{n}_plain' for B in WING_B for n in WING_N] + [f'wing_B{B}_n{n}_{v}' for v, (B, n) in WING_VARIANTS.items()]


def parse_wing_case(name):
    _, b, n, v = name.split('_')
    return int(b[1:]), int(n[1:]), v


def wing_inputs(B, n, variant='plain'):
    """(pred, target) float32 [B,3,n].  |target - pred| is spread over [0, 30) (over [0, 10) for 'small'), both signs; the first two
    elements have pred = 0 and target = omega / the fp32 neighbour below omega, so those differences are exact."""
    rng = np.random.default_rng(1000 * B + n)
    N = B * 3 * n
    pred = (rng.integers(0, 1 << 20, N).astype(np.float64) / (1 << 20) * 120.0).astype(np.float32)
    span = 10.0 if variant == 'small' else 30.0
    delta = rng.integers(0, 1 << 20, N).astype(np.float64) / (1 << 20) * span
    sign = rng.integers(0, 2, N) * 2.0 - 1.0
    target = (pred.astype(np.float64) + sign * delta).astype(np.float32)
    below = np.nextafter(np.float32(OMEGA), np.float32(0))
    pred[:2] = 0
    target[0], target[1] = (below if variant == 'small' else np.float32(OMEGA)), below
    if variant == 'nan':
        target[N // 2] = np.nan
    elif variant == 'inf':
        target[N // 2] = np.inf
    elif variant == 'allnan':
        target[:] = np.nan
    return pred.reshape(B, 3, n), target.reshape(B, 3, n)


def param_inputs(B, same=False):
    rng = np.random.default_rng(2000 + B)
    a = (rng.integers(-(1 << 20), 1 << 20, (B, 62)).astype(np.float64) / (1 << 19)).astype(np.float32)
    b = (rng.integers(-(1 << 20), 1 << 20, (B, 62)).astype(np.float64) / (1 << 19)).astype(np.float32)
    return (a, a.copy()) if same else (a, b)


def ramp(B=1, H=120, W=120, C=3):
    """uint8 [B,H,W,C], never 0 (a zeroed pixel always differs from the input)"""
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C), indexing='ij')
    return (1 + (7 * y + 3 * x + 11 * c + 5 * b) % 255).astype(np.uint8)


def checksum(*arrays):
    """order-sensitive float64 digest of the finite values + the count of non-finite ones"""
    out = []
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        fin = np.isfinite(a)
        out += [float(np.dot(np.where(fin, a, 0.0), 1.0 + (np.arange(a.size) % 31))), float((~fin).sum())]
    return np.array(out)


# ---- the restatement ----
def wing(pred, target, omega=OMEGA, epsilon=EPSILON, count_nan=False, boundary_to_log=False, C=None):
    """sum of the branch terms / number of elements in a branch; count_nan / boundary_to_log / C: the wrong variants of the bite tests"""
    d = np.abs(np.asarray(target, dtype=np.float64) - np.asarray(pred, dtype=np.float64)).ravel()
    if C is None:
        C = omega - omega * np.log(1.0 + omega / epsilon)
    with np.errstate(invalid='ignore'):
        lo = (d <= omega) if boundary_to_log else (d < omega)
        hi = (d > omega) if boundary_to_log else (d >= omega)
    total = (omega * np.log(1.0 + d[lo] / epsilon)).sum() + (d[hi] - C).sum()
    count = d.size if count_nan else int(lo.sum() + hi.sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64(total) / np.float64(count)


def param_loss(a, b, mode='normal', aligned=False):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if mode == 'normal':
        return np.sqrt(((a[:, :12] - b[:, :12]) ** 2).mean(1) + ((a[:, 12:62] - b[:, 12:62]) ** 2).mean(1))
    assert mode == 'only_3dmm'
    lhs = a[:, 12:62] if aligned else a[:, :50]              # aligned: the wrong variant
    return np.sqrt(((lhs - b[:, 12:62]) ** 2).mean(1))


def graph_losses(param, target, lmk, lmk_gt, lmk_refined, param_rev, aligned=False):
    """model_building.py:146-155 from the graph's tensors -> the five weighted losses in LOSS_NAMES order"""
    return (WEIGHTS[0] * wing(lmk, lmk_gt), WEIGHTS[1] * wing(lmk_refined, lmk_gt), WEIGHTS[2] * param_loss(param, target),
            WEIGHTS[3] * param_loss(param_rev, target, 'only_3dmm', aligned), WEIGHTS[4] * param_loss(param_rev, param, 'only_3dmm', aligned))


def center_crop(img, margin):
    """[..., H, W, C]: the interior [margin, H - margin) x [margin, W - margin) survives"""
    img = np.asarray(img)
    out = np.zeros_like(img)
    H, W = img.shape[-3], img.shape[-2]
    if H - margin > margin and W - margin > margin:
        out[..., margin:H - margin, margin:W - margin, :] = img[..., margin:H - margin, margin:W - margin, :]
    return out


def average_meter(batch_dicts, sizes):
    """main_train.py:128-134 in float64: every loss's batch mean (a 0-d loss is its own mean) weighs in with the batch size, and so does
    the sum of the five means -> {name: average} + 'loss_total'"""
    acc, n = np.zeros(6), 0.0
    for d, B in zip(batch_dicts, sizes):
        means = [float(np.mean(np.asarray(d[k], dtype=np.float64))) for k in LOSS_NAMES]
        acc[:5] += np.array(means) * B
        acc[5] += sum(means) * B
        n += B
    return dict(zip(LOSS_NAMES + ('loss_total',), acc / n))


def same_class(got, want):
    """NaN and inf results are compared by class"""
    got, want = float(got), float(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    if np.isinf(want):
        return got == want
    return bool(np.isfinite(got))
