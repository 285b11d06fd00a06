"""Train-time augmentation without a GPU and without the reference: a numpy restatement of the reference's training
transform written from the formulas (ColorJitter through PIL's ImageEnhance / Image.blend / convert('L'), CenterCrop in its train form,
Normalize), the table of cases tests/golden/make_augment_golden.py records with the REAL classes, and the wrong variants the fixture
has to catch.  Integers and fp32 only: every comparison is bit for bit.

Record fields as include/synergy_hip.h syn_train_record: op 0 skip, 1 brightness, 2 contrast, 3 saturation; mask 0..7."""
import itertools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'augment_golden.npz')
F32 = np.float32
SKIP, BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2, 3
ORDERS = tuple(itertools.permutations((BRIGHTNESS, CONTRAST, SATURATION)))          # all six
SPECIAL_FACTORS = (0.0, 0.6, 0.8, 1.0, 1.2, 1.4, 3.0)       # 0.6 / 0.8 / 1.2: where a fused multiply-add changes bytes; 3.0: below 0, above 255
NORM_A, NORM_B = (127.5, 128.0), (110.25, 57.375)           # the reference's, and one whose std is no power of two (both exact in fp32)
DRAW_SEED, DRAW_COUNT, DRAW_PROB = 20240607, 64, 0.5


# ---------------------------------------------------------------------------------------------- the restatement
def grey(x, swapped=False):
    """PIL convert('L') of uint8 [..., 3] -> integers; channel 0 is whatever lies first in memory"""
    c = x.astype(np.int64)
    a, b = (2, 0) if swapped else (0, 2)
    return (19595 * c[..., a] + 38470 * c[..., 1] + 7471 * c[..., b] + 32768) >> 16


def blend(d, x, f, fused=False):
    """PIL Image.blend(degenerate d, image x, f) per byte; d, x integer arrays of one shape.  fused: the product and the sum rounded
    ONCE, as a fused multiply-add does (exact in fp64: 24 + 9 bits of product, 8 bits of d)."""
    f = F32(f)
    diff = (x.astype(np.int64) - d.astype(np.int64))
    if fused:
        t = (d.astype(np.float64) + np.float64(f) * diff.astype(np.float64)).astype(F32)
    else:
        t = d.astype(F32) + (f * diff.astype(F32)).astype(F32)
    if F32(0) <= f <= F32(1):
        return t.astype(np.int64) & 255
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64)))


def contrast_mean(x, round_down=False, swapped=False):
    n = x.shape[0] * x.shape[1]
    s = int(grey(x, swapped).sum())
    return s // n if round_down else (2 * s + n) // (2 * n)


def jitter(x, ops, factors, fused=False, swapped=False, stale_mean=False, round_down=False):
    """the colour steps in the order given -> uint8 [H,W,3].  stale_mean: the contrast mean of the image as it ARRIVED (wrong)."""
    first = x
    x = x.astype(np.int64)
    for op, f in zip(ops, factors):
        if op == SKIP:
            continue
        if op == BRIGHTNESS:
            d = np.zeros_like(x)
        elif op == CONTRAST:
            d = np.full_like(x, contrast_mean(first if stale_mean else x, round_down, swapped))
        elif op == SATURATION:
            d = np.repeat(grey(x, swapped)[..., None], 3, axis=2)
        else:
            raise ValueError(op)
        x = blend(d, x, f, fused)
    return x.astype(np.uint8)


def keep_box(H, W, margin, mask, true_rdown=False, center_floor=False):
    """rows [r0, r1) x columns [c0, c1) that survive CenterCrop(margin) in its train form with mask kind `mask`"""
    r0, r1, c0, c1 = 0, H, 0, W
    if mask in (1, 2, 4):
        r1 = H // 2
    if mask == 3:
        r0 = H // 2
    if mask in (1, 3, 4, 5):
        c1 = W // 2
    if mask in (2, 6):
        c0 = W // 2
    if mask == 4 and true_rdown:
        r0, r1, c0, c1 = H // 2, H, W // 2, W
    if mask == 7:
        r0, r1, c0, c1 = H // 4, H + ((-H) // 4), W // 4, W + ((-W) // 4)
        if center_floor:
            r1, c1 = H - H // 4, W - W // 4
    return max(r0, margin), min(r1, H - margin), max(c0, margin), min(c1, W - margin)


def crop_mask(x, margin, mask, **wrong):
    r0, r1, c0, c1 = keep_box(x.shape[0], x.shape[1], margin, mask, **wrong)
    out = np.zeros_like(x)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = x[r0:r1, c0:c1]
    return out


def normalize(u8, mean, std):
    """uint8 [H,W,3] -> fp32 [3,H,W]: fp32(fp32(byte - mean) / std), numpy's fp32 division is correctly rounded"""
    return np.ascontiguousarray(((u8.astype(F32) - F32(mean)) / F32(std)).astype(F32).transpose(2, 0, 1))


def train_transform(x, ops, factors, mask, margin, mean, std, box_wrong=None, **wrong):
    """-> (uint8 [H,W,3], fp32 [3,H,W]) of one face"""
    u8 = crop_mask(jitter(x, ops, factors, **wrong), margin, mask, **(box_wrong or {}))
    return u8, normalize(u8, mean, std)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- images (built from integers)
def _lcg(seed):
    s = seed & 0xFFFFFFFF
    while True:
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        yield s >> 8


def image(H, W, seed, coarse=False):
    g = _lcg(seed)
    a = np.array([next(g) & 255 for _ in range(H * W * 3)], dtype=np.uint8).reshape(H, W, 3)
    return (a & 0xF0) | 8 if coarse else a


def smooth_image(H, W, seed):
    """a 120 x 120-sized stand-in for a photograph that compresses: ramps with a coarse texture"""
    y, x = np.mgrid[0:H, 0:W]
    c = np.stack([(2 * x + y + seed) % 256, (x + 2 * y + 3 * seed) % 256, (255 - x - y + 5 * seed) % 256], axis=2)
    return ((c & 0xFC) ^ (((x // 8 + y // 8) % 2) * 0x30)[..., None]).astype(np.uint8)


def grey_sum_image(H, W, total):
    """grey pixels (c, c, c has L = c) whose grey values add up to `total`"""
    n = H * W
    v = np.full(n, total // n, dtype=np.uint8)
    v[:total - n * (total // n)] += 1
    return np.repeat(v.reshape(H, W, 1), 3, axis=2)


def _rand_factor(g):
    return 0.6 + 0.8 * (next(g) % 10001) / 10000.0


# ---------------------------------------------------------------------------------------------- the case table
def build_groups():
    """-> list of dicts: name, src uint8 [N,H,W,3], margin, mean, std, and per case src_index / op [B,3] / factor [B,3] float64 /
    mask [B].  One group is one launch's worth: one shape, one margin, one normalisation."""
    groups = []

    def group(name, srcs, margin, norm, cases):
        B = len(cases)
        g = dict(name=name, src=np.stack(srcs), margin=margin, mean=norm[0], std=norm[1],
                 src_index=np.array([c[0] for c in cases], dtype=np.int32), op=np.array([c[1] for c in cases], dtype=np.uint8).reshape(B, 3),
                 factor=np.array([c[2] for c in cases], dtype=np.float64).reshape(B, 3), mask=np.array([c[3] for c in cases], dtype=np.uint8))
        groups.append(g)

    def sweep(n_src, count, seed, masks=range(8)):
        g, out, masks = _lcg(seed), [], list(masks)
        for i in range(count):
            S = SPECIAL_FACTORS
            fac = (S[i % 7], S[(3 * i + 1) % 7], S[(5 * i + 2) % 7]) if i % 3 != 2 else (_rand_factor(g), _rand_factor(g), _rand_factor(g))
            out.append((i % n_src, ORDERS[i % 6], fac, masks[(i // 6 + i) % len(masks)]))
        return out

    groups_spec = [('p1x1', 1, 1, 0, NORM_A, 14), ('p3x2', 3, 2, 0, NORM_A, 16), ('p3x2_m1', 3, 2, 1, NORM_A, 3),
                   ('p7x5_m1', 7, 5, 1, NORM_B, 16), ('p16x33_m5', 16, 33, 5, NORM_A, 16), ('p16x33_m0', 16, 33, 0, NORM_B, 8),
                   ('p4x4_m2', 4, 4, 2, NORM_A, 4)]
    for k, (name, H, W, margin, norm, count) in enumerate(groups_spec):
        srcs = [image(H, W, 101 + 10 * k), image(H, W, 102 + 10 * k, coarse=True), image(H, W, 103 + 10 * k)]
        group(name, srcs, margin, norm, sweep(3, count, 7 + k))
    # 7 x 5, margin 0: every order with every mask kind (the odd //2, //4 and (-h)//4)
    srcs = [image(7, 5, 201), np.maximum(image(7, 5, 202), 1), image(7, 5, 203, coarse=True)]
    g, cases = _lcg(5), []
    for i, (order, mask) in enumerate(itertools.product(ORDERS, range(8))):
        S = SPECIAL_FACTORS
        fac = (S[(i + 1) % 7], S[(2 * i + 3) % 7], S[(3 * i + 5) % 7]) if i % 2 else (_rand_factor(g), _rand_factor(g), _rand_factor(g))
        cases.append((1 if mask in (4, 7) else i % 3, order, fac, mask))            # masks 4 and 7 on the image without a zero byte
    group('p7x5_m0', srcs, 0, NORM_A, cases)
    # 4 x 4 specials: all 255 under brightness 1.4, a uniform image, grey means exactly k + 0.5 and just below, repeats and skips
    srcs = [np.full((4, 4, 3), 255, np.uint8), np.full((4, 4, 3), 77, np.uint8), grey_sum_image(4, 4, 16 * 90 + 8),
            grey_sum_image(4, 4, 16 * 90 + 7), image(4, 4, 301)]
    cases = [(0, (BRIGHTNESS, SKIP, SKIP), (1.4, 1.0, 1.0), 0), (0, ORDERS[3], (1.4, 0.6, 1.2), 0), (1, ORDERS[0], (0.8, 1.2, 0.6), 0),
             (1, ORDERS[5], (3.0, 3.0, 3.0), 7), (2, (CONTRAST, SKIP, SKIP), (0.5, 1.0, 1.0), 0), (3, (CONTRAST, SKIP, SKIP), (0.5, 1.0, 1.0), 0),
             (2, (SKIP, CONTRAST, SKIP), (1.0, 0.0, 1.0), 0), (3, (SKIP, SKIP, CONTRAST), (1.0, 1.0, 0.0), 0),
             (4, (CONTRAST, CONTRAST, SATURATION), (1.3, 0.7, 3.0), 2), (4, (SKIP, SKIP, SKIP), (1.0, 1.0, 1.0), 6),
             (4, (BRIGHTNESS, BRIGHTNESS, CONTRAST), (0.6, 1.4, 0.0), 0), (4, (SATURATION, BRIGHTNESS, SATURATION), (0.0, 1.2, 1.4), 3)]
    group('p4x4_special', srcs, 0, NORM_A, cases)
    # two pixels: grey mean exactly k + 0.5, and its neighbour with one grey level less
    srcs = [grey_sum_image(1, 2, 21), grey_sum_image(1, 2, 20), grey_sum_image(1, 2, 255 + 254)]
    group('p1x2_half', srcs, 0, NORM_A, [(i, (CONTRAST, SKIP, SKIP), (f, 1.0, 1.0), 0) for i in range(3) for f in (0.0, 0.5)])
    # 120 x 120, the reference's margin 5: a handful
    srcs = [image(120, 120, 401), smooth_image(120, 120, 7)]
    cases = [(0, ORDERS[0], (0.6, 0.8, 1.2), 0), (0, ORDERS[4], (1.2, 0.6, 0.8), 7), (1, ORDERS[3], (1.4, 3.0, 0.8), 4),
             (1, ORDERS[5], (0.8731, 1.2217, 0.6449), 0), (0, ORDERS[2], (3.0, 0.6, 1.0), 6)]
    group('p120', srcs, 5, NORM_A, cases)
    group('p120_m60', srcs[1:], 60, NORM_A, [(0, ORDERS[1], (0.9, 1.1, 1.3), 0)])
    return groups


def group_expected(g, **wrong):
    """the restatement over one group -> (uint8 [B,H,W,3], fp32 [B,3,H,W])"""
    u8, f32 = [], []
    for i in range(len(g['mask'])):
        a, b = train_transform(g['src'][g['src_index'][i]], g['op'][i], g['factor'][i], int(g['mask'][i]), int(g['margin']),
                               float(g['mean']), float(g['std']), **wrong)
        u8.append(a)
        f32.append(b)
    return np.stack(u8), np.stack(f32)


def load_golden():
    """the recording -> {group name: dict as build_groups() gives, plus 'u8' / 'f32' as the reference produced them}, and the draws"""
    z = dict(np.load(GOLDEN, allow_pickle=False))
    groups = {}
    for name in [str(n) for n in z['groups']]:
        groups[name] = dict(name=name, **{k: z[f'{name}.{k}'] for k in ('src', 'margin', 'mean', 'std', 'src_index', 'op', 'factor', 'mask', 'u8', 'f32')})
    draws = {k[len('draws.'):]: v for k, v in z.items() if k.startswith('draws.')}
    return groups, draws, z
