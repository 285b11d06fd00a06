"""Shared by tests/test_detector_cases_cpu.py and tests/test_gpu_detector_edges.py: the two ends of the FaceBoxes detector that are
exact -- the input stage (det_preproc_kernel: optional fixed-point bilinear down-scale, mean subtraction) and the back end
(det_nms_kernel: top-k by score, greedy NMS) -- stated in numpy, and the cases both are held to.  Every comparison built on this
module is equality of bits: the input stage is integer arithmetic, the NMS is float32 one operation at a time as
FaceBoxes/utils/nms/cpu_nms.pyx:17-68 has it (one correctly rounded IEEE operation per numpy call below).

A select/NMS case is a candidate list as det_decode_kernel leaves it: rows x1, y1, x2, y2, score in the order of the atomic appends
(any order), the prior index of each row (unique per frame), a count that may exceed the list's capacity, and the four parameters of
FaceBoxes.py:114-127 (top_k, nms threshold, keep_top_k; max_cand is the list's capacity).  Rows past the count are filled with
`POISON` rows (score 2, a box that covers everything): a kernel that read one would put it first and suppress the frame.
"""
import functools
from collections import namedtuple

import numpy as np

f32 = np.float32
SORT_CAPACITY = 8192                        # det_sort_capacity(): slots of the in-LDS sort network; more candidates go through the select
MEANS = np.array((104, 117, 123), dtype=np.float32)                      # FaceBoxes.py:90
SENTINEL = np.float32(-12345.5)             # what `dets` holds before the launch; no case has it as a coordinate or score
POISON = np.array([-1e6, -1e6, 1e6, 1e6, 2.0], dtype=np.float32)

Case = namedtuple('Case', 'name rows prior n_cand max_cand top_k nms_thr keep_top_k')
PreprocCase = namedtuple('PreprocCase', 'name frames Hs Ws')


# ------------------------------------------------------------------------------------------------ the operations
def sort_key(rows, prior):
    """the kernel's 64-bit key: score bits << 32 | ~prior index (scores are positive: bit order is value order)"""
    sb = np.ascontiguousarray(np.asarray(rows, dtype=f32)[:, 4]).view(np.uint32).astype(np.uint64)
    return (sb << np.uint64(32)) | (~np.asarray(prior, dtype=np.uint32)).astype(np.uint64)


def iou_terms(a, b):
    """cpu_nms.pyx:38-63 for one box `a` against rows `b`, float32 operation by operation -> (inter, union, ovr)"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32).reshape(-1, 4)
    one, zero = f32(1), f32(0)
    area_a = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    area_b = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    xx1, yy1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    xx2, yy2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    w = np.maximum(zero, xx2 - xx1 + one)
    h = np.maximum(zero, yy2 - yy1 + one)
    inter = w * h
    union = area_a + area_b - inter
    with np.errstate(divide='ignore', invalid='ignore'):
        ovr = inter / union
    assert inter.dtype == union.dtype == ovr.dtype == np.float32
    return inter, union, ovr


def select_nms(rows, prior, n_cand, max_cand, top_k, nms_thr, keep_top_k):
    """-> (dets [n,5] float32, n): the first min(n_cand, max_cand) rows, ordered by score descending (equal scores: lower prior index
    first), cut to top_k, greedy NMS (suppress on ovr >= thr; a NaN never suppresses), cut to keep_top_k."""
    n = min(int(n_cand), int(max_cand))
    rows = np.asarray(rows, dtype=f32)[:n, :5]
    prior = np.asarray(prior, dtype=np.uint32)[:n]
    order = np.lexsort((prior, -rows[:, 4].astype(np.float64)))[:int(top_k)]
    r = rows[order]
    thr = f32(nms_thr)
    dead = np.zeros(r.shape[0], dtype=bool)
    keep = []
    for i in range(r.shape[0]):
        if dead[i]:
            continue
        keep.append(i)
        if i + 1 < r.shape[0]:
            ovr = iou_terms(r[i, :4], r[i + 1:, :4])[2]
            dead[i + 1:] |= ovr >= thr                # False for NaN
    out = r[keep][:int(keep_top_k)]
    return np.ascontiguousarray(out, dtype=f32), out.shape[0]


def preproc(frame, Hs, Ws):
    """FaceBoxes.py:71-90: cv2.resize to (Ws, Hs) when the size changes (the oracle's fixed-point restatement), float32, minus the means"""
    from oracle.faceboxes_torch import resize_linear_u8
    frame = np.asarray(frame)
    img = frame if (Hs, Ws) == frame.shape[:2] else resize_linear_u8(frame, Hs, Ws)
    return img.astype(np.float32) - MEANS


def pack_candidates(case):
    """-> (cand uint32 [max_cand,6]: the bit patterns the kernel reads, POISON rows past the count;  n_cand)"""
    cand = np.empty((case.max_cand, 6), dtype=np.uint32)
    cand[:, :5] = POISON.view(np.uint32)
    cand[:, 5] = 0
    n = min(case.n_cand, case.max_cand)
    assert case.rows.shape == (n, 5) and case.rows.dtype == np.float32 and case.prior.shape == (n,) and case.prior.dtype == np.uint32
    cand[:n, :5] = case.rows.view(np.uint32)
    cand[:n, 5] = case.prior
    return cand, case.n_cand


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case_by_name(name)
    return select_nms(c.rows, c.prior, c.n_cand, c.max_cand, c.top_k, c.nms_thr, c.keep_top_k)


# ------------------------------------------------------------------------------------------------ builders
def unique_priors(n, rng):
    """n distinct uint32 prior indices in shuffled order: small ones, both sides of 2^16 and of 2^24, and the two ends of the range"""
    pinned = np.array([0, 1, 0xFFFF, 0x10000, 0x10001, 0xFFFFFF, 0x1000000, 0x1000001, 0x7F800001, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)
    pool = np.concatenate([rng.integers(0, 1 << 15, n), rng.integers(1 << 16, 1 << 20, n), rng.integers(1 << 24, 1 << 32, n)]).astype(np.uint64)
    pool = np.setdiff1d(np.unique(pool), pinned)
    pool = pool[rng.permutation(pool.size)]
    out = np.concatenate([pinned, pool])[:n] if n >= pinned.size else pool[:n]
    assert np.unique(out).size == n
    return out[rng.permutation(n)].astype(np.uint32)


def unique_scores(n, rng):
    """n distinct float32 scores in (0.05, 1), shuffled: no ties, so the append order is not the sorted order"""
    s = (0.05 + 0.95 * (rng.permutation(n) + 1.0) / (n + 1.0)).astype(f32)
    assert np.unique(s).size == n
    return s


def cluster_boxes(n, rng, max_cluster=8):
    """n boxes on quarter pixels: clusters of 1..max_cluster boxes of about 20 px jittered by up to 6 px (most pairs of one cluster overlap
    above 0.3, some below), cluster centres 48 px apart on a grid (boxes of different clusters rarely touch).  Quarter-pixel coordinates
    below 2^12 keep every area, intersection and union exact in float32."""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, max_cluster + 1)))
    cid = np.repeat(np.arange(len(sizes)), sizes)[:n]
    cx, cy = (cid % 64) * 48.0, (cid // 64) * 48.0
    q = lambda lo, hi: rng.integers(lo * 4, hi * 4 + 1, n) / 4.0
    x1, y1 = cx + q(0, 6), cy + q(0, 6)
    boxes = np.stack([x1, y1, x1 + q(14, 26), y1 + q(14, 26)], axis=1).astype(f32)
    return boxes[rng.permutation(n)]


def _case(name, boxes, scores, prior, top_k, nms_thr=0.3, keep_top_k=SORT_CAPACITY, n_cand=None, max_cand=None):
    rows = np.ascontiguousarray(np.concatenate([np.asarray(boxes, dtype=f32).reshape(-1, 4), np.asarray(scores, dtype=f32).reshape(-1, 1)], axis=1))
    n = rows.shape[0]
    return Case(name, rows, np.asarray(prior, dtype=np.uint32), n if n_cand is None else n_cand, n + 3 if max_cand is None else max_cand,
                int(top_k), f32(nms_thr), int(keep_top_k))


# ------------------------------------------------------------------------------------------------ select / NMS cases
COUNTS = (0, 1, 2, 1023, 1024, 1025, 2048, 2049, 4097, 8191, 8192, 8193, 12000)


def legal_top_ks(n):
    return sorted({k for k in (1, n - 1, n, n + 1, 5000, SORT_CAPACITY) if 1 <= k <= SORT_CAPACITY})


@functools.lru_cache(maxsize=None)
def count_cases(n):
    """n candidates around a size of the sort network (1024 / 2048 / 4096 / 8192 slots) or of the select (> 8192): clustered boxes, distinct scores"""
    rng = np.random.default_rng(100 + n)
    boxes, scores, prior = cluster_boxes(n, rng), unique_scores(n, rng), unique_priors(n, rng)
    return tuple(_case(f'count n={n} top_k={k}', boxes, scores, prior, k) for k in legal_top_ks(n))


def _three_scores(n, counts, values, rng):
    s = np.repeat(np.asarray(values, dtype=f32), counts)
    assert s.size == n
    return s[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def tie_cases():
    """three distinct scores only; the top_k-th and the (top_k+1)-th key share the score word, so the prior index alone decides who enters.
    Every box stands alone (clusters of one), so whoever enters shows in the result."""
    out = []
    for tag, n, counts, top_k in (('select', 9000, (2000, 4000, 3000), 5000), ('select, cut at the network size', 9000, (2000, 4000, 3000), SORT_CAPACITY),
                                  ('network', 3000, (1000, 1000, 1000), 1500), ('network, first group', 5000, (3000, 1000, 1000), 1024)):
        rng = np.random.default_rng(200 + n + top_k)
        out.append(_case(f'ties {tag} n={n} top_k={top_k}', cluster_boxes(n, rng, max_cluster=1), _three_scores(n, counts, (0.9, 0.5, 0.1), rng),
                         unique_priors(n, rng), top_k))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def radix_cases():
    """what each digit of the 8-bit radix select sees: (a) scores that are float32 neighbours, distinct, differing in the two lowest score bytes;
    (b) 256 neighbouring scores, each held by ~35 rows: only the lowest score byte differs, then the prior; (c) scores decades apart: 1.0, 0.05
    and the smallest positive normal; (d) 36 scores, each held by 256 rows whose priors differ only in their top byte."""
    out = []
    n, base = 9000, np.array([0.5], dtype=f32).view(np.uint32)[0]
    rng = np.random.default_rng(301)
    bits = (base + rng.permutation(n).astype(np.uint32)).astype(np.uint32)
    out.append(_case('radix nextafter chain, distinct', cluster_boxes(n, rng, 3), bits.view(f32), unique_priors(n, rng), 5000))
    rng = np.random.default_rng(302)
    bits = (base + (rng.permutation(n) % 256).astype(np.uint32)).astype(np.uint32)
    out.append(_case('radix nextafter chain, lowest byte', cluster_boxes(n, rng, 1), bits.view(f32), unique_priors(n, rng), 5000))
    rng = np.random.default_rng(303)
    out.append(_case('radix decades', cluster_boxes(n, rng, 1), _three_scores(n, (3000, 3000, 3000), (1.0, 0.05, np.finfo(f32).tiny), rng),
                     unique_priors(n, rng), 5000))
    rng = np.random.default_rng(304)
    n = 36 * 256
    g, b = np.divmod(rng.permutation(n), 256)
    prior = ((b.astype(np.uint64) << 24) | (g.astype(np.uint64) + 7)).astype(np.uint32)
    scores = (0.1 + 0.02 * g).astype(f32)
    out.append(_case('radix priors differ in the top byte', cluster_boxes(n, rng, 1), scores, prior, 5000))
    return tuple(out)


# integer boxes whose IoU is exact in float32 and in float64: (box A, box B, inter, union)
EXACT_IOU = {0.5: ((0, 0, 9, 9), (0, 0, 9, 4), 50, 100), 0.25: ((0, 0, 9, 9), (0, 0, 4, 4), 25, 100)}


def _rounded_iou_pairs():
    """pairs of arbitrary float32 boxes whose IoU is NOT exact, with the threshold set to the float32 quotient itself: the pair is suppressed at
    that threshold and kept one ulp above it.  Chosen (deterministically, by search) so that fusing either product of the union into the
    addition or subtraction that follows it -- one rounding instead of two -- gives another quotient: an FMA contraction flips the decision."""
    rng = np.random.default_rng(77)
    pairs = []
    while len(pairs) < 4:
        a = np.concatenate([rng.uniform(0, 20, 2), rng.uniform(30, 60, 2)]).astype(f32)
        b = (a + rng.uniform(-8, 8, 4)).astype(f32)
        ovr = iou_terms(a, b[None])[2][0]
        if not 0.2 < ovr < 0.8:
            continue
        if any(v != ovr for v in contracted_iou(a, b)):
            pairs.append((a, b, ovr))
    return pairs


def contracted_iou(a, b):
    """the quotients a compiler would produce by contracting a multiply of the union expression into the add / subtract that consumes it
    (float64 holds a float32 product exactly; the one rounding to float32 follows the sum)"""
    one = f32(1)
    a32, b32 = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    wa, ha, wb, hb = a32[2] - a32[0] + one, a32[3] - a32[1] + one, b32[2] - b32[0] + one, b32[3] - b32[1] + one
    w = max(f32(0), min(a32[2], b32[2]) - max(a32[0], b32[0]) + one)
    h = max(f32(0), min(a32[3], b32[3]) - max(a32[1], b32[1]) + one)
    area_a, area_b, inter = f32(wa * ha), f32(wb * hb), f32(w * h)
    fused_add = f32(np.float64(wb) * np.float64(hb) + np.float64(area_a))             # fma(wb, hb, area_a)
    fused_sub = f32(np.float64(f32(area_a + area_b)) - np.float64(w) * np.float64(h))   # fma(-w, h, area_a + area_b)
    return f32(inter / f32(fused_add - inter)), f32(inter / fused_sub)


@functools.lru_cache(maxsize=None)
def threshold_cases():
    out = []
    for v, (a, b, _, _) in EXACT_IOU.items():
        for tag, thr in (('at', f32(v)), ('one ulp above', np.nextafter(f32(v), f32(1)))):
            out.append(_case(f'threshold exact IoU {v}, thr {tag}', [a, b], [0.9, 0.8], [70000, 3], 2, nms_thr=thr, keep_top_k=4))
    for i, (a, b, ovr) in enumerate(_rounded_iou_pairs()):
        for tag, thr in (('at', ovr), ('one ulp above', np.nextafter(ovr, f32(1)))):
            out.append(_case(f'threshold rounded IoU pair {i}, thr {tag}', [a, b], [0.9, 0.8], [5, 1 << 25], 2, nms_thr=thr, keep_top_k=4))
    return tuple(out)


CHAIN = ((0, 0, 9, 9), (3, 0, 12, 9), (6, 0, 15, 9))         # A, B, C: IoU(A,B) = IoU(B,C) = 70/130, IoU(A,C) = 40/160


@functools.lru_cache(maxsize=None)
def small_cases():
    out = []
    # chain: A suppresses B; B would have suppressed C; A does not reach C: C survives.  Appended C, A, B.
    a, b, c = CHAIN
    out.append(_case('chain', [c, a, b], [0.7, 0.9, 0.8], [1, 2, 3], 3, keep_top_k=4))
    # the same chain 400 times over, far apart, one score per triple position: 400 live rows between the two ends of each chain
    rng = np.random.default_rng(401)
    off = np.stack([(np.arange(400) % 20) * 64.0, (np.arange(400) // 20) * 64.0] * 2, axis=1)
    boxes = np.concatenate([np.asarray(bx, dtype=np.float64) + off for bx in CHAIN])
    scores = np.concatenate([unique_scores(400, rng) / f32(8) + f32(lvl) for lvl in (0.8, 0.5, 0.2)]).astype(f32)
    p = rng.permutation(1200)
    out.append(_case('chain x400', boxes[p], scores[p], unique_priors(1200, rng)[p], 1200))
    # order decides: equal scores, IoU 0.5 >= thr: the lower prior index wins, whichever was appended first
    big, small = EXACT_IOU[0.5][:2]
    out.append(_case('order decides, winner appended first', [big, small], [0.6, 0.6], [4, 1 << 24], 2, keep_top_k=4))
    out.append(_case('order decides, winner appended last', [small, big], [0.6, 0.6], [1 << 24, 4], 2, keep_top_k=4))
    out.append(_case('order decides, small wins', [small, big], [0.6, 0.6], [0xFFFF, 0x10000], 2, keep_top_k=4))
    # degenerate boxes
    z = (10, 10, 9, 30)                                      # x2 = x1 - 1: zero area
    out.append(_case('degenerate zero-area pair', [z, z, (0, 0, 40, 40)], [0.9, 0.8, 0.7], [3, 2, 1], 3, keep_top_k=4))
    out.append(_case('degenerate zero area under a box', [(0, 0, 40, 40), z, (10, 10, 9, 9)], [0.9, 0.8, 0.7], [3, 2, 1], 3, keep_top_k=4))
    neg = (30, 0, 20, 9)                                     # x2 < x1 - 1: negative area
    # its intersection with anything is empty (w = 0); against a box of area +90 the union is 0 and the quotient 0 / 0: all five are kept
    out.append(_case('degenerate negative area', [neg, (18, 0, 32, 9), (31, 1, 21, 10), (0, 0, 8, 9), (25, 2, 28, 7)], [0.9, 0.8, 0.7, 0.6, 0.5],
                     [9, 8, 7, 6, 5], 5, keep_top_k=8))
    out.append(_case('degenerate negative area second', [(18, 0, 32, 9), neg, (22, 0, 28, 9)], [0.9, 0.8, 0.7], [9, 8, 7], 3, nms_thr=0.1, keep_top_k=8))
    out.append(_case('negative coordinates', [(-50, -50, -41, -41), (-50, -50, -41, -46), (-30.25, -7.5, 2.75, 11), (-28, -6, 3, 12)],
                     [0.9, 0.8, 0.7, 0.6], [1, 2, 3, 4], 4, nms_thr=0.5, keep_top_k=8))
    rng = np.random.default_rng(402)
    n = 1500
    xy = rng.normal(0, 60, (n, 2))
    wh = np.exp(rng.normal(3.0, 0.6, (n, 2)))
    out.append(_case('arbitrary float32 coordinates', np.concatenate([xy, xy + wh], axis=1), unique_scores(n, rng), unique_priors(n, rng), n))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def keep_cases():
    """keep_top_k = 1, one below the number of survivors, the number itself, above it"""
    rng = np.random.default_rng(501)
    n = 700
    boxes, scores, prior = cluster_boxes(n, rng), unique_scores(n, rng), unique_priors(n, rng)
    survivors = select_nms(np.concatenate([boxes, scores[:, None]], axis=1), prior, n, n, n, 0.3, SORT_CAPACITY)[1]
    return tuple(_case(f'keep_top_k={k} of {survivors} survivors', boxes, scores, prior, n, keep_top_k=k)
                 for k in (1, survivors - 1, survivors, survivors + 9)), survivors


@functools.lru_cache(maxsize=None)
def overflow_cases():
    """n_cand = max_cand + 5: the decode kernel counted past a full list; only the first max_cand rows exist"""
    out = []
    for max_cand, top_k in ((600, 600), (9000, 5000)):
        rng = np.random.default_rng(600 + max_cand)
        out.append(_case(f'n_cand past max_cand={max_cand}', cluster_boxes(max_cand, rng), unique_scores(max_cand, rng), unique_priors(max_cand, rng),
                         top_k, n_cand=max_cand + 5, max_cand=max_cand))
    return tuple(out)


FRAME_COUNTS = (12000, 0, 5)
FRAMES_MAX_CAND = 12003


@functools.lru_cache(maxsize=None)
def frame_cases():
    """N = 3 in one launch: a frame that takes the select, an empty one, a tiny one; all share max_cand, top_k and keep_top_k"""
    out = []
    for f, n in enumerate(FRAME_COUNTS):
        rng = np.random.default_rng(700 + f)
        out.append(_case(f'frames[{f}] n={n}', cluster_boxes(n, rng), unique_scores(n, rng), unique_priors(n, rng), 5000, keep_top_k=750,
                         max_cand=FRAMES_MAX_CAND))
    return tuple(out)


def groups():
    """name -> cases; the GPU test takes one group per test"""
    g = {f'count {n}': count_cases(n) for n in COUNTS}
    g.update({'ties': tie_cases(), 'radix': radix_cases(), 'threshold': threshold_cases(), 'small': small_cases(), 'keep_top_k': keep_cases()[0],
              'overflow': overflow_cases(), 'frames': frame_cases()})
    return g


GROUP_NAMES = tuple(f'count {n}' for n in COUNTS) + ('ties', 'radix', 'threshold', 'small', 'keep_top_k', 'overflow', 'frames')


@functools.lru_cache(maxsize=None)
def _by_name():
    out = {}
    for cases in groups().values():
        for c in cases:
            assert c.name not in out, c.name
            out[c.name] = c
    return out


def case_by_name(name):
    return _by_name()[name]


# ------------------------------------------------------------------------------------------------ preproc cases
def noise_frames(N, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def extreme_frames(H, W):
    """columns of 0 and of 255 in runs of 1, 2 and 3 (first column 255, last column 0), and two rows of the opposite value"""
    runs = np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0], dtype=np.uint8)
    col = np.resize(runs, W)
    col[0], col[-1] = 1, 0
    fr = np.broadcast_to((col * 255)[None, :, None], (H, W, 3)).copy()
    fr[H // 3] = 255 - fr[H // 3]
    fr[H - 1] = 255 - fr[H - 1]
    return fr[None]


@functools.lru_cache(maxsize=None)
def preproc_cases():
    c = [PreprocCase('no scaling 33x47', noise_frames(1, 33, 47, 1), 33, 47),
         PreprocCase('no scaling 33x47 N=3', noise_frames(3, 33, 47, 2), 33, 47)]
    for hs, ws in ((96, 130), (48, 65), (24, 33), (1, 1)):
        c.append(PreprocCase(f'97x131 -> {hs}x{ws}', noise_frames(1, 97, 131, 3), hs, ws))
    c.append(PreprocCase('64x9 -> 63x9', noise_frames(1, 64, 9, 4), 63, 9))
    c.append(PreprocCase('366x1647 -> 239x1079', noise_frames(1, 366, 1647, 5), 239, 1079))
    c.append(PreprocCase('97x131 -> 31x77 N=2', noise_frames(2, 97, 131, 6), 31, 77))
    c.append(PreprocCase('extreme 50x70 -> 31x45', extreme_frames(50, 70), 31, 45))
    c.append(PreprocCase('extreme 50x70 -> 49x70', extreme_frames(50, 70), 49, 70))
    c.append(PreprocCase('extreme 50x70 -> 50x23', extreme_frames(50, 70), 50, 23))
    return tuple(c)


def linear_taps(n_dst, n_src):
    """the source position of cv2's bilinear resize before its clamps -> (floor, fraction) as float32 arithmetic has them"""
    fd = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5).astype(f32)
    s = np.floor(fd).astype(np.int64)
    return s, fd - s.astype(f32)
