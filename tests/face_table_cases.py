"""Cases shared by tests/test_face_tables_cpu.py (the arithmetic of csrc/face_tables.h compiled for the host) and
tests/test_gpu_face_tables.py (the kernels): crop sides, detections and padded detector rows, and the values expected for them
from the host code the device path replaces -- inference.lanczos4_tables, SynergyNet._face_tables fed lists of np.float32
scalars (what FaceBoxes returns), faceboxes.split_detections.  Every comparison made with them is integer or bit equality.
Device-free: SynergyNet._face_tables is a staticmethod and imports no library."""
import numpy as np

f32 = np.float32

ALL_SIDES = np.arange(1, 4097, dtype=np.int32)                               # every side 1..4096 in one call
LARGE_SIDES = np.array([5000, 65535, 65536, 2 ** 20 + 1, 2 ** 24], dtype=np.int32)
REPEATED_SIDES = np.array([37, 211, 37], dtype=np.int32)                     # the same side twice in one call
SINGLE_SIDE = np.array([121], dtype=np.int32)                                # n = 1

# heights whose margin floor(h * 1.2 / 2) differs between float32 arithmetic (64, 143, 164, 229: what numpy computes on float32
# detections) and double arithmetic (one less)
MARGIN_HEIGHTS = [106.66666412353516, 238.33331298828125, 273.33331298828125, 381.6666564941406]
MARGINS_F32 = [64, 143, 164, 229]


def host_tables(sides):
    """(ofs [n,120] int32, coef [n,120,8] int16) from inference.lanczos4_tables."""
    from synergynet_amd.inference import lanczos4_tables
    tabs = [lanczos4_tables(int(s)) for s in sides]
    return np.stack([t[0] for t in tabs]).astype(np.int32), np.stack([t[1] for t in tabs]).astype(np.int16)


def random_detections(n=20000, seed=7):
    """float32 [n,5]: sides 8..600, origins overhanging a 1080 x 720 frame, scores in (0.5, 1)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(8, 600, n)
    h = rng.uniform(8, 600, n)
    x1 = rng.uniform(-300, 1080, n)
    y1 = rng.uniform(-300, 720, n)
    return np.stack([x1, y1, x1 + w, y1 + h, rng.uniform(0.5, 1, n)], axis=1).astype(f32)


def margin_rows():
    return np.array([[20.0, 0.0, 20.0 + hh, hh, 0.9] for hh in MARGIN_HEIGHTS], dtype=f32)


def tie_rows():
    """wc - margin ends in .5 with an even (x1 = 10, x2 = 21) and an odd (11, 22) lower neighbour: rint, not round-half-away."""
    return np.array([[10, 5, 21, 45, 0.8], [11, 5, 22, 45, 0.7]], dtype=f32)


GOOD = np.array([[100.25, 50.5, 180.75, 150.0, 0.91], [-20.5, -10.25, 60.0, 90.5, 0.62], [900.0, 600.0, 1100.5, 790.25, 0.77]], dtype=f32)


def degenerate_rows():
    """[(name, row)]: each must give status != 0 (the host path raises 'degenerate detection box')."""
    big = float(2 ** 30 + 1024)
    out = [('y2 == y1', [10, 40, 60, 40, 0.9]), ('y2 < y1', [10, 80, 60, 40, 0.9]), ('height 1.5: margin 0', [10, 40, 60, 41.5, 0.9])]
    for k in range(4):
        for name, v in (('nan', np.nan), ('inf', np.inf), ('-inf', -np.inf)):
            row = [10.0, 40.0, 60.0, 100.0, 0.9]
            row[k] = v
            out.append((f'{name} in coordinate {k}', row))
    # a coordinate of 2^30 + 1024 (its neighbour on the same axis next to it, or the centre would lie at 2^29)
    out += [('x beyond 2^30', [big, 40, big + 128, 100, 0.9]), ('y beyond 2^30', [10, big, 60, big + 128, 0.9]),
            ('x below -2^30', [-big - 128, 40, -big, 100, 0.9])]
    return [(name, np.array(row, dtype=f32)) for name, row in out]


def handmade_detections():
    """(dets float32 [n,5], degenerate [n] bool): the margin heights, the rounding ties, and every degenerate row in the middle of
    good rows."""
    rows, bad = [], []
    for r in list(margin_rows()) + list(tie_rows()):
        rows.append(r)
        bad.append(False)
    for i, (_, r) in enumerate(degenerate_rows()):
        rows += [GOOD[i % 3], r]
        bad += [False, True]
    rows.append(GOOD[1])
    bad.append(False)
    return np.stack(rows).astype(f32), np.array(bad)


def host_face_tables(dets):
    """SynergyNet._face_tables face by face on lists of np.float32 scalars -> dict(roi [n,5], box [n,4], ofs [2,n,120], coef
    [2,n,120,8], bad [n]): for a face on which the host path raises 'degenerate detection box', bad is True, box is (0,0,1,1) and
    the tables are those of side 1 (what the device path is specified to leave there); its roi is not compared."""
    from synergynet_amd.synergy3DMM import SynergyNet
    assert int(np.__version__.split('.')[0]) >= 2, 'the float32 array arithmetic of _face_tables needs NumPy 2'
    dets = np.asarray(dets, dtype=f32)
    n = dets.shape[0]
    roi, box = np.zeros((n, 5), f32), np.zeros((n, 4), np.int32)
    ofs, coef, bad = np.zeros((2, n, 120), np.int32), np.zeros((2, n, 120, 8), np.int16), np.zeros(n, bool)
    o1, c1 = host_tables([1])
    good = []
    with np.errstate(all='ignore'):
        for i in range(n):
            try:
                SynergyNet._face_tables([[[f32(v) for v in dets[i]]]], 1)
                good.append(i)
            except ValueError as e:
                assert 'degenerate detection box' in str(e)
                bad[i] = True
                box[i] = (0, 0, 1, 1)
                ofs[:, i], coef[:, i] = o1[0], c1[0]
    if good:            # the good faces in ONE call (the array form; per face it is the same statement on arrays of length 1)
        r, b, o, c = SynergyNet._face_tables([[[f32(v) for v in dets[i]] for i in good]], len(good))
        roi[good], box[good], ofs[:, good], coef[:, good] = r, b, o, c
    return dict(roi=roi, box=box, ofs=ofs, coef=coef, bad=bad)


def host_face_tables_batch(dets):
    """The same for a batch known to hold no degenerate face, in one call (20 000 faces: no per-face loop)."""
    from synergynet_amd.synergy3DMM import SynergyNet
    dets = np.asarray(dets, dtype=f32)
    r, b, o, c = SynergyNet._face_tables([[[v for v in row] for row in dets]], dets.shape[0])
    return dict(roi=r, box=b, ofs=o, coef=c, bad=np.zeros(dets.shape[0], bool))


# ---- compaction ----
THRES = 0.5


def compaction_cases():
    """[(name, rows [N,K,5] float32, counts [N] int32, order or None)].  Rows past counts[i] carry score 0.99 (poison: they must not
    count); inside the valid prefixes scores lie on both sides of THRES, one equals it and one is NaN."""
    rng = np.random.default_rng(11)

    def make(N, K, counts, scores):
        rows = rng.uniform(0, 500, (N, K, 5)).astype(f32)
        rows[:, :, 4] = 0.99
        for i, s in enumerate(scores):
            rows[i, :len(s), 4] = s
        return rows, np.array(counts, dtype=np.int32)

    cases = []
    r, c = make(1, 4, [3], [[0.9, 0.5, 0.7]])
    cases.append(('N=1 K=4', r, c, None))
    scores = [[], [0.95, np.nan, 0.51], [0.99, 0.8, 0.5, 0.49999, 0.7, 0.2], [0.3, 0.6], []]
    r, c = make(5, 6, [0, 3, 6, 2, 0], scores)
    cases.append(('N=5 K=6', r, c, None))
    cases.append(('N=5 K=6 permuted', r, c, np.array([3, 0, 2, 4, 1], dtype=np.int32)))
    r, c = make(5, 6, [9, -2, 6, 2, 1], [[0.9, 0.8, 0.1, 0.7, 0.6, 0.55], [0.9, 0.9], scores[2], scores[3], [0.75]])
    cases.append(('count above K and negative count', r, c, np.array([1, 2, 0, 4, 3], dtype=np.int32)))
    r, c = make(3, 200, [200, 130, 64], [rng.uniform(0.3, 0.7, 200), rng.uniform(0.3, 0.7, 130), rng.uniform(0.3, 0.7, 64)])
    cases.append(('more rows than a wave', r, c, np.array([2, 0, 1], dtype=np.int32)))
    return cases


def host_compaction(rows, counts, order, thres=THRES):
    """(packed [total,5], face_frame [total], frame_faces [N+1]) from faceboxes.split_detections on the rows in output order.  The
    kernel clamps a count to 0..K; split_detections slices with it, so the clamp is applied here first (a negative count would
    otherwise slice from the end)."""
    from synergynet_amd.faceboxes import split_detections
    N, K = rows.shape[:2]
    order = np.arange(N) if order is None else np.asarray(order)
    per = split_detections(rows[order], np.clip(counts[order], 0, K), thres)
    flat = [r for fr in per for r in fr]
    packed = np.array(flat, dtype=f32).reshape(len(flat), 5)
    face_frame = np.repeat(np.arange(N, dtype=np.int32), [len(fr) for fr in per])
    frame_faces = np.array([len(fr) for fr in per] + [len(flat)], dtype=np.int32)
    return packed, face_frame, frame_faces
