"""The premises of tests/detector_cases.py, asserted on the CPU: every case is what its name says (the cut falls inside a tie group, the
exact IoUs are exact, C survives and B does not, every list has unique keys, ...), and the numpy statement `select_nms` agrees with the
oracle's cpu_nms wherever scores do not tie.  tests/test_gpu_detector_edges.py holds det_nms_kernel / det_preproc_kernel to the same cases."""
import numpy as np
import pytest

import detector_cases as dc
from oracle import faceboxes_torch as ofb

f32 = np.float32


def all_cases():
    return [c for g in dc.GROUP_NAMES for c in dc.groups()[g]]


def sorted_rows(c):
    n = min(c.n_cand, c.max_cand)
    key = dc.sort_key(c.rows[:n], c.prior[:n])
    order = np.argsort(key, kind='stable')[::-1]
    return c.rows[:n][order], c.prior[:n][order], key[order]


def test_every_list_has_unique_keys_and_is_not_sorted():
    assert set(dc.groups()) == set(dc.GROUP_NAMES)
    for c in all_cases():
        n = min(c.n_cand, c.max_cand)
        assert c.rows.shape == (n, 5) and 1 <= c.top_k <= dc.SORT_CAPACITY and c.keep_top_k >= 1 and c.max_cand >= 1
        key = dc.sort_key(c.rows, c.prior)
        assert np.unique(key).size == n, c.name
        assert np.unique(c.prior).size == n, c.name                                    # prior indices are unique per frame
        assert np.all(c.rows[:, 4] > 0) and not np.any(c.rows == dc.SENTINEL), c.name    # positive scores: bit order is value order
        if n >= 1000:
            assert np.mean(np.diff(key.astype(np.float64)) < 0) < 0.6, c.name            # appended in no particular order
            assert 'top byte' in c.name or (c.prior < (1 << 16)).any() and ((c.prior >= (1 << 16)) & (c.prior < (1 << 24))).any() and (c.prior >= (1 << 24)).any(), c.name
        # the order select_nms uses (score descending, lower prior first) is the order of the kernel's keys
        order = np.lexsort((c.prior, -c.rows[:, 4].astype(np.float64)))
        assert np.array_equal(key[order], np.sort(key)[::-1]), c.name
        cand, cnt = dc.pack_candidates(c)
        assert cand.shape == (c.max_cand, 6) and cnt == c.n_cand
        assert np.array_equal(cand[n:, :5].view(f32), np.broadcast_to(dc.POISON, (c.max_cand - n, 5)))


def network_size(n):
    """det_nms_kernel's choice: 1024 slots at least, the next power of two"""
    sn = 1024
    while sn < n:
        sn <<= 1
    return sn


def test_counts_reach_every_network_size_and_the_select():
    assert dc.COUNTS == (0, 1, 2, 1023, 1024, 1025, 2048, 2049, 4097, 8191, 8192, 8193, 12000)
    sizes = {network_size(n) for n in dc.COUNTS if n <= dc.SORT_CAPACITY}
    assert sizes == {1024, 2048, 4096, 8192}
    assert sum(n > dc.SORT_CAPACITY for n in dc.COUNTS) == 2
    for n in dc.COUNTS:
        ks = {c.top_k for c in dc.count_cases(n)}
        assert ks == {k for k in (1, n - 1, n, n + 1, 5000, 8192) if 1 <= k <= 8192}, n
    for n in (1023, 2049, 8193, 12000):
        c = [c for c in dc.count_cases(n) if c.top_k == min(n, 8192)][0]
        kept = dc.expected(c.name)[1]
        assert kept >= 200 and min(n, c.top_k) - kept >= 200, (n, kept)                   # hundreds survive and hundreds die


@pytest.mark.parametrize('group', ['ties', 'radix'])
def test_the_cut_falls_inside_a_tie_group(group):
    for c in dc.groups()[group]:
        rows, prior, key = sorted_rows(c)
        if 'distinct' in c.name:
            assert np.unique(rows[:, 4]).size == rows.shape[0]
            continue
        assert c.top_k < rows.shape[0]
        assert key[c.top_k - 1] >> np.uint64(32) == key[c.top_k] >> np.uint64(32), c.name       # same score word on both sides of the cut
        assert key[c.top_k - 1] > key[c.top_k]
        # the tie direction shows: with the higher prior index first, other rows come out
        flipped = dc.select_nms(c.rows, ~c.prior, c.n_cand, c.max_cand, c.top_k, c.nms_thr, c.keep_top_k)[0]
        assert not np.array_equal(flipped, dc.expected(c.name)[0]), c.name
        # and so does the place of the cut: one row fewer or one row more gives another result
        for k in (c.top_k - 1, c.top_k + 1):
            assert not np.array_equal(dc.select_nms(c.rows, c.prior, c.n_cand, c.max_cand, k, c.nms_thr, c.keep_top_k + 1)[0], dc.expected(c.name)[0]), (c.name, k)
    if group == 'ties':
        for c in dc.tie_cases():
            assert np.unique(c.rows[:, 4]).size == 3
        assert sum(c.n_cand > dc.SORT_CAPACITY for c in dc.tie_cases()) == 2 and sum(c.n_cand <= dc.SORT_CAPACITY for c in dc.tie_cases()) == 2


def test_radix_cases_exercise_the_digits_they_name():
    a, b, c, d = dc.radix_cases()
    for case in (a, b, c, d):
        assert case.n_cand > dc.SORT_CAPACITY                                            # the select runs
    bits = lambda case: np.ascontiguousarray(case.rows[:, 4]).view(np.uint32)
    assert np.unique(bits(a) >> 16).size == 1 and np.unique(bits(a)).size == a.n_cand and np.unique(bits(a) & 0xFF).size == 256
    assert np.unique(bits(b) >> 8).size == 1 and np.unique(bits(b)).size == 256
    s = np.sort(bits(a))
    assert np.all(np.diff(s) == 1) and np.nextafter(s[:1].view(f32), f32(2)).view(np.uint32)[0] == s[1]       # a nextafter chain
    assert sorted(np.unique(c.rows[:, 4]).tolist()) == [float(np.finfo(f32).tiny), float(f32(0.05)), 1.0]
    for sc in np.unique(d.rows[:, 4]):
        p = d.prior[d.rows[:, 4] == sc]
        assert p.size == 256 and np.unique(p & 0xFFFFFF).size == 1 and np.unique(p >> 24).size == 256


def test_exact_iou_pairs_are_exact_and_decide_at_the_threshold():
    for v, (a, b, inter, union) in dc.EXACT_IOU.items():
        i32, u32, o32 = dc.iou_terms(np.array(a, f32), np.array([b], f32))
        assert (i32[0], u32[0], o32[0]) == (inter, union, v) and f32(v) == v
        assert np.float64(inter) / np.float64(union) == v                                # ... and in float64
    for c in dc.threshold_cases():
        got, n = dc.expected(c.name)
        ovr = dc.iou_terms(c.rows[0, :4], c.rows[1:, :4])[2][0]
        if 'thr at' in c.name:
            assert c.nms_thr == ovr and n == 1, c.name                                   # >= suppresses
        else:
            assert c.nms_thr == np.nextafter(ovr, f32(1)) and n == 2, c.name
        if 'rounded' in c.name:
            assert any(x != ovr for x in dc.contracted_iou(c.rows[0, :4], c.rows[1, :4])), c.name     # one rounding less: another quotient
    assert sum('rounded' in c.name for c in dc.threshold_cases()) == 8 and sum('exact' in c.name for c in dc.threshold_cases()) == 4


def test_chain_order_and_degenerate_premises():
    by = {c.name: c for c in dc.small_cases()}
    a, b, c_ = (np.array(x, f32) for x in dc.CHAIN)
    thr = by['chain'].nms_thr
    assert dc.iou_terms(a, b[None])[2][0] >= thr and dc.iou_terms(b, c_[None])[2][0] >= thr and dc.iou_terms(a, c_[None])[2][0] < thr
    got, n = dc.expected('chain')
    assert n == 2 and np.array_equal(got[:, :4], np.stack([a, c_]))                      # C survives and B does not
    got, n = dc.expected('chain x400')
    assert n == 800 and np.all((got[:, 4] > 0.8) | (got[:, 4] < 0.5))                      # every A and every C, no B
    big, small = (np.array(x, f32) for x in dc.EXACT_IOU[0.5][:2])
    for name, winner in (('order decides, winner appended first', big), ('order decides, winner appended last', big), ('order decides, small wins', small)):
        got, n = dc.expected(name)
        assert n == 1 and np.array_equal(got[0, :4], winner), name
        assert by[name].rows[0, 4] == by[name].rows[1, 4]
    assert np.array_equal(by['order decides, winner appended first'].rows[::-1], by['order decides, winner appended last'].rows)
    z = by['degenerate zero-area pair']
    inter, union, ovr = dc.iou_terms(z.rows[0, :4], z.rows[1:2, :4])
    assert inter[0] == 0 and union[0] == 0 and np.isnan(ovr[0])                          # 0 / 0: a NaN never suppresses
    assert dc.expected(z.name)[1] == 3
    ng = by['degenerate negative area']
    r = ng.rows[0]
    assert r[2] < r[0] - 1 and (r[2] - r[0] + 1) * (r[3] - r[1] + 1) < 0
    assert dc.iou_terms(r[:4], ng.rows[3:4, :4])[1][0] == 0                              # area -90 against area +90: 0 / 0
    assert dc.expected(ng.name)[1] == 5 and dc.expected('degenerate negative area second')[1] == 2
    assert (by['negative coordinates'].rows[:, :4] < 0).any() and dc.expected('negative coordinates')[1] == 2
    arb = by['arbitrary float32 coordinates']
    assert np.any(arb.rows[:, :4] * 4 != np.round(arb.rows[:, :4] * 4))
    assert 100 < dc.expected(arb.name)[1] < arb.n_cand - 100


def test_keep_top_k_overflow_and_frames():
    cases, survivors = dc.keep_cases()
    assert survivors > 100 and [c.keep_top_k for c in cases] == [1, survivors - 1, survivors, survivors + 9]
    assert [dc.expected(c.name)[1] for c in cases] == [1, survivors - 1, survivors, survivors]
    full = dc.expected(cases[-1].name)[0]
    for c in cases:
        assert np.array_equal(dc.expected(c.name)[0], full[:c.keep_top_k])
    for c in dc.overflow_cases():
        assert c.n_cand == c.max_cand + 5 and c.rows.shape[0] == c.max_cand
        assert dc.expected(c.name)[1] > 100
    assert sum(c.max_cand > dc.SORT_CAPACITY for c in dc.overflow_cases()) == 1
    fr = dc.frame_cases()
    assert tuple(c.n_cand for c in fr) == (12000, 0, 5) == dc.FRAME_COUNTS
    assert len({(c.max_cand, c.top_k, float(c.nms_thr), c.keep_top_k) for c in fr}) == 1
    assert dc.expected(fr[0].name)[1] == fr[0].keep_top_k and dc.expected(fr[1].name)[1] == 0 and 1 <= dc.expected(fr[2].name)[1] <= 5


def test_select_nms_is_cpu_nms_wherever_scores_do_not_tie():
    """oracle.faceboxes_torch.cpu_nms (pinned by the reference's golden detections) on the rows FaceBoxes.py:114-116 hands it"""
    checked = 0
    for c in all_cases():
        n = min(c.n_cand, c.max_cand)
        if np.unique(c.rows[:, 4]).size != n or n == 0:
            continue
        rows = sorted_rows(c)[0][:c.top_k]
        keep = ofb.cpu_nms(rows, c.nms_thr)
        want = rows[keep][:c.keep_top_k]
        got, cnt = dc.expected(c.name)
        assert cnt == want.shape[0] and np.array_equal(got, want), c.name
        checked += 1
    assert checked >= 60
    for n in (600, 3000, 9000):                                                           # random quarter-pixel boxes, FaceBoxes' own parameters
        rng = np.random.default_rng(n)
        xy = rng.integers(0, 4 * 400, (n, 2)) / 4.0
        wh = rng.integers(4 * 10, 4 * 60, (n, 2)) / 4.0
        rows = np.concatenate([xy, xy + wh, dc.unique_scores(n, rng)[:, None]], axis=1).astype(f32)
        got, cnt = dc.select_nms(rows, np.arange(n, dtype=np.uint32), n, n, ofb.TOP_K, ofb.NMS_THRESHOLD, ofb.KEEP_TOP_K)
        srt = rows[np.argsort(-rows[:, 4].astype(np.float64))][:ofb.TOP_K]
        want = srt[ofb.cpu_nms(srt, ofb.NMS_THRESHOLD)][:ofb.KEEP_TOP_K]
        assert cnt == want.shape[0] > 50 and np.array_equal(got, want)


def test_preproc_cases_reach_the_branches_they_name():
    names = [c.name for c in dc.preproc_cases()]
    assert len(set(names)) == len(names)
    sizes = {(c.frames.shape[0],) + c.frames.shape[1:3] + (c.Hs, c.Ws) for c in dc.preproc_cases()}
    for want in ((1, 33, 47, 33, 47), (3, 33, 47, 33, 47), (1, 97, 131, 96, 130), (1, 97, 131, 48, 65), (1, 97, 131, 24, 33), (1, 97, 131, 1, 1),
                 (1, 64, 9, 63, 9), (1, 366, 1647, 239, 1079)):
        assert want in sizes, want
    assert any(c.frames.shape[0] == 2 and (c.Hs, c.Ws) != c.frames.shape[1:3] for c in dc.preproc_cases())
    hi_clamp = lo_clamp = False
    for c in dc.preproc_cases():
        N, H, W = c.frames.shape[:3]
        assert c.frames.dtype == np.uint8 and c.Hs <= H and c.Ws <= W
        want = dc.preproc(c.frames[0], c.Hs, c.Ws)
        assert want.shape == (c.Hs, c.Ws, 3) and want.dtype == np.float32
        if (c.Hs, c.Ws) == (H, W):
            assert np.array_equal(want, c.frames[0].astype(f32) - dc.MEANS)
            continue
        for n_dst, n_src in ((c.Hs, H), (c.Ws, W)):
            s, _ = dc.linear_taps(n_dst, n_src)
            lo_clamp |= bool((s < 0).any())
            hi_clamp |= bool((s >= n_src - 1).any())
        if 'extreme' in c.name:
            v = want + dc.MEANS
            assert set(np.unique(c.frames)) == {0, 255} and v.min() == 0 and v.max() == 255        # both ends of the final clip's range
            assert ((v > 0) & (v < 255)).any()                                                      # and blends in between
    # a target no larger than the source never puts a tap in front of the first sample (the `s < 0` clamp serves cv2's up-scaling only);
    # the clamp at the last sample is reached on every axis that keeps its size
    assert hi_clamp and not lo_clamp
    one = [c for c in dc.preproc_cases() if (c.Hs, c.Ws) == (1, 1)][0]
    fr = one.frames[0].astype(np.int64)                       # 97x131 -> 1x1: position 48 / 65 exactly, fraction 0: the centre pixel
    assert np.array_equal(dc.preproc(one.frames[0], 1, 1)[0, 0], fr[48, 65].astype(f32) - dc.MEANS)
