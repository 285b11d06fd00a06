"""GPU tests of the batched FaceBoxes detector: syn_detect_batch (N frames of one size in the launches of syn_detect, a frame index on
every kernel, counts left on the device), FaceBoxes.detect_batch / call_batch (frames grouped by size, one upload per group, one
synchronisation per call) and get_all_outputs_batch detecting through call_batch.

The contract is BITWISE: the per-thread arithmetic of the kernels does not see the frame index, and the sort on unique
[score | ~prior] keys removes the order in which the atomics appended the candidates, so a frame's rows equal those of the single-frame
call on that frame whatever the batch size, the slice it falls into and its neighbours are.  Every comparison with the per-frame
result below is therefore np.array_equal; only the comparison with the reference's golden keeps that test's tolerances."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CONF, NMS, TOP_K, KEEP = 0.05, 0.3, 5000, 750


@pytest.fixture(scope='module')
def det():
    from synergynet_amd import synth
    from synergynet_amd.faceboxes import FaceBoxes
    return FaceBoxes(state_dict=synth.make_faceboxes_state())


@pytest.fixture(scope='module')
def five(det):
    """Five 97x131 frames (every cdiv level of the network rounds), frame 4 a copy of frame 0, and detect_all of each."""
    from synergynet_amd import synth
    frames = [synth.make_frame(97, 131, seed=40 + i) for i in range(4)]
    frames.append(frames[0].copy())
    want = [det.detect_all(f) for f in frames]
    assert all(w.shape[0] > 0 for w in want) and not np.array_equal(want[0], want[1])
    return frames, want


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (i, g.shape, w.shape)
        assert np.array_equal(g, w), i


def _raw_batch(det, block, conf_thr=CONF, top_k=TOP_K, keep=KEEP, dets=None, counts=None, n=None, n_dets_null=False):
    """syn_detect_batch on a device block [N,H,W,3] -> (dets [N,keep,5], counts [N]) as numpy, after one synchronisation."""
    import torch
    from synergynet_amd import abi
    N, h, w = (int(v) for v in block.shape[:3])
    scale = det.frame_scale(h, w)
    hs, ws = det.scaled_size(h, w, scale)
    dets = torch.empty((N, keep, 5), device='cuda') if dets is None else dets
    counts = torch.full((N,), -7, dtype=torch.int32, device='cuda') if counts is None else counts
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().syn_detect_batch(det._h, block.data_ptr(), N if n is None else n, h, w, hs, ws, float(scale), conf_thr, NMS, top_k,
                                         keep, dets.data_ptr(), None if n_dets_null else counts.data_ptr(), stream))
    torch.cuda.synchronize()
    return dets.cpu().numpy(), counts.cpu().numpy()


def _raw_single(det, frame_t, conf_thr=CONF, top_k=TOP_K, keep=KEEP):
    import torch
    from synergynet_amd import abi
    h, w = (int(v) for v in frame_t.shape[:2])
    scale = det.frame_scale(h, w)
    hs, ws = det.scaled_size(h, w, scale)
    out = torch.empty((keep, 5), device='cuda')
    n = C.c_int(0)
    abi.check(abi.lib().syn_detect(det._h, frame_t.data_ptr(), h, w, hs, ws, float(scale), conf_thr, NMS, top_k, keep, out.data_ptr(),
                                   C.byref(n), None))
    return out[:n.value].cpu().numpy()


def test_a_frames_result_does_not_depend_on_the_batch(det, five):
    frames, want = five
    got = det.detect_batch(frames)
    _same(got, want)
    assert np.array_equal(got[0], got[4])
    _same(det.detect_batch(frames[:1]), want[:1])                        # N = 1
    _same(det.detect_batch(frames, max_frames=2), want)                  # slices 2 + 2 + 1
    _same(det.detect_batch(np.stack(frames)), want)                      # one [N,H,W,3] block


def test_smallest_geometry(det):
    from synergynet_amd import synth
    frames = [synth.make_frame(33, 47, seed=s) for s in (47, 48, 49)]    # the smallest grid the suite uses: 2x2 cells + 1 + 1, 86 priors
    assert det._lib.syn_detector_prior_count(33, 47) == 86
    _same(det.detect_batch(frames), [det.detect_all(f) for f in frames])


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_batch_entries_match_reference_golden(det, tag):
    from synergynet_amd import synth
    g = np.load(os.path.join(HERE, 'golden', 'faceboxes_golden.npz'))
    hh, ww = [int(v) for v in g[tag + '_hw']]
    frame = synth.make_frame(hh, ww, seed=hh)
    got = det.detect_batch([frame, synth.make_frame(hh, ww, seed=hh + 1), frame])
    want = g[tag + '_dets']
    for k in (0, 2):
        assert got[k].shape == want.shape
        np.testing.assert_allclose(got[k][:, 4], want[:, 4], rtol=0, atol=1e-5)
        np.testing.assert_allclose(got[k][:, :4], want[:, :4], rtol=0, atol=1e-2)
    assert not np.array_equal(got[1], got[0])


@pytest.mark.parametrize('hw', [(366, 1647), (800, 1300)])
def test_downscaling_branch_in_a_batch(det, hw):
    """366x1647: the scaled height differs between python-double and float32 arithmetic (239 vs 240 rows)."""
    from synergynet_amd import synth
    assert det.frame_scale(*hw) != 1
    frames = [synth.make_frame(*hw, seed=hw[1] + i) for i in range(2)]
    _same(det.detect_batch(frames), [det.detect_all(f) for f in frames])


def test_more_candidates_than_the_sorter_holds_per_frame(det):
    import torch
    from synergynet_amd import abi, synth
    block = torch.from_numpy(np.stack([synth.make_frame(720, 1080, seed=5 + i) for i in range(2)])).cuda()
    thr = 1e-4
    rows, counts = _raw_batch(det, block, conf_thr=thr)
    for i in range(2):
        want = _raw_single(det, block[i], conf_thr=thr)
        assert want.shape[0] > 0 and counts[i] == want.shape[0]
        assert np.array_equal(rows[i, :counts[i]], want), i
    with pytest.raises(abi.SynergyHipError, match='top_k'):
        _raw_batch(det, block, conf_thr=thr, top_k=9000)


def test_counters_are_per_frame_and_per_call(det, five):
    import torch
    frames, want = five
    block = torch.from_numpy(np.stack(frames[:4])).cuda()
    dets = torch.empty((4, KEEP, 5), device='cuda')
    counts = torch.empty((4,), dtype=torch.int32, device='cuda')
    rows1, cnt1 = _raw_batch(det, block, dets=dets, counts=counts)
    assert cnt1.tolist() == [w.shape[0] for w in want[:4]]
    _, cnt0 = _raw_batch(det, block, conf_thr=2.0, dets=dets, counts=counts)      # no score exceeds 2
    assert cnt0.tolist() == [0, 0, 0, 0]
    rows2, cnt2 = _raw_batch(det, block, dets=dets, counts=counts)
    assert np.array_equal(cnt2, cnt1)
    for i in range(4):
        assert np.array_equal(rows2[i, :cnt2[i]], rows1[i, :cnt1[i]]) and np.array_equal(rows2[i, :cnt2[i]], want[i])


def test_workspace_regrowth_and_poison(five):
    """A handle of its own: its scratch starts empty and regrows at N = 6."""
    from synergynet_amd import abi, synth
    from synergynet_amd.faceboxes import FaceBoxes
    frames, want = five
    d = FaceBoxes(state_dict=synth.make_faceboxes_state())
    six = frames + [frames[1]]
    _same(d.detect_batch(six[:1]), want[:1])
    _same(d.detect_batch(six), want + [want[1]])
    _same(d.detect_batch(six[2:4]), want[2:4])
    abi.check(abi.lib().syn_debug_poison_workspace(d._h, 1, 0xFF))
    _same(d.detect_batch(frames), want)


def test_mixed_sizes_come_back_in_input_order(det):
    from synergynet_amd import synth
    sizes = [(300, 420), (240, 320), (300, 420), (33, 47)]
    frames = [synth.make_frame(h, w, seed=200 + i) for i, (h, w) in enumerate(sizes)]
    want = [det.detect_all(f) for f in frames]
    assert not np.array_equal(want[0], want[2])
    got = det.detect_batch(frames)
    assert len(got) == 4
    _same(got, want)
    calls = [det(f) for f in frames]
    assert sum(len(c) for c in calls) > 0
    assert det.call_batch(frames) == calls


def test_device_resident_form(det, five):
    import torch
    frames, want = five
    out = det.detect_batch(frames, to_host=False)
    assert len(out) == 5
    torch.cuda.synchronize()
    for (d, c), w in zip(out, want):
        assert d.is_cuda and c.is_cuda and tuple(d.shape) == (KEEP, 5) and c.dim() == 0 and c.dtype == torch.int32
        assert np.array_equal(d[:int(c)].cpu().numpy(), w)
    # device frames in, device rows out
    out = det.detect_batch([torch.from_numpy(f).cuda() for f in frames], to_host=False)
    torch.cuda.synchronize()
    for (d, c), w in zip(out, want):
        assert np.array_equal(d[:int(c)].cpu().numpy(), w)


def test_refusals_leave_the_handle_usable(det, five):
    import torch
    from synergynet_amd import abi
    frames, want = five
    block = torch.from_numpy(np.stack(frames)).cuda()
    with pytest.raises(abi.SynergyHipError, match='N=0'):
        _raw_batch(det, block, n=0)
    with pytest.raises(abi.SynergyHipError, match='NULL'):
        _raw_batch(det, block, n_dets_null=True)
    with pytest.raises(abi.SynergyHipError, match='N='):                 # refused on the host before any buffer is touched
        _raw_batch(det, block, n=abi.SYN_DETECT_BATCH_MAX_FRAMES + 1)
    _same(det.detect_batch(frames), want)
    with pytest.raises(ValueError):
        det.detect_batch([np.zeros((10, 10), np.uint8)])
    with pytest.raises(ValueError):
        det.detect_batch([np.zeros((10, 10, 3), np.float32)])


def test_the_entry_point_detects_through_call_batch(det, monkeypatch):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(n_vert=640), backbone_state=synth.make_backbone_state(), face_detector=det)
    frames = [synth.make_frame(300, 420, seed=300), synth.make_frame(240, 320, seed=302), synth.make_frame(300, 420, seed=303)]
    rects = [[list(r) for r in det(f)] for f in frames]
    assert sum(len(r) for r in rects) > 0
    want = m.get_all_outputs_batch(frames, rects=[[list(r) for r in fr] for fr in rects])

    def same(out):
        assert len(out) == len(want) == 3
        for (l, v, p), (l2, v2, p2) in zip(out, want):
            assert len(l) == len(l2) and len(v) == len(v2) and len(p) == len(p2)
            for a, b in zip(l, l2):
                assert np.array_equal(a, b)
            for a, b in zip(v, v2):
                assert np.array_equal(a, b)
            for (a, ta), (b, tb) in zip(p, p2):
                assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(ta), np.asarray(tb))

    def no_detect_all(*a, **k):
        raise AssertionError('the batch entry point went through detect_all')
    with monkeypatch.context() as mp:
        mp.setattr(det, 'detect_all', no_detect_all)
        same(m.get_all_outputs_batch(frames))
    # a user's own detector is any callable: no call_batch, the per-frame loop
    m.face_detector = lambda f: det(f)
    same(m.get_all_outputs_batch(frames))
