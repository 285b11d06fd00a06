"""GPU tests of the two exact ends of the FaceBoxes detector (run with `-m gpu`), each launched alone through a test hook of the C ABI:
det_nms_kernel (syn_debug_det_select_nms: radix select of the top-k above 8192 candidates, bitonic network of 1024 / 2048 / 4096 / 8192
slots, greedy NMS) on candidate lists made on the host, and det_preproc_kernel (syn_debug_det_preproc: fixed-point bilinear down-scale,
mean subtraction).  Yardstick: the numpy statements of tests/detector_cases.py, whose premises tests/test_detector_cases_cpu.py asserts.
Every comparison is equality of bits: rows, counts, and the sentinel the rows past the count must keep.

On an MI355X every case passed on the kernels as they were: no kernel change was needed.  Each group was shown to bite on a variant
library with one token of det_nms_kernel changed (first failing case per group):
  `ovr > nms_thr`           count n=2048 top_k=2047, count n=8191 top_k=8190, threshold exact IoU 0.5 (thr at), negative coordinates
  key `| idx` (tie flipped) ties select n=9000 top_k=5000, radix nextafter chain lowest byte, order decides (winner appended first)
  select with K - 1         count n=8193 / n=12000 top_k=1 (no row comes out), ties select n=9000 top_k=5000, radix lowest byte
  select with K + 1         count n=8193 / n=12000 top_k=8192, ties select cut at the network size
  union as fmaf(-w, h, ..)  threshold rounded IoU pair 0 (thr at): one rounding less in the union moves the quotient off the threshold"""
import ctypes as C

import numpy as np
import pytest

import detector_cases as dc
from synergynet_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def det():
    from synergynet_amd import synth
    from synergynet_amd.faceboxes import FaceBoxes
    return FaceBoxes(state_dict=synth.make_faceboxes_state())


def run_select_nms(det, cases):
    """the cases as frames of ONE launch (they share max_cand, top_k, nms_thr and keep_top_k) -> per frame (dets [keep_top_k,5], count)"""
    import torch
    c0 = cases[0]
    assert all((c.max_cand, c.top_k, c.nms_thr, c.keep_top_k) == (c0.max_cand, c0.top_k, c0.nms_thr, c0.keep_top_k) for c in cases)
    N = len(cases)
    packed = [dc.pack_candidates(c) for c in cases]
    cand = torch.from_numpy(np.stack([p[0] for p in packed]).view(np.int32)).cuda()
    cnt = torch.tensor([p[1] for p in packed], dtype=torch.int32, device='cuda')
    dets = torch.full((N, c0.keep_top_k, 5), float(dc.SENTINEL), dtype=torch.float32, device='cuda')
    n_out = torch.full((N,), -7, dtype=torch.int32, device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().syn_debug_det_select_nms(det._h, cand.data_ptr(), cnt.data_ptr(), N, c0.max_cand, c0.top_k, C.c_float(float(c0.nms_thr)),
                                                 c0.keep_top_k, dets.data_ptr(), n_out.data_ptr(), stream))
    torch.cuda.synchronize()
    return list(zip(dets.cpu().numpy(), n_out.cpu().numpy().tolist()))


def check(case, got, n):
    want, n_want = dc.expected(case.name)
    assert n == n_want, f'{case.name}: {n} detections, expected {n_want}'
    assert np.array_equal(got[:n], want), f'{case.name}: rows differ, first at {np.argmax((got[:n] != want).any(1))}'
    assert np.all(got[n:] == dc.SENTINEL), f'{case.name}: a row at or after n_dets was written'


@pytest.mark.parametrize('group', [g for g in dc.GROUP_NAMES if g != 'frames'])
def test_select_and_nms_match_the_numpy_statement(det, group):
    """counts on both sides of every sort-network size and of the select with every legal top_k of the table; tie groups across the cut; what
    each radix digit sees; IoUs exactly at the threshold and one ulp below it; suppression chains; equal scores; degenerate boxes; keep_top_k
    below, at and above the number of survivors; a count past the list's capacity."""
    for case in dc.groups()[group]:
        (got, n), = run_select_nms(det, [case])
        check(case, got, n)


def test_frames_of_one_launch_are_their_own_launches(det):
    """N = 3 with 12000, 0 and 5 candidates: every frame's rows and count are those of its own N = 1 launch, and the numpy statement's"""
    cases = dc.frame_cases()
    together = run_select_nms(det, list(cases))
    for case, (got, n) in zip(cases, together):
        (alone, n_alone), = run_select_nms(det, [case])
        assert n == n_alone and np.array_equal(got, alone), case.name
        check(case, got, n)


def test_select_nms_hook_refuses_what_the_detector_refuses(det):
    import torch
    lib = abi.lib()
    buf = torch.zeros(64, dtype=torch.float32, device='cuda')
    cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
    p, q = buf.data_ptr(), cnt.data_ptr()
    ok = dict(cand=p, n_cand=q, N=1, max_cand=4, top_k=4, thr=C.c_float(0.3), keep=4, dets=p, n_dets=q)
    call = lambda **kw: (lambda a: lib.syn_debug_det_select_nms(det._h, a['cand'], a['n_cand'], a['N'], a['max_cand'], a['top_k'], a['thr'], a['keep'],
                                                                a['dets'], a['n_dets'], None))(dict(ok, **kw))
    assert call() == 0
    for bad in (dict(cand=None), dict(n_cand=None), dict(dets=None), dict(n_dets=None), dict(N=0), dict(max_cand=0), dict(top_k=0),
                dict(top_k=dc.SORT_CAPACITY + 1), dict(keep=0)):
        assert call(**bad) == abi.SYN_ERR_INVALID, bad
    assert call(top_k=dc.SORT_CAPACITY) == 0
    with pytest.raises(abi.SynergyHipError, match='top_k'):
        abi.check(call(top_k=9000))
    frames = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device='cuda')
    pre = lambda fr, N, H, W, Hs, Ws, out: lib.syn_debug_det_preproc(det._h, fr, N, H, W, Hs, Ws, out, None)
    out = torch.zeros(4 * 4 * 3, dtype=torch.float32, device='cuda')
    assert pre(frames.data_ptr(), 1, 4, 4, 4, 4, out.data_ptr()) == 0
    for args in ((None, 1, 4, 4, 4, 4, out.data_ptr()), (frames.data_ptr(), 1, 4, 4, 4, 4, None), (frames.data_ptr(), 0, 4, 4, 4, 4, out.data_ptr()),
                 (frames.data_ptr(), 1, 4, 4, 5, 4, out.data_ptr()), (frames.data_ptr(), 1, 4, 4, 4, 5, out.data_ptr()),
                 (frames.data_ptr(), 1, 4, 4, 0, 4, out.data_ptr())):
        assert pre(*args) == abi.SYN_ERR_INVALID, args
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', dc.preproc_cases(), ids=lambda c: c.name)
def test_preproc_is_the_fixed_point_resize_minus_the_means(det, case):
    """uint8 noise frames and frames of 0 / 255 columns, unscaled and scaled (one axis or both, down to 1x1), N = 1, 2, 3: every float equals
    resize_linear_u8's byte minus the channel mean; the floats in front of and behind the output keep their sentinel"""
    import torch
    N, H, W = case.frames.shape[:3]
    body = N * case.Hs * case.Ws * 3
    guard = 256
    flat = torch.full((guard + body + guard,), float(dc.SENTINEL), dtype=torch.float32, device='cuda')
    fr = torch.from_numpy(case.frames).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().syn_debug_det_preproc(det._h, fr.data_ptr(), N, H, W, case.Hs, case.Ws, flat[guard:].data_ptr(), stream))
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert np.all(got[:guard] == dc.SENTINEL) and np.all(got[guard + body:] == dc.SENTINEL)
    got = got[guard:guard + body].reshape(N, case.Hs, case.Ws, 3)
    for f in range(N):
        want = dc.preproc(case.frames[f], case.Hs, case.Ws)
        assert np.array_equal(got[f], want), f'{case.name} frame {f}: {(got[f] != want).sum()} floats differ'
