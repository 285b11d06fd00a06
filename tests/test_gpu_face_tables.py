"""GPU: syn_lanczos4_tables, syn_face_tables and syn_compact_detections (csrc/face_tables.hip) on the cases of
tests/face_table_cases.py against the host code they replace (inference.lanczos4_tables, SynergyNet._face_tables on float32
detections, faceboxes.split_detections).  Every comparison is integer or bit equality: the kernels restate the host arithmetic with
its rounding points (tests/test_face_tables_cpu.py pins those on the CPU), and the device's sin / cos -- the one thing the CPU
test cannot see -- are checked here over every side 1..4096.  Output buffers are pre-filled with a poison value so that an
element no lane wrote shows."""
import ctypes as C

import numpy as np
import pytest

import face_table_cases as cases

pytestmark = pytest.mark.gpu
POISON = 0x5A


@pytest.fixture(scope='module')
def model():
    from synergynet_amd.synergy3DMM import SynergyNet
    return SynergyNet(device='cuda:0', load_constants=False)


def _poisoned(shape, dtype):
    import torch
    t = torch.empty(shape, dtype=dtype, device='cuda')
    t.view(torch.uint8).fill_(POISON)
    return t


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_tables(model, sides):
    """syn_lanczos4_tables into poisoned buffers -> (ofs, coef) as numpy."""
    import torch
    from synergynet_amd import abi
    n = len(sides)
    s = torch.from_numpy(np.ascontiguousarray(sides, dtype=np.int32)).cuda()
    ofs, coef = _poisoned((n, 120), torch.int32), _poisoned((n, 120, 8), torch.int16)
    abi.check(abi.lib().syn_lanczos4_tables(model._h, s.data_ptr(), n, ofs.data_ptr(), coef.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return ofs.cpu().numpy(), coef.cpu().numpy()


def _raw_face_tables(model, dets):
    import torch
    from synergynet_amd import abi
    n = dets.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(dets, dtype=np.float32)).cuda()
    roi, box, status = _poisoned((n, 5), torch.float32), _poisoned((n, 4), torch.int32), _poisoned((n,), torch.int32)
    ofs, coef = _poisoned((2, n, 120), torch.int32), _poisoned((2, n, 120, 8), torch.int16)
    abi.check(abi.lib().syn_face_tables(model._h, d.data_ptr(), n, roi.data_ptr(), box.data_ptr(), ofs[0].data_ptr(), coef[0].data_ptr(),
                                        ofs[1].data_ptr(), coef[1].data_ptr(), status.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return dict(roi=roi.cpu().numpy(), box=box.cpu().numpy(), ofs=ofs.cpu().numpy(), coef=coef.cpu().numpy(), status=status.cpu().numpy())


def _same_tables(got, want, sides):
    ofs, coef = got
    bad = np.nonzero((ofs != want[0]).any(1) | (coef != want[1]).any((1, 2)))[0]
    assert bad.size == 0, f'{bad.size} sides differ from inference.lanczos4_tables, the first: {np.asarray(sides)[bad][:10]}'


def _same_faces(got, want):
    bad = want['bad']
    assert np.array_equal(got['status'] != 0, bad), np.nonzero((got['status'] != 0) != bad)[0][:10]
    assert np.array_equal(got['box'], want['box']), np.nonzero((got['box'] != want['box']).any(1))[0][:10]
    assert np.array_equal(got['roi'][~bad].view(np.uint32), want['roi'][~bad].view(np.uint32))
    assert np.array_equal(got['ofs'], want['ofs']) and np.array_equal(got['coef'], want['coef'])


def test_every_side_up_to_4096_in_one_call(model):
    _same_tables(_raw_tables(model, cases.ALL_SIDES), cases.host_tables(cases.ALL_SIDES), cases.ALL_SIDES)


@pytest.mark.parametrize('name', ['LARGE_SIDES', 'REPEATED_SIDES', 'SINGLE_SIDE'])
def test_large_repeated_and_single_sides(model, name):
    sides = getattr(cases, name)
    got = _raw_tables(model, sides)
    _same_tables(got, cases.host_tables(sides), sides)
    if name == 'REPEATED_SIDES':
        assert np.array_equal(got[0][0], got[0][2]) and np.array_equal(got[1][0], got[1][2])


def test_the_wrapper_returns_the_host_tables(model):
    ofs, coef = model.lanczos4_tables_device(cases.REPEATED_SIDES)
    assert ofs.is_cuda and coef.is_cuda and tuple(ofs.shape) == (3, 120) and tuple(coef.shape) == (3, 120, 8)
    _same_tables((ofs.cpu().numpy(), coef.cpu().numpy()), cases.host_tables(cases.REPEATED_SIDES), cases.REPEATED_SIDES)


def test_twenty_thousand_random_detections(model):
    dets = cases.random_detections()
    _same_faces(_raw_face_tables(model, dets), cases.host_face_tables_batch(dets))


def test_handmade_detections_and_degenerate_rows_among_good_ones(model):
    dets, bad = cases.handmade_detections()
    want = cases.host_face_tables(dets)
    assert np.array_equal(want['bad'], bad) and bad.sum() == len(cases.degenerate_rows())
    got = _raw_face_tables(model, dets)
    _same_faces(got, want)
    assert np.array_equal(got['roi'][:, 4], dets[:, 4])                     # the score passes through, degenerate or not


@pytest.mark.parametrize('n', [1, 7, 65])
def test_batch_sizes(model, n):
    import torch
    dets = np.concatenate([cases.handmade_detections()[0], cases.random_detections(64, seed=3)])[:n]
    want = cases.host_face_tables(dets)
    _same_faces(_raw_face_tables(model, dets), want)
    roi, box, ofs, coef, status = model.face_tables(torch.from_numpy(dets).cuda())          # the wrapper: device in, device out
    assert all(t.is_cuda for t in (roi, box, ofs, coef, status))
    _same_faces(dict(roi=roi.cpu().numpy(), box=box.cpu().numpy(), ofs=ofs.cpu().numpy(), coef=coef.cpu().numpy(),
                     status=status.cpu().numpy()), want)


def _raw_compact(det_handle, rows, counts, order, thres=cases.THRES):
    import torch
    from synergynet_amd import abi
    N, K = rows.shape[:2]
    d, c = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    o = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).cuda() if order is not None else None
    out, ff, nf = _poisoned((N * K, 5), torch.float32), _poisoned((N * K,), torch.int32), _poisoned((N + 1,), torch.int32)
    abi.check(abi.lib().syn_compact_detections(det_handle, d.data_ptr(), c.data_ptr(), o.data_ptr() if o is not None else None, N, K,
                                               thres, out.data_ptr(), ff.data_ptr(), nf.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), ff.cpu().numpy(), nf.cpu().numpy()


@pytest.mark.parametrize('case', cases.compaction_cases(), ids=lambda c: c[0])
def test_compaction_equals_split_detections(model, case):
    _, rows, counts, order = case
    want_rows, want_ff, want_nf = cases.host_compaction(rows, counts, order)
    out, ff, nf = _raw_compact(model._h, rows, counts, order)
    assert np.array_equal(nf, want_nf)
    total = int(want_nf[-1])
    assert np.array_equal(out[:total].view(np.uint32), want_rows.view(np.uint32)) and np.array_equal(ff[:total], want_ff)
    assert np.all(out[total:].view(np.uint8) == POISON) and np.all(ff[total:].view(np.uint8) == POISON)      # nothing written past the total


def test_refusals_leave_the_handle_usable(model):
    import torch
    from synergynet_amd import abi
    lib, h, st = abi.lib(), model._h, _stream()
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device='cuda')
    i16 = lambda *shape: torch.zeros(shape, dtype=torch.int16, device='cuda')
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device='cuda')
    sides, ofs, coef = torch.tensor([5, 0, 7], dtype=torch.int32, device='cuda'), i32(3, 120), i16(3, 120, 8)
    ofs.fill_(-7)
    assert lib.syn_lanczos4_tables(h, sides.data_ptr(), 3, ofs.data_ptr(), coef.data_ptr(), st) == abi.SYN_ERR_INVALID       # side 0
    assert b'sides[1]=0' in lib.syn_last_error()
    torch.cuda.synchronize()
    assert bool((ofs == -7).all())                                                                                            # nothing ran
    assert lib.syn_lanczos4_tables(h, sides.data_ptr(), -1, ofs.data_ptr(), coef.data_ptr(), st) == abi.SYN_ERR_INVALID
    assert lib.syn_lanczos4_tables(h, None, 3, ofs.data_ptr(), coef.data_ptr(), st) == abi.SYN_ERR_INVALID
    assert lib.syn_lanczos4_tables(h, sides.data_ptr(), 3, None, coef.data_ptr(), st) == abi.SYN_ERR_INVALID
    assert lib.syn_lanczos4_tables(None, sides.data_ptr(), 3, ofs.data_ptr(), coef.data_ptr(), st) == abi.SYN_ERR_INVALID
    assert lib.syn_lanczos4_tables(h, sides.data_ptr(), 0, None, None, st) == 0                                               # n = 0: nothing to do
    d, roi, box, status = f32(2, 5), f32(2, 5), i32(2, 4), i32(2)
    o2, c2 = i32(2, 2, 120), i16(2, 2, 120, 8)
    args = [d.data_ptr(), 2, roi.data_ptr(), box.data_ptr(), o2[0].data_ptr(), c2[0].data_ptr(), o2[1].data_ptr(), c2[1].data_ptr(), status.data_ptr()]
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        a = list(args)
        a[k] = None
        assert lib.syn_face_tables(h, *a, st) == abi.SYN_ERR_INVALID, k
    assert lib.syn_face_tables(h, *(args[:1] + [-1] + args[2:]), st) == abi.SYN_ERR_INVALID
    assert lib.syn_face_tables(h, *(args[:1] + [0] + args[2:]), st) == 0
    rows, counts, out, ff, nf = f32(2, 4, 5), i32(2), f32(8, 5), i32(8), i32(3)
    cargs = [rows.data_ptr(), counts.data_ptr(), None, 2, 4, 0.5, out.data_ptr(), ff.data_ptr(), nf.data_ptr()]
    for k in (0, 1, 6, 7, 8):
        a = list(cargs)
        a[k] = None
        assert lib.syn_compact_detections(h, *a, st) == abi.SYN_ERR_INVALID, k
    for k, v in ((3, -1), (4, 0), (4, -3)):
        a = list(cargs)
        a[k] = v
        assert lib.syn_compact_detections(h, *a, st) == abi.SYN_ERR_INVALID, (k, v)
    assert lib.syn_compact_detections(h, *(cargs[:3] + [0] + cargs[4:]), st) == 0
    # ... and good calls follow on the same handle
    _same_tables(_raw_tables(model, cases.SINGLE_SIDE), cases.host_tables(cases.SINGLE_SIDE), cases.SINGLE_SIDE)
    dets = cases.GOOD
    _same_faces(_raw_face_tables(model, dets), cases.host_face_tables(dets))
    with pytest.raises(abi.SynergyHipError, match='sides'):
        model.lanczos4_tables_device([4, -2])
