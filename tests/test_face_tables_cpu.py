"""CPU: the arithmetic of the device path from detections to crop tables (synergynet_amd/csrc/face_tables.h, the header the kernels
of face_tables.hip compile) built for the host (tests/face_tables_harness.cpp) against the host functions it replaces --
inference.lanczos4_tables and SynergyNet._face_tables on float32 detections -- integer for integer and bit for bit.  This pins
the rounding points and the order of operations (double source position rounded to float32, float32 1.2f margin, ties to even,
contraction off) without a GPU; the device's own sin / cos are the business of tests/test_gpu_face_tables.py.  Also: the three
new symbols are declared, listed and exported."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import face_table_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('syn_lanczos4_tables', 'syn_face_tables', 'syn_compact_detections')


def test_the_three_symbols_are_declared_listed_and_exported():
    from synergynet_amd import abi
    from synergynet_amd.build import LIB, SOURCES
    header = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    for s in SYMBOLS:
        assert re.search(r'^int %s\(syn_handle \*h,' % s, header, re.M), s
        assert s in abi.EXPORTED_SYMBOLS
    assert 'face_tables.hip' in SOURCES
    import torch  # noqa: F401  (the library binds to the HIP runtime torch loads, as in synergynet_amd/abi.py)
    lib = ctypes.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    lib.syn_abi_version.restype = ctypes.c_int
    assert lib.syn_abi_version() == 1


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp('face_tables')
    exe = str(d / 'harness')
    src = os.path.join(ROOT, 'tests', 'face_tables_harness.cpp')
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if os.path.isfile(hipcc):
        cmd = [hipcc, '-x', 'c++']                       # clang in host mode: the contraction pragma of the header is honoured
    elif shutil.which('clang++'):
        cmd = ['clang++']
    else:
        cmd = ['g++', '-ffp-contract=off', '-Wno-unknown-pragmas']
    subprocess.run(cmd + ['-O2', '-std=c++17', '-o', exe, src], check=True)

    def run(mode, arr):
        src_f, out_f = str(d / f'{mode}.in'), str(d / f'{mode}.out')
        arr.tofile(src_f)
        subprocess.run([exe, mode, src_f, str(arr.shape[0]), out_f], check=True, timeout=120)
        return np.fromfile(out_f, dtype=np.uint8)
    return run


def _tables(harness, sides):
    n = len(sides)
    raw = harness('sides', np.ascontiguousarray(sides, dtype=np.int32))
    assert raw.size == n * 120 * 4 + n * 120 * 8 * 2
    return raw[:n * 480].view(np.int32).reshape(n, 120), raw[n * 480:].view(np.int16).reshape(n, 120, 8)


def _boxes(harness, dets):
    n = dets.shape[0]
    raw = harness('boxes', np.ascontiguousarray(dets, dtype=np.float32))
    assert raw.size == n * (20 + 16 + 8 + 4)
    at = np.cumsum([0, n * 20, n * 16, n * 8, n * 4])
    return (raw[at[0]:at[1]].view(np.float32).reshape(n, 5), raw[at[1]:at[2]].view(np.int32).reshape(n, 4),
            raw[at[2]:at[3]].view(np.int32).reshape(n, 2), raw[at[3]:at[4]].view(np.int32))


def test_tap_tables_of_every_side_equal_the_host_function(harness):
    sides = np.concatenate([cases.ALL_SIDES, cases.LARGE_SIDES, cases.REPEATED_SIDES, cases.SINGLE_SIDE])
    ofs, coef = _tables(harness, sides)
    want_o, want_c = cases.host_tables(sides)
    bad = np.nonzero((ofs != want_o).any(1) | (coef != want_c).any((1, 2)))[0]
    assert bad.size == 0, f'sides that differ: {sides[bad][:10]}'


def test_handmade_detections_equal_face_tables(harness):
    dets, bad = cases.handmade_detections()
    want = cases.host_face_tables(dets)
    assert np.array_equal(want['bad'], bad), 'the case list and the host path disagree on which rows are degenerate'
    roi, box, wh, status = _boxes(harness, dets)
    assert np.array_equal(status != 0, bad)
    assert np.array_equal(box, want['box'])
    good = ~bad
    assert np.array_equal(roi[good].view(np.uint32), want['roi'][good].view(np.uint32))
    assert np.array_equal(wh[good, 0], box[good, 2] - box[good, 0]) and np.array_equal(wh[good, 1], box[good, 3] - box[good, 1])
    assert np.all(wh[bad] == 1)
    ofs_x, coef_x = _tables(harness, wh[:, 0])
    ofs_y, coef_y = _tables(harness, wh[:, 1])
    assert np.array_equal(np.stack([ofs_x, ofs_y]), want['ofs']) and np.array_equal(np.stack([coef_x, coef_y]), want['coef'])


def test_the_margin_heights_need_the_float32_constant(harness):
    roi, box, wh, status = _boxes(harness, cases.margin_rows())
    assert not status.any()
    hc = np.array(cases.MARGIN_HEIGHTS, dtype=np.float32) / np.float32(2)
    m = np.array(cases.MARGINS_F32, dtype=np.float32)
    assert np.array_equal(roi[:, 1], hc - m) and np.array_equal(roi[:, 3], hc + m)
    assert not np.array_equal(box[:, 1], np.rint(hc - (m - 1)).astype(np.int32))          # (a margin one less would show in the box)
    # ... and the case list is what it claims: double arithmetic gives one less
    assert [int(np.floor(float(np.float32(h)) * 1.2 / 2)) for h in cases.MARGIN_HEIGHTS] == [m - 1 for m in cases.MARGINS_F32]


def test_rounding_ties_go_to_even(harness):
    roi, box, wh, status = _boxes(harness, cases.tie_rows())
    assert not status.any()
    assert roi[:, 0].tolist() == [-8.5, -7.5] and box[:, 0].tolist() == [-8, -8]
    assert roi[:, 2].tolist() == [39.5, 40.5] and box[:, 2].tolist() == [40, 40]


def test_random_detections_equal_face_tables(harness):
    dets = cases.random_detections()
    want = cases.host_face_tables_batch(dets)
    roi, box, wh, status = _boxes(harness, dets)
    assert not status.any()
    assert np.array_equal(roi.view(np.uint32), want['roi'].view(np.uint32)) and np.array_equal(box, want['box'])
    assert np.array_equal(wh[:, 0], box[:, 2] - box[:, 0]) and np.array_equal(wh[:, 1], box[:, 3] - box[:, 1])


def test_compaction_cases_say_what_they_claim():
    """The expected values of the GPU test: poison past the counts is not counted, NaN and a score equal to the threshold are out."""
    for name, rows, counts, order in cases.compaction_cases():
        packed, face_frame, frame_faces = cases.host_compaction(rows, counts, order)
        assert frame_faces[-1] == packed.shape[0] == face_frame.shape[0] == frame_faces[:-1].sum(), name
        assert not np.isnan(packed[:, 4]).any() and (packed[:, 4] > cases.THRES).all(), name
    _, rows, counts, _ = cases.compaction_cases()[1]
    assert cases.host_compaction(rows, counts, None)[2].tolist() == [0, 2, 3, 1, 0, 6]
