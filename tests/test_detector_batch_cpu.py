"""CPU-side tests of the batched detector (no GPU): the two host helpers of synergynet_amd/faceboxes.py -- frames grouped by size with
their positions, detection rows and counts split into the per-frame lists FaceBoxes.__call__ returns -- and header / ctypes table /
library agreeing on syn_detect_batch."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_grouping_by_size_keeps_input_positions():
    from synergynet_amd.faceboxes import group_by_size
    shapes = [(300, 420), (240, 320), (300, 420), (33, 47), (240, 320)]
    groups = group_by_size([s + (3,) for s in shapes])
    assert [g[0] for g in groups] == [(300, 420), (240, 320), (33, 47)]               # order of first appearance
    assert [g[1] for g in groups] == [[0, 2], [1, 4], [3]]                            # stable within a group
    assert sorted(i for _, pos in groups for i in pos) == list(range(5))
    for hw, pos in groups:
        assert all(shapes[i] == hw for i in pos)
    assert group_by_size([]) == []
    assert group_by_size([(7, 9)] * 3) == [((7, 9), [0, 1, 2])]


def test_rows_and_counts_split_into_call_shaped_lists():
    from synergynet_amd.faceboxes import split_detections, vis_thres
    assert vis_thres == 0.5
    rows = np.zeros((3, 4, 5), dtype=np.float32)
    rows[..., :4] = np.arange(48, dtype=np.float32).reshape(3, 4, 4)
    rows[0, :, 4] = [0.9, 0.4, 0.99, 0.99]            # rows 2, 3 lie beyond the count: stale, must not appear
    rows[1, :, 4] = [0.99, 0.99, 0.99, 0.99]          # count 0: nothing
    rows[2, :, 4] = [0.95, 0.75, 0.5, 0.51]           # 0.5 itself is not > 0.5
    out = split_detections(rows, [2, 0, 4])
    assert isinstance(out, list) and [len(o) for o in out] == [1, 0, 3]
    assert out[0] == [[0.0, 1.0, 2.0, 3.0, np.float32(0.9)]]
    assert out[1] == []
    assert out[2] == [list(rows[2, 0]), list(rows[2, 1]), list(rows[2, 3])]
    assert all(isinstance(b, list) and len(b) == 5 for o in out for b in o)
    # the same expression __call__ applies to one frame's rows
    for i, c in enumerate([2, 0, 4]):
        assert out[i] == [[b[0], b[1], b[2], b[3], b[4]] for b in rows[i, :c] if b[4] > 0.5]
    assert [len(o) for o in split_detections(rows, np.array([4, 4, 4]), thres=0.0)] == [4, 4, 4]
    with pytest.raises(ValueError):
        split_detections(rows, [1, 2])
    with pytest.raises(ValueError):
        split_detections(rows[0], [1])


def test_new_symbol_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import build_library
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    s = 'syn_detect_batch'
    assert s in abi.EXPORTED_SYMBOLS and hasattr(l, s)
    decl = re.search(r'\bint ' + s + r'\(([^;]*)\);', hdr)
    assert decl
    assert len(decl.group(1).split(',')) == len(abi._SIGS[s][1]) == 15
    assert 'int *n_dets' in decl.group(1) and 'int N' in decl.group(1)
    for macro in ('SYN_DETECT_BATCH_MAX_FRAMES', 'SYN_DETECT_BATCH_MAX_SCRATCH_BYTES'):
        assert re.search(r'#define ' + macro + r'\b', hdr), macro
    assert int(re.search(r'#define SYN_DETECT_BATCH_MAX_FRAMES (\d+)', hdr).group(1)) == abi.SYN_DETECT_BATCH_MAX_FRAMES
    l.syn_abi_version.restype = ctypes.c_int
    assert l.syn_abi_version() == 1
    from synergynet_amd.faceboxes import FaceBoxes
    assert callable(FaceBoxes.detect_batch) and callable(FaceBoxes.call_batch)
