"""The premises of tests/preproc_cases.py, asserted on the CPU: every box is where its name says it is against its frame, the crop written
there is the product's crop_img (and the oracle's wherever the oracle's is defined), both saturations of the final clip are reached, and
the block of syn_crop_resize_frames is laid out as described.  tests/test_gpu_preproc.py holds crop_resize_kernel to the same cases."""
import numpy as np

import preproc_cases as pc


def all_boxes():
    return [b for g in pc.GROUP_NAMES for b in pc.groups()[g]]


def test_boxes_are_where_their_names_say():
    g = pc.groups()
    assert set(g) == set(pc.GROUP_NAMES)
    names = [b.name for b in all_boxes()]
    assert len(set(names)) == len(names)
    fr = pc.frames()
    assert [f.shape[:2] for f in fr[:4]] == [(40, 56), (23, 17), (31, 64), (130, 141)]
    for b in all_boxes():
        assert b.box[2] > b.box[0] and b.box[3] > b.box[1], b.name
    # sides: 37, 119, 120 and 121, each whole inside a frame and over each single border
    for s in (37, 119, 120, 121):
        seen = set()
        for b in g['sides']:
            sx, sy, ex, ey = b.box
            if (ex - sx, ey - sy) != (s, s):
                continue
            h, w = fr[b.frame].shape[:2]
            over = (sx < 0, ex > w, sy < 0, ey > h)
            assert sum(over) <= 1, b.name
            seen.add(over)
            assert ('inside' in b.name) == (sum(over) == 0), b.name
        assert len(seen) == 5, s
    # up-scaling: the first taps are negative (replicated at the crop border), also where the crop's border lies outside the frame (zeros)
    xo = pc.tables([(0, 0, 37, 37)])[0]
    assert xo.min() < 0 and xo.max() + 7 > 36
    sizes = {(b.box[2] - b.box[0], b.box[3] - b.box[1]) for b in g['narrow']}
    assert sizes == {(1, 1), (2, 3), (7, 8)} and all(max(s) <= 8 for s in sizes)
    assert {(b.box[2] - b.box[0], b.box[3] - b.box[1]) for b in g['non-square']} == {(50, 90), (90, 50)}
    for b in g['outside']:
        assert 0 in pc.inside(fr[b.frame], b.box), b.name
        assert not pc.expected(b).any(), b.name                                         # all zeros
    h, w = fr[0].shape[:2]
    sides_out = {(b.box[2] <= 0, b.box[0] >= w, b.box[3] <= 0, b.box[1] >= h) for b in g['outside']}
    assert {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)} <= sides_out
    ins = [pc.inside(fr[b.frame], b.box) for b in g['one line inside']]
    assert ins[0][0] == 1 and ins[1][0] == 1 and ins[0][1] > 1 and ins[2][1] == 1 and ins[3][1] == 1 and ins[2][0] > 1 and ins[4] == (1, 1)
    for b in g['one line inside']:
        assert pc.expected(b).any(), b.name
    a, wide, c = g['frame inside crop']
    assert a.frame == 1 and (a.box[2] - a.box[0], a.box[3] - a.box[1]) == (300, 300)
    for b in (a, c):
        hh, ww = fr[b.frame].shape[:2]
        assert b.box[0] < 0 and b.box[1] < 0 and b.box[2] > ww and b.box[3] > hh        # strictly inside
    assert wide.frame == 0 and wide.box[2] - wide.box[0] == 2047
    assert pc.BATCH_SIZES == (1, 7) and (pc.OUT * pc.OUT) % 256 != 0


def test_the_crop_is_the_products_and_the_oracles():
    from oracle import preproc_numpy as opn
    from synergynet_amd.inference import crop_img
    fr = pc.frames()
    for b in all_boxes() + list(pc.block_case().faces):
        want = crop_img(fr[b.frame], [float(v) for v in b.box])
        got = pc.crop(fr[b.frame], b.box)
        assert np.array_equal(got, want), b.name
        if all(pc.inside(fr[b.frame], b.box)):                                           # the oracle's has no guard for a box outside the frame
            assert np.array_equal(got, opn.crop_img(fr[b.frame], [float(v) for v in b.box])), b.name
    # the tables the device gets are the oracle's taps (both restate cv2; tests/test_oracle_golden.py holds that for every side up to 400)
    for side in (1, 2, 3, 7, 8, 37, 119, 120, 121, 300, 2047):
        xo, xc = pc.tables([(0, 0, side, 1)])[:2]
        first, fixed = opn.lanczos4_taps(pc.OUT, side)
        assert np.array_equal(xo[0], first) and np.array_equal(xc[0], fixed), side


def test_both_saturations_are_reached():
    fr = pc.frames()[pc.STRIPED]
    assert set(np.unique(fr)) == {0, 255}
    below = above = 0
    for b in pc.groups()['saturation']:
        v = pc.unclipped(fr, b.box)
        assert np.array_equal(np.clip(v, 0, 255).astype(np.uint8), pc.expected(b)), b.name
        below += int((v < 0).sum())
        above += int((v > 255).sum())
    assert below > 100 and above > 100, (below, above)


def test_block_layout():
    blk = pc.block_case()
    fr = pc.frames()
    assert all(int(o) % 4 for o in blk.frame_off)
    ends = [int(o) + fr[i].size for i, o in enumerate(blk.frame_off)]
    assert blk.frame_off[1] == ends[0] and blk.frame_off[2] > ends[1] and ends[2] < blk.block.size        # adjacent; a gap; slack behind
    for i, o in enumerate(blk.frame_off):
        assert np.array_equal(blk.block[o:o + fr[i].size].reshape(fr[i].shape), fr[i])
        assert tuple(blk.frame_dim[i]) == fr[i].shape[:2]
    ff = blk.face_frame.tolist()
    assert ff[:6] == [2, 0, 2, 0, 0, 2] and 1 not in ff and set(ff) == {0, 2}                             # interleaved; frame 1 has no face
    assert ff == [b.frame for b in blk.faces]
    on0, on2 = {b.box for b in blk.faces if b.frame == 0}, {b.box for b in blk.faces if b.frame == 2}
    assert len(on0 & on2) >= 5 and on0 - on2 and on2 - on0                                                # the same box on two frames
    for box in on0 & on2:
        a, b = (pc._expected(f, box) for f in (0, 2))
        assert not np.array_equal(a, b)                                                                   # reading the wrong frame would show
