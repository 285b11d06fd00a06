"""Shared by tests/test_preproc_cases_cpu.py and tests/test_gpu_preproc.py: crop_resize_kernel (syn_crop_resize, syn_crop_resize_frames)
at its edges.  The operation: the zero-padded crop of a rounded box (the meaning of synergynet_amd.inference.crop_img: a box entirely outside
the frame gives an all-zero crop) resized to 120x120 by the oracle's restatement of cv2's 8-bit INTER_LANCZOS4
(oracle.preproc_numpy.resize_lanczos4).  Integer arithmetic on both sides: every comparison is equality of bytes.

The frames are small so that boxes of ordinary sizes overhang them: up-scaling (sides below 120, where the first taps are negative and the
replicate-at-the-crop-border path meets the zero-outside-the-frame path), crops narrower than the 8 taps, non-square boxes, boxes outside
the frame, a frame strictly inside the crop, both saturations of the final clip."""
import functools
from collections import namedtuple

import numpy as np

OUT = 120
FRAME_SIZES = ((40, 56), (23, 17), (31, 64), (130, 141))        # H, W; the last one holds the 119 / 120 / 121 boxes whole
STRIPED = 4                                                     # index of the 0 / 255 striped frame (40x56)
Box = namedtuple('Box', 'name frame box')                       # box: sx, sy, ex, ey (already rounded, as syn_crop_resize takes it)


@functools.lru_cache(maxsize=None)
def frames():
    out = [np.random.default_rng(900 + i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(FRAME_SIZES)]
    h, w = FRAME_SIZES[0]
    stripes = (((np.arange(w) // 4) % 2) * 255).astype(np.uint8)
    fr = np.broadcast_to(stripes[None, :, None], (h, w, 3)).copy()
    fr[h // 2:] = 255 - fr[h // 2:]                              # and one horizontal edge
    out.append(fr)
    for f in out:
        f.setflags(write=False)
    return tuple(out)


def crop(img, box):
    """the (ey-sy) x (ex-sx) crop: the part of the box inside the frame copied, the rest zero; all zero when no part is inside"""
    h, w = img.shape[:2]
    sx, sy, ex, ey = (int(v) for v in box)
    res = np.zeros((ey - sy, ex - sx, 3), dtype=np.uint8)
    x0, x1, y0, y1 = max(sx, 0), min(ex, w), max(sy, 0), min(ey, h)
    if x1 > x0 and y1 > y0:
        res[y0 - sy:y1 - sy, x0 - sx:x1 - sx] = img[y0:y1, x0:x1]
    return res


def inside(img, box):
    """number of frame pixel columns and rows the box holds"""
    h, w = img.shape[:2]
    sx, sy, ex, ey = box
    return max(0, min(ex, w) - max(sx, 0)), max(0, min(ey, h) - max(sy, 0))


@functools.lru_cache(maxsize=None)
def _expected(frame, box):
    from oracle.preproc_numpy import resize_lanczos4
    out = resize_lanczos4(crop(frames()[frame], box), OUT, OUT)
    out.setflags(write=False)
    return out


def expected(b):
    return _expected(b.frame, tuple(b.box))


def unclipped(img, box):
    """resize_lanczos4's value in front of its final clip to 0..255 (same taps, same sums, same rounding shift)"""
    from oracle.preproc_numpy import lanczos4_taps
    src = crop(img, box).astype(np.int64)
    h, w = src.shape[:2]
    fx, wx = lanczos4_taps(OUT, w)
    fy, wy = lanczos4_taps(OUT, h)
    cols = np.clip(fx[:, None] + np.arange(8), 0, w - 1)
    rows = np.clip(fy[:, None] + np.arange(8), 0, h - 1)
    hor = np.einsum('yxkc,xk->yxc', src[:, cols, :], wx)
    ver = np.einsum('ykxc,yk->yxc', hor[rows], wy)
    return (ver + (1 << 21)) >> 22


def tables(boxes):
    """per box the tap tables syn_crop_resize takes: (xofs [B,120] int32, xcoef [B,120,8] int16, yofs, ycoef)"""
    from synergynet_amd.inference import lanczos4_tables
    xs = [lanczos4_tables(b[2] - b[0]) for b in boxes]
    ys = [lanczos4_tables(b[3] - b[1]) for b in boxes]
    return (np.stack([t[0] for t in xs]), np.stack([t[1] for t in xs]), np.stack([t[0] for t in ys]), np.stack([t[1] for t in ys]))


def _placements(f, side_w, side_h):
    """a box of side_w x side_h on frame f: inside it (or centred on it where it cannot fit), and overhanging each of its four borders"""
    h, w = FRAME_SIZES[f]
    cx, cy = (w - side_w) // 2, (h - side_h) // 2
    over_x, over_y = max(3, side_w // 3), max(3, side_h // 3)
    at = {'inside': (cx, cy), 'over left': (-over_x, cy), 'over right': (w - side_w + over_x, cy), 'over top': (cx, -over_y),
          'over bottom': (cx, h - side_h + over_y)}
    return [Box(f'{side_w}x{side_h} {k} frame {f}', f, (x, y, x + side_w, y + side_h)) for k, (x, y) in at.items()]


@functools.lru_cache(maxsize=None)
def groups():
    g = {}
    # up-scaling (37, 119), identity (120), the first down-scaling (121): whole inside the 130x141 frame and over each border; 37 also on 40x56
    g['sides'] = tuple(b for s in (37, 119, 120, 121) for b in _placements(3, s, s)) + tuple(_placements(0, 37, 37))
    # below the tap count, and non-square (independent x and y tables)
    g['narrow'] = tuple(_placements(0, 1, 1) + _placements(0, 2, 3) + _placements(0, 7, 8) + _placements(1, 7, 8))
    g['non-square'] = tuple(_placements(0, 50, 90) + _placements(0, 90, 50) + _placements(3, 50, 90) + _placements(3, 90, 50))
    h, w = FRAME_SIZES[0]
    g['outside'] = (Box('left of the frame', 0, (-37, 2, 0, 39)), Box('right of the frame', 0, (w, 2, w + 37, 39)),
                    Box('above the frame', 0, (5, -50, 42, 0)), Box('below the frame', 0, (5, h, 42, h + 37)),
                    Box('far away', 0, (-5000, 7000, -4800, 7200)), Box('off the corner', 0, (w, h, w + 9, h + 200)))
    g['one line inside'] = (Box('last column inside', 0, (w - 1, 2, w + 36, 39)), Box('first column inside', 0, (-36, 2, 1, 39)),
                            Box('last row inside', 0, (5, h - 1, 42, h + 36)), Box('first row inside', 0, (5, -36, 42, 1)),
                            Box('one pixel inside', 0, (w - 1, h - 1, w + 149, h + 149)))
    g['frame inside crop'] = (Box('23x17 frame in a 300x300 box', 1, (-100, -120, 200, 180)), Box('2047 wide over 40x56', 0, (-1000, -10, 1047, 60)),
                              Box('31x64 frame in a 121x70 box', 2, (-30, -20, 91, 50)))
    g['saturation'] = tuple(Box(f'striped {b.name}', STRIPED, b.box) for b in _placements(0, 37, 37) + _placements(0, 23, 31))
    return g


GROUP_NAMES = ('sides', 'narrow', 'non-square', 'outside', 'one line inside', 'frame inside crop', 'saturation')
BATCH_SIZES = (1, 7)                    # 14400 pixels per face: face boundaries fall inside a 256-thread block from the second face on


def batches(boxes, size):
    """consecutive batches of `size` boxes of ONE frame (syn_crop_resize takes one frame per call); the last one may be shorter"""
    out = []
    for f in sorted({b.frame for b in boxes}):
        bs = [b for b in boxes if b.frame == f]
        out += [bs[i:i + size] for i in range(0, len(bs), size)]
    return out


# ------------------------------------------------------------------------------------------------ syn_crop_resize_frames
BlockCase = namedtuple('BlockCase', 'block frame_off frame_dim face_frame faces')


@functools.lru_cache(maxsize=None)
def block_case():
    """frames 0, 1, 2 in one byte block: starts that are no multiples of 4, a gap between two of them; frame 1 has no face; the faces of frames 2
    and 0 interleaved; the same boxes on both frames."""
    fr = frames()[:3]
    sizes = [f.size for f in fr]
    off = [1, 1 + sizes[0], 1 + sizes[0] + sizes[1] + 13]                 # frame 1 right behind frame 0 (odd start), 13 unused bytes, frame 2
    block = np.full(off[2] + sizes[2] + 5, 0xAA, dtype=np.uint8)
    for o, f in zip(off, fr):
        block[o:o + f.size] = f.reshape(-1)
    shared = [(-6, -4, 31, 33), (10, 5, 30, 22), (20, 12, 141, 133), (16, 30, 53, 67), (-3, 3, 4, 11)]     # each on frame 2 AND on frame 0
    own0 = [(-10, -10, 70, 50), (39, 20, 76, 57)]
    own2 = [(60, -5, 97, 32), (0, 0, 64, 31)]
    f2 = [Box(f'block {b} frame 2', 2, b) for b in shared + own2]
    f0 = [Box(f'block {b} frame 0', 0, b) for b in shared + own0]
    faces = []
    for a, b in zip(f2, f0):                                               # 2, 0, 2, 0, ...
        faces += [a, b]
    faces[4], faces[5] = faces[5], faces[4]                                # 2, 0, 2, 0, 0, 2, 2, 0, ...: not a plain alternation either
    return BlockCase(block, np.array(off, dtype=np.int64), np.array([f.shape[:2] for f in fr], dtype=np.int32),
                     np.array([b.frame for b in faces], dtype=np.int32), tuple(faces))
