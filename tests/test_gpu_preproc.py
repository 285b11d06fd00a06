"""GPU tests of crop_resize_kernel at its edges (run with `-m gpu`) through syn_crop_resize and syn_crop_resize_frames: up-scaling, identity
and down-scaling boxes inside a frame and over each of its borders, crops narrower than the 8 taps, non-square boxes, boxes outside the
frame, frames inside the crop, both saturations of the final clip, batches of 1 and of 7 faces, and faces of several frames of one byte
block in interleaved order.  Yardstick: tests/preproc_cases.py (premises asserted by tests/test_preproc_cases_cpu.py); equality of bytes.
The crops are written into a 0x5A-filled buffer with a guard on both sides, which must keep its bytes.

On an MI355X every case passed on the kernel as it was.  With the replicate-at-the-crop-border clamp of the column taps taken out of
crop_resize_kernel (a variant library), sides, narrow, non-square, outside, one line inside and saturation fail at both batch sizes, and so
does the several-frames test; `frame inside crop` does not see that clamp (what lies past those crops' borders is zero either way)."""
import ctypes as C

import numpy as np
import pytest

import preproc_cases as pc
from synergynet_amd import abi

pytestmark = pytest.mark.gpu
FACE = pc.OUT * pc.OUT * 3
GUARD = 4096


@pytest.fixture(scope='module')
def handle():
    """any handle serves: the kernel needs no weights"""
    from synergynet_amd import synth
    from synergynet_amd.faceboxes import FaceBoxes
    return FaceBoxes(state_dict=synth.make_faceboxes_state())


def _upload_tables(boxes):
    import torch
    bx = torch.from_numpy(np.array(boxes, dtype=np.int32).reshape(-1, 4)).cuda()
    return [bx] + [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in pc.tables(boxes)]


def _guarded(B):
    import torch
    return torch.full((GUARD + B * FACE + GUARD,), 0x5A, dtype=torch.uint8, device='cuda')


def _crops(flat, B):
    got = flat.cpu().numpy()
    assert np.all(got[:GUARD] == 0x5A) and np.all(got[GUARD + B * FACE:] == 0x5A), 'bytes outside the output were written'
    return got[GUARD:GUARD + B * FACE].reshape(B, pc.OUT, pc.OUT, 3)


def crop_resize(handle, frame, boxes):
    """syn_crop_resize of `boxes` (sx, sy, ex, ey) on one frame -> uint8 [B,120,120,3]"""
    import torch
    fr = torch.from_numpy(np.array(frame, dtype=np.uint8, order='C')).cuda()          # (a copy: the case frames are read-only)
    bx, xo, xc, yo, yc = _upload_tables(boxes)
    B = len(boxes)
    flat = _guarded(B)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().syn_crop_resize(handle._h, fr.data_ptr(), fr.shape[0], fr.shape[1], bx.data_ptr(), xo.data_ptr(), xc.data_ptr(),
                                        yo.data_ptr(), yc.data_ptr(), flat[GUARD:].data_ptr(), B, stream))
    torch.cuda.synchronize()
    return _crops(flat, B)


@pytest.mark.parametrize('size', pc.BATCH_SIZES)
@pytest.mark.parametrize('group', pc.GROUP_NAMES)
def test_crop_resize_matches_the_oracle_at_its_edges(handle, group, size):
    frames = pc.frames()
    for batch in pc.batches(pc.groups()[group], size):
        got = crop_resize(handle, frames[batch[0].frame], [b.box for b in batch])
        for b, g in zip(batch, got):
            want = pc.expected(b)
            assert np.array_equal(g, want), f'{b.name} (batch of {len(batch)}): {(g != want).sum()} bytes differ'


def test_crop_resize_frames_reads_every_face_from_its_own_frame(handle):
    """three frames at odd byte offsets in one block with a gap, one of them without a face, faces of the other two interleaved, the same boxes
    on both: per face the oracle's crop, and the crop syn_crop_resize gives for that face on its own frame"""
    import torch
    blk = pc.block_case()
    faces = blk.faces
    B = len(faces)
    block = torch.from_numpy(blk.block).cuda()
    foff, fdim, fidx = (torch.from_numpy(a).cuda() for a in (blk.frame_off, blk.frame_dim, blk.face_frame))
    bx, xo, xc, yo, yc = _upload_tables([b.box for b in faces])
    flat = _guarded(B)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().syn_crop_resize_frames(handle._h, block.data_ptr(), foff.data_ptr(), fdim.data_ptr(), fidx.data_ptr(), bx.data_ptr(),
                                               xo.data_ptr(), xc.data_ptr(), yo.data_ptr(), yc.data_ptr(), flat[GUARD:].data_ptr(), B, stream))
    torch.cuda.synchronize()
    got = _crops(flat, B)
    frames = pc.frames()
    for i, b in enumerate(faces):
        want = pc.expected(b)
        assert np.array_equal(got[i], want), f'face {i} ({b.name}): {(got[i] != want).sum()} bytes differ from the oracle'
        alone = crop_resize(handle, frames[b.frame], [b.box])[0]
        assert np.array_equal(got[i], alone), f'face {i} ({b.name}) differs from syn_crop_resize on its own frame'
