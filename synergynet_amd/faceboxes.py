"""FaceBoxes face detector on the GPU behind the reference's class surface.

    from FaceBoxes import FaceBoxes            # root shim -> this module
    face_boxes = FaceBoxes()                   # loads FaceBoxes/weights/FaceBoxesProd.pth like the reference (FaceBoxes.py:29,50)
    rects = face_boxes(img_bgr_uint8)          # [[xmin, ymin, xmax, ymax, score], ...] with score > 0.5 (FaceBoxes.py:60-143)

Everything from the uint8 frame to the NMS result runs in HIP kernels (csrc/detector_kernels.hip) through `syn_detect`; the
host only computes the down-scaling factor and applies the visualisation threshold, as the reference does in Python.

Not in the reference: a list of frames in one call.  `detect_batch(frames)` / `call_batch(frames)` group the frames by size, upload
each group with one copy and run it through `syn_detect_batch` (the same kernels with a frame index), with one synchronisation
for the whole call, or none with `to_host=False`; per frame the rows are bit for bit those of `detect_all` / `__call__`.
`detect_faces(frames)` is `call_batch` whose result stays on the device: the rows above vis_thres packed in frame order
(`syn_compact_detections`), for `SynergyNet.get_all_outputs_frames`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import abi, synth

confidence_threshold, top_k, keep_top_k, nms_threshold, vis_thres = 0.05, 5000, 750, 0.3, 0.5     # FaceBoxes.py:18-22
scale_flag, HEIGHT, WIDTH = True, 720, 1080                                                        # FaceBoxes.py:25-26


def flatten_detector(sd) -> np.ndarray:
    """state_dict (numpy arrays or tensors, optional 'module.' prefixes as load_model strips them, utils/functions.py:21-25)
    -> the flat float32 vector syn_load_detector takes (order documented in include/synergy_hip.h)."""
    sd = {(k.split('module.', 1)[-1] if k.startswith('module.') else k): v for k, v in sd.items()}
    get = lambda k: np.asarray(sd[k].detach().cpu().numpy() if isinstance(sd[k], torch.Tensor) else sd[k], dtype=np.float32).reshape(-1)
    parts = []
    for name, cin, cout, k, _, _, kind in synth.faceboxes_convs():
        if kind == 'head':
            parts += [get(name + '.weight'), get(name + '.bias')]
        else:
            parts += [get(name + '.conv.weight'), get(name + '.bn.weight'), get(name + '.bn.bias'), get(name + '.bn.running_mean'),
                      get(name + '.bn.running_var')]
    flat = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)
    return flat


def group_by_size(shapes):
    """shapes: per frame (H, W[, ...]).  -> [((H, W), [positions]), ...]: one entry per distinct size in order of first
    appearance, the positions of its frames in input order; all positions together are range(len(shapes))."""
    groups = {}
    for i, sh in enumerate(shapes):
        groups.setdefault((int(sh[0]), int(sh[1])), []).append(i)
    return list(groups.items())


def split_detections(rows, counts, thres=vis_thres):
    """rows [N,K,5] (x1, y1, x2, y2, score), counts [N] valid rows per frame -> per frame the list FaceBoxes.__call__ returns:
    [[x1, y1, x2, y2, score], ...] of the valid rows with score > thres (FaceBoxes.py:131-141)."""
    rows, counts = np.asarray(rows), np.asarray(counts)
    if rows.ndim != 3 or rows.shape[2] != 5 or counts.shape != rows.shape[:1]:
        raise ValueError('rows must be [N,K,5] and counts [N]')
    return [[[b[0], b[1], b[2], b[3], b[4]] for b in rows[i, :int(counts[i])] if b[4] > thres] for i in range(rows.shape[0])]


class FaceBoxes:
    """reference FaceBoxes/FaceBoxes.py:46-143."""

    def __init__(self, timer_flag=False, state_dict=None, weights_path=None, device='cuda:0'):
        if not torch.cuda.is_available():
            raise RuntimeError('FaceBoxes needs an MI355X GPU (there is no CPU path)')
        self.device = torch.device(device)
        self.timer_flag = timer_flag
        self._lib = abi.lib()
        self._h = C.c_void_p()
        abi.check(self._lib.syn_create(self.device.index or 0, C.byref(self._h)))
        if state_dict is None:
            path = weights_path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'FaceBoxes', 'weights',
                                                'FaceBoxesProd.pth')
            if not os.path.isfile(path):
                # the reference prints this and exits the interpreter (utils/functions.py:30-32); raising is kinder to callers
                raise RuntimeError(f'The pre-trained FaceBoxes model {path} does not exist')
            ck = torch.load(path, map_location='cpu')
            state_dict = ck['state_dict'] if 'state_dict' in ck else ck
        flat = flatten_detector(state_dict)
        if flat.size != self._lib.syn_detector_flat_count():
            raise RuntimeError(f'FaceBoxes state_dict has {flat.size} values, expected {self._lib.syn_detector_flat_count()}')
        abi.check(self._lib.syn_load_detector(self._h, flat.ctypes.data_as(C.c_void_p), flat.size))
        self._dets = torch.empty((keep_top_k, 5), dtype=torch.float32, device=self.device)

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                self._lib.syn_destroy(self._h)
        except Exception:
            pass

    @staticmethod
    def frame_scale(h, w):
        """FaceBoxes.py:63-70."""
        scale = 1
        if scale_flag:
            if h > HEIGHT:
                scale = HEIGHT / h
            if w * scale > WIDTH:
                scale *= WIDTH / (w * scale)
        return scale

    @staticmethod
    def scaled_size(h, w, scale):
        """FaceBoxes.py:71-75: the network input size, int() of a python-double product exactly like the reference (a float32
        product differs by one pixel on ~8 % of frame sizes, which would move the resize taps and the prior grid)."""
        if scale == 1:
            return h, w
        return int(scale * h), int(scale * w)

    def detect_all(self, img_):
        """Rows before the vis_thres filter: float32 [n,5] (x1, y1, x2, y2, score), score-descending.  img_: uint8 [H,W,3] BGR,
        numpy array or device tensor."""
        frame = img_ if isinstance(img_, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img_))
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise ValueError('frame must be uint8 [H,W,3] (BGR)')
        frame = frame.to(self.device).contiguous()
        h, w = int(frame.shape[0]), int(frame.shape[1])
        scale = self.frame_scale(h, w)
        h_s, w_s = self.scaled_size(h, w, scale)
        n = C.c_int(0)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            abi.check(self._lib.syn_detect(self._h, frame.data_ptr(), h, w, h_s, w_s, float(scale), confidence_threshold, nms_threshold,
                                           top_k, keep_top_k, self._dets.data_ptr(), C.byref(n), stream))
        return self._dets[:n.value].cpu().numpy()

    def __call__(self, img_):
        dets = self.detect_all(img_)
        return [[b[0], b[1], b[2], b[3], b[4]] for b in dets if b[4] > vis_thres]      # FaceBoxes.py:131-141

    def _adjacent_block(self, frames, pos, h, w):
        """The frames `pos` as ONE [m,h,w,3] view without a copy, when they are contiguous uint8 tensors on this device that lie back to
        back in one storage (views of a block staged by the caller: get_all_outputs_frames); else None."""
        fs = [frames[i] for i in pos]
        if not all(isinstance(f, torch.Tensor) and f.device == self.device and f.is_contiguous() for f in fs):
            return None
        base, step = fs[0].data_ptr(), h * w * 3
        if any(f.untyped_storage().data_ptr() != fs[0].untyped_storage().data_ptr() or f.data_ptr() != base + k * step
               for k, f in enumerate(fs)):
            return None
        return torch.as_strided(fs[0], (len(fs), h, w, 3), (step, w * 3, 3, 1))

    def _enqueue_batch(self, frames, max_frames, in_place=False):
        """-> (dets [N,keep_top_k,5] float32, counts [N] int32, row [N]): device buffers written size group after size group, and for
        input frame i its row in them; enqueued on the current stream, nothing synchronised.  in_place (detect_faces): a size group
        whose frames already lie back to back on the device is used where it lies (_adjacent_block)."""
        whole = None
        if isinstance(frames, (np.ndarray, torch.Tensor)):
            if frames.ndim != 4:
                raise ValueError('frames must be a list of uint8 [H,W,3] frames or one uint8 [N,H,W,3] block (BGR)')
            if isinstance(frames, torch.Tensor) and frames.device == self.device:
                whole = frames                                   # already one block on the device: no copy
            frames = [frames[i] for i in range(frames.shape[0])]
        frames = list(frames)
        if max_frames < 1:
            raise ValueError('max_frames must be at least 1')
        for f in frames:
            ok = (isinstance(f, torch.Tensor) and f.dtype == torch.uint8) or (isinstance(f, np.ndarray) and f.dtype == np.uint8)
            if not ok or f.ndim != 3 or f.shape[2] != 3:
                raise ValueError('frame must be uint8 [H,W,3] (BGR)')
        n = len(frames)
        dets = torch.empty((n, keep_top_k, 5), dtype=torch.float32, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device)
        groups = group_by_size([f.shape for f in frames])
        row = [0] * n
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            done = 0
            for (h, w), pos in groups:
                adjacent = self._adjacent_block(frames, pos, h, w) if in_place and whole is None else None
                if whole is not None:
                    block = whole.contiguous()
                elif adjacent is not None:
                    block = adjacent
                elif all(isinstance(frames[i], np.ndarray) or not frames[i].is_cuda for i in pos):
                    block = torch.empty((len(pos), h, w, 3), dtype=torch.uint8, pin_memory=True)      # one page-locked block, one copy
                    for k, i in enumerate(pos):
                        block[k].copy_(frames[i] if isinstance(frames[i], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames[i])))
                    block = block.to(self.device, non_blocking=True)
                elif len(pos) == 1 and isinstance(frames[pos[0]], torch.Tensor):
                    block = frames[pos[0]].to(self.device).contiguous()[None]
                else:
                    block = torch.stack([(f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))).to(self.device)
                                         for f in (frames[i] for i in pos)])
                scale = self.frame_scale(h, w)
                h_s, w_s = self.scaled_size(h, w, scale)
                for a in range(0, len(pos), max_frames):
                    m = min(max_frames, len(pos) - a)
                    abi.check(self._lib.syn_detect_batch(self._h, block[a].data_ptr(), m, h, w, h_s, w_s, float(scale), confidence_threshold,
                                                         nms_threshold, top_k, keep_top_k, dets[done + a].data_ptr(),
                                                         counts[done + a:].data_ptr(), stream))
                for k, i in enumerate(pos):
                    row[i] = done + k
                done += len(pos)
        return dets, counts, row

    def detect_batch(self, frames, to_host=True, max_frames=16):
        """detect_all for a list of frames: uint8 [H,W,3] BGR numpy arrays or tensors whose sizes may differ, or one [N,H,W,3] block.
        Frames of one size are stacked into one page-locked block, uploaded with one copy and run through syn_detect_batch in slices of
        at most `max_frames` (the scratch grows with the slice: about 25 MB per 720x1080 frame).
        to_host=True: one synchronisation for the whole call; -> per frame, in input order, float32 [n_i,5], the rows detect_all gives.
        to_host=False: nothing synchronises; -> per frame (dets [keep_top_k,5], count []) device views, valid on the current stream."""
        dets, counts, row = self._enqueue_batch(frames, max_frames)
        if not to_host:
            return [(dets[r], counts[r]) for r in row]
        rows, cnt = self._download(dets, counts)
        return [rows[r, :int(cnt[r])].copy() for r in row]

    def _download(self, dets, counts):
        rows = torch.empty(dets.shape, dtype=torch.float32, pin_memory=True)
        cnt = torch.empty(counts.shape, dtype=torch.int32, pin_memory=True)
        with torch.cuda.device(self.device):
            rows.copy_(dets, non_blocking=True)
            cnt.copy_(counts, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return rows.numpy(), cnt.numpy()

    def detect_faces(self, frames, max_frames=16):
        """call_batch whose result stays on the device: enqueues like detect_batch(to_host=False), then packs the rows with
        score > vis_thres in INPUT-frame order (syn_compact_detections; the size-group permutation goes in as its `order`).
        -> (rows [N * keep_top_k, 5] float32, face_frame [N * keep_top_k] int32, frame_faces [N + 1] int32), device tensors valid on the
        current stream, nothing synchronised: frame_faces holds the faces per frame and then their total n; rows[:n] are the faces
        frame after frame as call_batch lists them, face_frame[:n] the frame of each; what lies past n is unspecified.
        frames: as detect_batch takes them; an [m,H,W,3] block on the device, or device frames that already lie back to back, are used
        in place."""
        dets, counts, row = self._enqueue_batch(frames, max_frames, in_place=True)
        n = dets.shape[0]
        rows = torch.empty((n * keep_top_k, 5), dtype=torch.float32, device=self.device)
        face_frame = torch.empty((n * keep_top_k,), dtype=torch.int32, device=self.device)
        frame_faces = torch.empty((n + 1,), dtype=torch.int32, device=self.device)
        if n == 0:
            return rows, face_frame, frame_faces.zero_()
        with torch.cuda.device(self.device):
            order = torch.tensor(row, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
            abi.check(self._lib.syn_compact_detections(self._h, dets.data_ptr(), counts.data_ptr(), order.data_ptr(), n, keep_top_k, vis_thres,
                                                       rows.data_ptr(), face_frame.data_ptr(), frame_faces.data_ptr(),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return rows, face_frame, frame_faces

    def call_batch(self, frames):
        """__call__ for a list of frames (see detect_batch): a list, in input order, of the lists __call__ returns."""
        dets, counts, row = self._enqueue_batch(frames, 16)
        rows, cnt = self._download(dets, counts)
        return split_detections(rows[row], cnt[row])
