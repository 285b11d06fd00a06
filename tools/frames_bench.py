"""Frames in, faces out, detector inside: get_all_outputs_batch(frames) -- detections through the host: call_batch, _face_tables, a second
staging of the frames -- against get_all_outputs_frames(frames) -- detections kept on the device -- ALTERNATELY in one process after a
warm-up, so that both see the same box, clocks and allocator state.  Synthetic weights for model and detector; 16 frames of 720x1080 and
16 of 300x420, with the mesh and without.  One JSON object on stdout: faces found, wall ms per call (median of 10 each) and the split of
a call into host work and waiting for the device (SynergyNet.last_timing)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from synergynet_amd import synth  # noqa: E402
from synergynet_amd.faceboxes import FaceBoxes  # noqa: E402
from synergynet_amd.synergy3DMM import SynergyNet  # noqa: E402

WARMUP, REPEAT = 3, 10


def main():
    det = FaceBoxes(state_dict=synth.make_faceboxes_state())
    model = SynergyNet(device='cuda:0', pack=synth.make_3dmm(), backbone_state=synth.make_backbone_state(), face_detector=det)
    paths = (('batch', model.get_all_outputs_batch), ('frames', model.get_all_outputs_frames))
    out = {}
    for h, w in ((720, 1080), (300, 420)):
        frames = [synth.make_frame(h, w, seed=40 + i) for i in range(16)]
        for dense in (True, False):
            ts = {k: [] for k, _ in paths}
            split = {k: [] for k, _ in paths}
            faces = {}
            for it in range(WARMUP + REPEAT):
                for k, fn in paths:                      # alternately: batch, frames, batch, frames, ...
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = fn(frames, dense=dense)
                    t = time.perf_counter() - t0
                    faces[k] = sum(len(r[0]) for r in res)
                    del res
                    if it >= WARMUP:
                        ts[k].append(t)
                        lt = model.last_timing
                        split[k].append((lt['host_s'], lt['device_wait_s']))
            assert faces['batch'] == faces['frames']
            row = dict(faces=faces['batch'])
            for k, _ in paths:
                row[k] = dict(ms_per_call=round(float(np.median(ts[k])) * 1e3, 4), min_ms=round(min(ts[k]) * 1e3, 4),
                              host_ms=round(float(np.median([s[0] for s in split[k]])) * 1e3, 4),
                              device_wait_ms=round(float(np.median([s[1] for s in split[k]])) * 1e3, 4))
            out[f'16_frames_{h}x{w}_{"dense" if dense else "lmk_pose_only"}'] = row
    out['what'] = ('16 uint8 frames -> FaceBoxes -> crop / Lanczos resize -> MobileNetV2 -> 68 landmarks, pose (dense: + 53215-vertex mesh) per '
                   'face -> page-locked host arrays; batch = get_all_outputs_batch (detections through the host), frames = '
                   'get_all_outputs_frames (detections stay on the device); alternating calls in one process, median of 10 after 3 warm-up '
                   'rounds.  batch.host_ms includes its whole detector call, the wait for the detection rows too (last_timing starts the '
                   'clock before it and counts only the final wait as device_wait); frames.device_wait_ms is both of its waits')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
