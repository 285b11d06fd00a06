"""GPU box: FaceBoxes detector timings.

    python tools/bench_detector.py
        latency per frame (syn_detect: preprocessing, 33 convolutions, pools, decode, sort, NMS) next to the torch-CPU oracle
    python tools/bench_detector.py --batch [--mode batch|loop] [--input device|host] [--sizes 300x420,720x1080] [--n 1,4,16] [--reps 20]
        frames per second of a list of N frames: `batch` = one FaceBoxes.detect_batch(frames) (syn_detect_batch), `loop` =
        [detect_all(f) for f in frames] (syn_detect per frame); warm-up, then the median of --reps repetitions, one line per (size, N).
        A/B against another build on one box: SYNERGY_HIP_LIB=<that library> with --mode loop (a library from before
        syn_detect_batch is accepted in that mode only), alternating with --mode batch on the in-tree library."""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import abi, synth

ap = argparse.ArgumentParser()
ap.add_argument('--batch', action='store_true')
ap.add_argument('--mode', choices=('batch', 'loop'), default='batch')
ap.add_argument('--input', choices=('device', 'host'), default='device')
ap.add_argument('--sizes', default='300x420,720x1080')
ap.add_argument('--n', default='1,4,16')
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--tag', default='')
args = ap.parse_args()
if args.batch and args.mode == 'loop' and 'SYNERGY_HIP_LIB' in os.environ:
    # the per-frame leg of an A/B may load a build that predates the batched entry, which this mode never calls
    import ctypes
    if not hasattr(ctypes.CDLL(os.environ['SYNERGY_HIP_LIB']), 'syn_detect_batch'):
        abi._SIGS.pop('syn_detect_batch')
from synergynet_amd.faceboxes import FaceBoxes
sd = synth.make_faceboxes_state()
det = FaceBoxes(state_dict=sd)

if not args.batch:
    from oracle import faceboxes_torch as ofb  # CPU-baseline leg only (same role as bench.py's cpu_baseline): timed beside, never inside, the GPU path
    for hw in ((300, 420), (720, 1080), (1080, 1920)):
        frame = synth.make_frame(*hw, seed=1)
        ft = torch.from_numpy(frame).cuda()
        for _ in range(3): det.detect_all(ft)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n = 20
        for _ in range(n): d = det.detect_all(ft)
        torch.cuda.synchronize(); gpu = (time.perf_counter() - t0) / n
        t0 = time.perf_counter(); w = ofb.detect(sd, frame, return_all=True); cpu = time.perf_counter() - t0
        print(f'{hw[0]}x{hw[1]}: GPU {gpu*1e3:6.2f} ms/frame ({1/gpu:6.0f} fps, {d.shape[0]} dets)   torch-CPU oracle {cpu*1e3:7.1f} ms ({torch.get_num_threads()} threads)')
    sys.exit(0)

for size in args.sizes.split(','):
    h, w = (int(v) for v in size.split('x'))
    for n in (int(v) for v in args.n.split(',')):
        frames = [synth.make_frame(h, w, seed=1 + i) for i in range(n)]
        if args.input == 'device':
            frames = [torch.from_numpy(f).cuda() for f in frames]
        run = (lambda: det.detect_batch(frames)) if args.mode == 'batch' else (lambda: [det.detect_all(f) for f in frames])
        for _ in range(args.warmup): out = run()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        print(f'{args.tag or args.mode:10s} {args.input:6s} {h}x{w} N={n:<3d} median {med*1e3:8.3f} ms/call  {n/med:8.0f} frames/s  '
              f'(min {min(ts)*1e3:.3f} max {max(ts)*1e3:.3f} ms, {args.reps} reps, {sum(o.shape[0] for o in out)} dets)', flush=True)
