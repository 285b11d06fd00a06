#!/usr/bin/env python3
"""Throughput bench of the SynergyNet inference hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W
      N = 1: runs in this process.  N > 1 without a torchrun environment: spawns N ranks of itself (one process per GPU,
      RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set here, rendezvous on 127.0.0.1) and relays rank 0's JSON line.
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (the driver's N > 1 launch)

One "step" = one pass of the hot path over one batch of synthetic crops per GPU:
uint8 crops [B,120,120,3] already resident in HBM -> MobileNetV2 -> 62 params ->
68 landmarks + 53215-vertex mesh (+ pose), all on device (BASELINE.json configs[2],
the configuration the metric "faces/sec (68-lmk + 53215-vert)" is quoted on; B = 1024
faces per GPU, i.e. configs[3]'s 8192 faces over 8 GPUs).  Weak scaling: every rank
processes its own shard of B faces; the only collective is the one-time RCCL broadcast
of the packed constants from rank 0 (outside the timed region).

`--lmk-only` times BASELINE configs[1] instead (B = 128 by default, 68 landmarks + pose, no mesh).

Prints ONE JSON line (rank 0) with the contract fields.  A plain run does only what that line needs: set-up, warm-up, the
timed steps.  `--full` adds `roofline`, `cpu_baseline` and `extra` (the other BASELINE configs and the reference-API variants
of the headline step, each timed briefly on the same box: configs[1] B = 128 landmarks only, fp32 NCHW ingest through
forward_test, the reference's packed [B,3,53215] output, one stream, ResNet-50 B = 512 = configs[4]).

`--dump-outputs DIR` writes what the last timed step returned (params, landmarks, pose, a fixed sample of the mesh) as
DIR/<name>.npy, so that two builds can be compared output for output on the same seeded inputs.
"""
import argparse
import ctypes
import json
import os
import platform
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from synergynet_amd import synth                      # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak
PEAK_F16_MFMA_TFLOPS = 2500.0     # dense fp16 / bf16 MFMA peak; the two-piece fp16 operand split issues 3 fp16 MFMAs per fp32 block product
PEAK_F16X2_TFLOPS = PEAK_F16_MFMA_TFLOPS / 3.0      # ceiling of fp32-equivalent work on that pipe
PEAK_HBM_GBS = 8000.0


# ------------------------------------------------------------------------------------------------ CPU baseline (checker leg)
def _cpu_info():
    model, phys = platform.processor() or 'unknown', None
    try:
        txt = open('/proc/cpuinfo').read()
        for line in txt.splitlines():
            if line.startswith('model name'):
                model = line.split(':', 1)[1].strip()
                break
        cores = set()
        pid = cid = None
        for line in txt.splitlines() + ['']:
            if line.startswith('physical id'):
                pid = line.split(':')[1].strip()
            elif line.startswith('core id'):
                cid = line.split(':')[1].strip()
            elif not line.strip():
                if pid is not None and cid is not None:
                    cores.add((pid, cid))
                pid = cid = None
        phys = len(cores) or None
    except OSError:
        pass
    return model, phys


def cpu_baseline(sd, pack, budget_s=26.0):
    """BASELINE.md section 2 on this box's host cores, on a bounded sample.

    kind "reference": /root/reference is importable (authoring container) -> the reference's OWN module is the timed code
    (oracle/ref_loader.py imports it from where it lies).  kind "port": the GPU box has no /root/reference -> the oracle's
    restatement of the same torch-CPU / numpy calls (oracle/backbone_torch.py, oracle/recon_numpy.py).
    Two variants: (i) the loop body of get_all_outputs per face (B = 1 forward_test + numpy sparse / dense vertices + pose,
    synergy3DMM.py:194-201) and (ii) best-case batched (forward_test(B = 128) + reconstruct_vertex_62 sparse and dense): BASELINE.md
    section 2's B = 1 and B = 128 (B = 1024 does not fit the time slice of a default bench run).
    Protocol: fp32, no_grad, eval; per thread count 2 warm-up iterations, then the median of >= 10 timed iterations
    (fewer only if the time slice runs out -- the count is reported); thread counts tried: all physical cores (BASELINE.md's
    protocol) and 32 / 16 / 8 (small convolutions do not scale to 128 threads); `value` = the best batched rate."""
    from oracle import backbone_torch, recon_numpy, ref_loader
    logical = os.cpu_count() or 1
    model_name, phys = _cpu_info()
    phys = phys or logical
    b = recon_numpy.Basis(pack)
    Bc = 128
    x = torch.from_numpy(synth.normalize_crops(synth.make_crops(Bc, seed=1)))
    roi = [0.0, 0.0, 120.0, 120.0, 1.0]
    kind = 'port'
    if ref_loader.available():
        try:
            _, ref_model = ref_loader.build_reference_model(pack, sd)
            inf = ref_loader._REF_MODULES['utils.inference']
            kind = 'reference'
        except Exception as e:                      # pragma: no cover - container quirks must not kill the bench line
            print('cpu_baseline: reference import failed, timing the port:', e, file=sys.stderr)

    if kind == 'reference':
        def batched():
            with torch.no_grad():
                p = ref_model.forward_test(x)
                ref_model.reconstruct_vertex_62(p, dense=False)
                ref_model.reconstruct_vertex_62(p, dense=True)

        def per_face(i):
            with torch.no_grad():
                p = ref_model.forward_test(x[i:i + 1]).numpy()[0]
            inf.predict_sparseVert(p, roi, transform=True)
            inf.predict_denseVert(p, roi, transform=True)
            inf.predict_pose(p, roi)
    else:
        def batched():
            p, _ = backbone_torch.mobilenet_v2_forward(sd, x.numpy())
            recon_numpy.reconstruct_vertex_62(b, p.numpy(), dense=False)
            recon_numpy.reconstruct_vertex_62(b, p.numpy(), dense=True)

        def per_face(i):
            p, _ = backbone_torch.mobilenet_v2_forward(sd, x[i:i + 1].numpy())
            p = p.numpy()[0]
            recon_numpy.predict_vertices(b, p, roi, dense=False)
            recon_numpy.predict_vertices(b, p, roi, dense=True)
            recon_numpy.predict_pose(b, p, roi)

    cands = sorted({t for t in (8, 16, 32, phys) if t <= logical})
    slice_s = budget_s / (2 * len(cands))

    def timed(fn, unit_faces):
        fn(); fn()
        ts, t_end = [], time.perf_counter() + slice_s
        while len(ts) < 10 or (len(ts) < 15 and time.perf_counter() < t_end):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
            if time.perf_counter() > t_end and len(ts) >= 3:
                break
        return unit_faces / float(np.median(ts)), len(ts)

    rows = []
    for t in cands:
        torch.set_num_threads(t)
        r2, n2 = timed(batched, Bc)
        k = [0]

        def one():
            per_face(k[0] % Bc)
            k[0] += 1
        r1, n1 = timed(one, 1)
        rows.append(dict(threads=t, batched_faces_s=round(r2, 2), batched_iters=n2, per_face_faces_s=round(r1, 2), per_face_iters=n1))
    best = max(rows, key=lambda r: r['batched_faces_s'])
    best1 = max(rows, key=lambda r: r['per_face_faces_s'])
    allc = next(r for r in rows if r['threads'] == max(cands))
    return dict(value=best['batched_faces_s'], unit='faces/s', cores=best['threads'], kind=kind,
                sample=f'median of {best["batched_iters"]} iterations of forward_test(B={Bc}) + reconstruct_vertex_62 (68 landmarks and '
                       f'53215 vertices), fp32, on {best["threads"]} torch threads of {phys} physical / {logical} logical cores '
                       f'({"the reference module itself" if kind == "reference" else "oracle restatement of the reference calls"}); '
                       f'per-face loop and the other thread counts in `variants`',
                cpu_model=model_name, physical_cores=phys, logical_cores=logical, torch=torch.__version__, numpy=np.__version__,
                protocol='2 warm-up + median of >= 10 timed iterations per variant and thread count (BASELINE.md section 2)',
                per_face_loop=dict(value=best1['per_face_faces_s'], threads=best1['threads'],
                                   what='B=1 forward_test + predict_sparseVert + predict_denseVert + predict_pose per face '
                                        '(synergy3DMM.py:194-201)'),
                all_physical_cores=dict(threads=allc['threads'], batched_faces_s=allc['batched_faces_s'],
                                        per_face_faces_s=allc['per_face_faces_s']),
                variants=rows)


# ------------------------------------------------------------------------------------------------ multi-process launch
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n, poll_s=0.05, grace_s=5.0):
    """`python bench.py --gpus N` outside torchrun: one child process per GPU, same argv; rank 0 inherits stdout (its ONE
    JSON line is this command's output), every rank inherits stderr.  The children are POLLED: the first rank that exits non-zero
    takes the others down (SIGTERM, SIGKILL after `grace_s`) -- a dead rank must not leave its peers waiting in
    init_process_group / the RCCL broadcast until the collective timeout.  Host threads: one OpenMP / MKL thread per rank unless the
    caller says otherwise (8 ranks must not each start a 256-thread pool)."""
    port = os.environ.get('MASTER_PORT') or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        env.setdefault('OMP_NUM_THREADS', '1')
        env.setdefault('MKL_NUM_THREADS', '1')
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    while any(p.poll() is None for p in procs):
        failed = [(r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
        if failed:
            rc = failed[0][1]
            print(f'bench.py: rank {failed[0][0]} exited with status {rc}; stopping the other ranks', file=sys.stderr)
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            t_end = time.monotonic() + grace_s
            while time.monotonic() < t_end and any(p.poll() is None for p in procs):
                time.sleep(poll_s)
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(poll_s)
    for p in procs:
        p.wait()
        rc = rc or p.returncode
    return rc


def _cpulist(txt):
    out = []
    for part in txt.strip().split(','):
        if '-' in part:
            lo, hi = part.split('-')
            out.extend(range(int(lo), int(hi) + 1))
        elif part:
            out.append(int(part))
    return out


def bind_rank_to_numa(local, local_world, pci_bdf=None):
    """Pin this rank's host threads to the NUMA node of its GPU (sysfs: /sys/bus/pci/devices/<bdf>/numa_node), or -- when the node
    is unknown (no GPU in a dry run, numa_node = -1) -- to its 1/local_world share of the CPUs this process may use.  Best effort:
    returns what it did for the `distributed` block, never raises."""
    info = dict(numa_node=None, cpus=None)
    try:
        allowed = sorted(os.sched_getaffinity(0))
        cpus = None
        if pci_bdf:
            try:
                node = int(open(f'/sys/bus/pci/devices/{pci_bdf.lower()}/numa_node').read())
                if node >= 0:
                    want = set(_cpulist(open(f'/sys/devices/system/node/node{node}/cpulist').read()))
                    cpus = [c for c in allowed if c in want]
                    info['numa_node'] = node
            except OSError:
                pass
        if not cpus and local_world > 1:
            per = max(1, len(allowed) // local_world)
            cpus = allowed[local * per:(local + 1) * per] or allowed
        if cpus:
            os.sched_setaffinity(0, cpus)
            info['cpus'] = len(cpus)
    except (AttributeError, OSError):
        pass
    return info


def _gpu_bdf(local):
    try:
        p = torch.cuda.get_device_properties(local)
        return '%04x:%02x:%02x.0' % (getattr(p, 'pci_domain_id', 0), p.pci_bus_id, p.pci_device_id)
    except Exception:
        return None


def dry_run(args):
    """`--dry-run`: the multi-process plumbing of the bench WITHOUT GPUs (CPU tests drive it with world 2 and 8 through spawn_ranks):
    rank start-up hygiene, gloo rendezvous on 127.0.0.1, the constants broadcast protocol on the REAL packed blob (device-free packer
    on rank 0, the library's acceptance checks on the receivers), face shards, barrier-bracketed timing with the MAX over ranks, the
    per-rank report, the ONE JSON line.  The "step" is a sleep: no throughput claim is made (`dry_run: true`)."""
    import torch.distributed as dist
    from synergynet_amd.dist import broadcast_constants, check_constants_host, pack_constants_host, shard_range
    rank, world, local = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('LOCAL_RANK', '0'))
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'
    if os.environ.get('SYN_BENCH_FAIL_RANK') == str(rank):          # test hook: a rank that dies before the rendezvous
        time.sleep(float(os.environ.get('SYN_BENCH_FAIL_AFTER', '0.2')))
        sys.exit(3)
    torch.set_num_threads(1)
    numa = bind_rank_to_numa(local, int(os.environ.get('LOCAL_WORLD_SIZE', world)))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', str(_free_port()))
    dist.init_process_group('gloo', rank=rank, world_size=world)

    class HostReplica:                                               # the export / import protocol of SynergyNet on host memory
        device = torch.device('cpu')
        blob = None

        def export_constants(self):
            return self.blob

        def import_constants(self, buf):
            self.header = check_constants_host(buf.numpy())          # syn_check_constants_host + the Python header parser
            self.blob = buf
    m = HostReplica()
    if rank == 0:
        m.blob = torch.from_numpy(pack_constants_host(pack=synth.make_3dmm(n_vert=2048), backbone_state=synth.make_backbone_state()))
    t0 = time.perf_counter()
    nbytes = broadcast_constants(m, src=0)
    B = args.batch or 1024
    lo, hi = shard_range(B * world, rank, world)                     # contiguous face shards (weak scaling: B per rank)
    assert hi - lo == B
    info = dict(backend=dist.get_backend(), world=world, constants_bytes=nbytes, broadcast_s=round(time.perf_counter() - t0, 4))

    def step():
        time.sleep(0.0005)
    for _ in range(args.warmup):
        step()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    el_own = time.perf_counter() - t0
    dist.barrier()
    el = time.perf_counter() - t0
    t = torch.tensor([el], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t.item())
    info.update(per_rank_report(dist, rank, world, B * args.steps / el_own, numa, torch.device('cpu')))
    if rank == 0:
        out = dict(metric='faces/sec (dry run: no GPU work)', value=round(B * world * args.steps / el, 1), unit='faces/s', n_gpus=world,
                   steps=args.steps, warmup=args.warmup, ms_per_step=round(el / args.steps * 1e3, 4), higher_is_better=True,
                   scaling='weak', vs_baseline=None, dtype='none', data='synthetic', dry_run=True,
                   config=dict(workload='multi-process plumbing only (gloo, host memory)', faces_per_gpu_per_step=B, global_batch=B * world),
                   distributed=info)
        sys.stdout.write(json.dumps(out) + '\n')
        sys.stdout.flush()
    dist.barrier()
    dist.destroy_process_group()
    return 0


def per_rank_report(dist, rank, world, own_rate, numa, dev):
    """faces/s of every rank over its own timed loop (all_gather) + min / max + the host placement of each rank."""
    mine = torch.tensor([own_rate, float(numa.get('numa_node') if numa.get('numa_node') is not None else -1), float(numa.get('cpus') or 0),
                         float(torch.get_num_threads())], dtype=torch.float64, device=dev)
    allr = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allr, mine)
    rows = [[float(v) for v in t.cpu()] for t in allr]
    rates = [r[0] for r in rows]
    return dict(per_rank_faces_s=[round(r, 1) for r in rates], min_rank_faces_s=round(min(rates), 1), max_rank_faces_s=round(max(rates), 1),
                rank_numa_node=[int(r[1]) for r in rows], rank_cpus=[int(r[2]) for r in rows], rank_host_threads=[int(r[3]) for r in rows])


# ------------------------------------------------------------------------------------------------ timing helpers
def _recon_rocprof():
    """(average ms of syn::recon_f16_kernel<4, true, ...> in the newest committed one-stream kernel-stats bundle, its path) -- a second,
    dispatch-free measurement of the kernel extra.reconstruction_alone.kernel times with HIP events."""
    import csv
    for rnd in ('r5', 'r4', 'r3'):
        fp = os.path.join(ROOT, 'profiles', rnd, 'kernel_stats_b1024_one_stream.csv')
        if os.path.isfile(fp):
            try:
                for row in csv.DictReader(open(fp)):
                    if 'recon_f16_kernel<4, true' in row['Name']:
                        return round(float(row['AverageNs']) * 1e-6, 4), 'profiles/%s/kernel_stats_b1024_one_stream.csv' % rnd
            except Exception:
                pass
    return None, None


RECON_ROCPROF = _recon_rocprof()


def dump_outputs(out_dir, param, lmk, mesh, pose):
    """`--dump-outputs`: what a caller of the timed step receives -- params [B,62], landmarks [B,3,68], pose angles and translation
    [B,3] and the mesh [B,3,53215] -- as float32 .npy files.  The mesh is a fixed sample, every face at 2048 seeded vertex indices
    (25 MB at B = 1024); above 1024 faces every array keeps 1024 seeded faces, so that the files stay under 64 MB at any batch."""
    os.makedirs(out_dir, exist_ok=True)
    B = param.shape[0]
    faces = torch.from_numpy(np.sort(np.random.default_rng(1).choice(B, 1024, replace=False))) if B > 1024 else None
    arrays = dict(param=param, lmk=lmk, pose_angles=pose[0], pose_t3d=pose[1])
    if mesh is not None:
        verts = np.sort(np.random.default_rng(0).choice(mesh.shape[2], min(2048, mesh.shape[2]), replace=False))
        arrays['mesh_sample'] = mesh[:, :, torch.from_numpy(verts).to(mesh.device)]
    for name, t in arrays.items():
        if faces is not None:
            t = t.index_select(0, faces.to(t.device))
        np.save(os.path.join(out_dir, name + '.npy'), t.detach().float().cpu().numpy())


def time_steps(fn, steps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    # defaults: 0.35 s of timed work after 35 ms of warm-up -- a 20-step / 40 ms window reads ~5 % low (clocks still ramping)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=None, help='faces per GPU per step (default 1024; 128 with --lmk-only; 512 with --arch resnet50)')
    ap.add_argument('--lmk-only', action='store_true', help='BASELINE configs[1]: 68 landmarks + pose only, no 53215-vertex mesh')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-extras', action='store_true', help='skip the `extra` measurements (other configs / API variants)')
    ap.add_argument('--overlap', type=int, default=None, help='2 (default): two replicas (handle + stream each) take the batches alternately; 1: one handle, reconstruction of batch i on a second stream beside the backbone of batch i+1; 0: one stream')
    ap.add_argument('--rec-priority', type=int, default=-1, help='HIP priority of the reconstruction stream (-1 high = default, 0 normal)')
    ap.add_argument('--arch', default='mobilenet_v2', choices=['mobilenet_v2', 'resnet50'],
                    help='resnet50 = BASELINE configs[4]; the default bench line is mobilenet_v2')
    ap.add_argument('--prewarm', type=float, default=0.3, help='seconds of untimed steps BEFORE the W warm-up steps: the clocks of an idle GPU ramp for '
                    '~0.2 s, and a 20-step / 24 ms window taken right after W = 5 steps reads ~5 %% low (reported as `prewarm_s`)')
    ap.add_argument('--dry-run', action='store_true', help='multi-process plumbing only (gloo on host memory, no GPU): what the CPU tests drive')
    ap.add_argument('--full', action='store_true', help='also measure the roofline, the sustained clocks, the `extra` configs and the CPU '
                    'baseline (--no-extras / --no-cpu-baseline still drop theirs); a plain run times the headline step only')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='write the outputs of the last timed step to DIR/<name>.npy (float32)')
    args = ap.parse_args()
    if args.overlap is None:
        args.overlap = 2

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    if args.dry_run:
        sys.exit(dry_run(args))

    # native libraries (RCCL, HIP) print banners on fd 1: keep the real stdout for the ONE JSON line only
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'
    assert torch.cuda.is_available(), 'bench.py needs MI355X GPUs'
    assert local < torch.cuda.device_count(), f'rank {rank}: LOCAL_RANK {local} but only {torch.cuda.device_count()} GPUs are visible'
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    numa = dict(numa_node=None, cpus=None)
    if world > 1:                # one process per GPU: a few host threads each, next to the GPU's memory controller
        torch.set_num_threads(1)
        numa = bind_rank_to_numa(local, int(os.environ.get('LOCAL_WORLD_SIZE', world)), _gpu_bdf(local))
    dist = None
    dist_info = None
    if world > 1 or os.environ.get('SYN_BENCH_FORCE_DIST') == '1':      # the env knob exercises the RCCL path with one rank
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(_free_port()))
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    from synergynet_amd.synergy3DMM import SynergyNet
    from synergynet_amd.dist import broadcast_constants
    pack = sd = None
    if rank == 0:
        pack = synth.make_3dmm()
        sd = synth.make_resnet50_state() if args.arch == 'resnet50' else synth.make_backbone_state()
        model = SynergyNet(device=dev, pack=pack, backbone_state=sd, arch=args.arch)
    else:
        model = SynergyNet(device=dev, load_constants=False, arch=args.arch)
    if dist is not None:
        t0 = time.perf_counter()
        nbytes = broadcast_constants(model, src=0)          # one RCCL broadcast over xGMI, then no collectives
        torch.cuda.synchronize()
        dist_info = dict(backend=dist.get_backend(), world=world, constants_bytes=nbytes, broadcast_s=round(time.perf_counter() - t0, 4))
        print(f'[rank {rank}] RCCL broadcast of {nbytes} constant bytes done in {dist_info["broadcast_s"]} s', file=sys.stderr)
        if os.environ.get('SYN_BENCH_FORCE_DIST') == '1' and world == 1:
            # single-rank exercise of the receive side too: a second handle that never saw host assets imports the blob
            twin = SynergyNet(device=dev, load_constants=False, arch=args.arch)
            twin.import_constants(model.export_constants())
            c8 = torch.from_numpy(synth.make_crops(8, seed=5)).to(dev)
            same = torch.equal(twin.forward_crops_u8(c8), model.forward_crops_u8(c8))
            dist_info['import_twin_bitwise_equal'] = bool(same)
            assert same, 'imported constants give different parameters'
            del twin

    B = args.batch or (128 if args.lmk_only else 512 if args.arch == 'resnet50' else 1024)
    crops = torch.from_numpy(synth.make_crops(B, seed=1000 + rank)).to(dev)      # this rank's shard
    rois = torch.from_numpy(synth.make_rois(B, seed=2000 + rank)).to(dev)
    lmk = torch.empty((B, 3, 68), dtype=torch.float32, device=dev)
    mesh = None if args.lmk_only else model.empty_vertices(B, dense=True)   # [B,3,53215] view, rows pitched to 128-byte lines

    # Two HIP streams (synergynet_amd/streams.py): the reconstruction of batch i (HBM-write bound) runs beside the backbone of
    # batch i+1 (issue bound); every step still does the whole pass, the final barrier waits for both streams.
    # The isolated-forward profile behind the roofline block (HIP events after every launch, syn_backbone_profile) is taken HERE, while
    # the process owns no stream but the default one: every further stream costs all of them (~5 % on these per-launch times with the two
    # replica streams alive), and the roofline is about the kernels, not about the schedule of batches.
    iso_profile = None
    if args.full and rank == 0 and args.arch != 'resnet50':
        from synergynet_amd import abi as _abi
        _lib = _abi.lib()
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < max(args.prewarm, 0.2):
            for _ in range(8):
                model.forward_crops_u8(crops)
            torch.cuda.synchronize()
        nmax = 64
        feat = (ctypes.c_int * nmax)()
        ms = (ctypes.c_float * nmax)()
        fl = (ctypes.c_double * nmax)()
        reps, all_ms, n = 9, [], 0
        for _ in range(reps):
            n = _lib.syn_backbone_profile(model._h, crops.data_ptr(), B, nmax, feat, ms, fl)
            assert n > 0, _lib.syn_last_error()
            all_ms.append(np.array(ms[:n], dtype=np.float64))
        # per launch: one pre-empted launch in one repetition must not move the figure
        iso_profile = (list(feat[:n]), np.median(np.stack(all_ms), axis=0), np.array(fl[:n]))

    from synergynet_amd.streams import OverlappedPipeline, ReplicaRing
    if args.overlap == 2:
        # two replicas (a handle + a HIP stream each; the second one imports the first one's packed constants on the device) take the
        # batches alternately: the whole tail of batch i runs beside batch i + 1.  Every batch still does the whole pass into buffers
        # of its own; the final barrier waits for both streams.
        twin = SynergyNet(device=dev, load_constants=False, arch=args.arch)
        twin.import_constants(model.export_constants())
        ring = ReplicaRing(models=[model, twin])
        outs = [(lmk, mesh), (torch.empty_like(lmk), None if args.lmk_only else twin.empty_vertices(B, dense=True))]
        pipe = None

        def step():
            lo, mo = outs[ring._k % 2]
            return ring.submit(crops, rois, dense=not args.lmk_only, lmk_out=lo, mesh_out=mo)[:4]
    else:
        pipe = OverlappedPipeline(model, overlap=bool(args.overlap), rec_priority=args.rec_priority)

        def step():
            return pipe.submit(crops, rois, lmk_out=lmk, mesh_out=mesh, dense=not args.lmk_only)

    t_pre, n_pre = time.perf_counter(), 0
    while time.perf_counter() - t_pre < args.prewarm:       # clock ramp of an idle GPU: untimed, before the contract's W warm-up steps
        step()
        n_pre += 1
        if n_pre % 8 == 0:
            torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    barrier()
    el = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, *last)
    sustained = None
    if args.full and rank == 0 and world == 1 and not args.no_extras:
        # sustained clocks: the same step for ~2 s, right here -- before any extra creates further HIP streams (they cost every stream)
        try:
            n2 = max(args.steps, int(2.0 / max(el / args.steps, 1e-4)))
            t1 = time.perf_counter()
            for _ in range(n2):
                step()
            torch.cuda.synchronize()
            e2 = time.perf_counter() - t1
            sustained = dict(faces_s=round(B * n2 / e2, 1), ms_per_step=round(e2 / n2 * 1e3, 4), faces_per_step=B, steps=n2)
        except Exception as e:
            sustained = dict(error=str(e)[:200])
    if dist is not None:
        el_own = el
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
        dist_info.update(per_rank_report(dist, rank, world, B * args.steps / el_own, numa, dev))

    # --- roofline of the dominant kernel family, measured live with HIP events on the launch stream:
    # syn_backbone_profile records an event after every launch of one forward (C ABI, include/synergy_hip.h)
    roof = None
    from synergynet_amd import abi
    lib = abi.lib()
    if args.full and rank == 0 and args.arch == 'resnet50':
        fl = lib.syn_resnet50_flops_per_face() * B
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(5):
            model.forward_crops_u8(crops)
        e1.record()
        torch.cuda.synchronize()
        bb_ms = e0.elapsed_time(e1) / 5
        ach = fl / (bb_ms * 1e-3) / 1e12
        roof = dict(bound='mfma', kernel='ResNet-50 backbone forward (syn::conv_lt_kernel LDS-tiled implicit GEMM in layers 2-4, syn::conv_h2s_kernel for the 64-channel convolutions, syn::conv_c3f_kernel = conv3 + next conv1 in layers 1 / 2, stem with the max-pool in its epilogue, heads); '
                                         'fp32-accurate results on v_mfma_f32_16x16x32_f16 with every operand as two fp16 pieces (3 MFMAs per '
                                         'block product); peak = dense fp16 MFMA peak 2500 TFLOP/s / 3',
                    achieved=round(ach, 3), peak=round(PEAK_F16X2_TFLOPS, 1), unit='TFLOP/s', frac=round(ach / PEAK_F16X2_TFLOPS, 4), traffic=None,
                    mfma_issue_tflops=round(3 * ach, 1), mfma_peak_fp16=PEAK_F16_MFMA_TFLOPS,
                    frac_of_fp32_mfma_peak=round(ach / PEAK_F32_MFMA_TFLOPS, 4),
                    flops_per_launch=fl, ms_per_launch=round(bb_ms, 4))
    elif args.full and rank == 0:
        feats, avg_ms, flops = iso_profile
        n = len(feats)
        fam = [i for i, f in enumerate(feats) if 2 <= f <= 17 or f >= 100]  # fused inverted-residual block launches (>= 100: a chain, 100 * first + last)
        fam_ms, fam_fl = float(avg_ms[fam].sum()), float(flops[fam].sum())
        achieved = fam_fl / (fam_ms * 1e-3) / 1e12
        # HBM bytes / MFMA-pipe occupancy come from rocprofv3 --pmc passes of THIS command taken in separate runs (tools/round_profile.sh ->
        # tools/make_profiles.py -> profiles/traffic_rN.json).  They are NOT measured by this run: counters_source says which file,
        # which commit and which box they are from, so a reader can tell a stale bundle from a fresh one.
        traffic = pipe_busy = counters_source = traffic_fwd = None
        for name in ('traffic_r6.json', 'traffic_r5.json', 'traffic_r4.json', 'traffic_r3.json', 'traffic_r2.json', 'traffic_r1.json'):
            tfp = os.path.join(ROOT, 'profiles', name)
            if os.path.isfile(tfp) and B == 1024:
                try:
                    tj = json.load(open(tfp))
                    traffic = tj.get('fused_block_bytes_per_launch')
                    pipe_busy = tj.get('fused_block_mfma_pipe_busy')
                    # the whole forward (stem + family + head), read + written, per 1024-face forward -- the figure to hold against the
                    # compulsory bytes of the path (43.2 KB of uint8 crop in, 62 parameters out per face)
                    pk_ = tj.get('per_kernel')
                    pk_ = pk_.items() if isinstance(pk_, dict) else pk_
                    fam_b = tj.get('fused_block_bytes_per_forward') or {}
                    one = [v for k_, v in pk_ if 'stem_rm_kernel' in k_ or 'head_f16x2_kernel' in k_]      # one launch per forward each
                    rd = fam_b.get('read', 0) + sum(v.get('read_bytes', 0) for v in one)
                    wr = fam_b.get('write', 0) + sum(v.get('write_bytes', 0) for v in one)
                    if rd and wr:
                        traffic_fwd = dict(read=round(rd), write=round(wr))
                    counters_source = dict(file='profiles/' + name, commit=tj.get('commit'), box=tj.get('box'), collected=tj.get('collected'),
                                           measured_by_this_run=False,
                                           fields=['roofline.traffic', 'roofline.mfma_pipe_busy'])
                    break
                except Exception:
                    pass
        ceiling = PEAK_F16X2_TFLOPS
        roof = dict(bound='mfma',
                    kernel=f'syn::fused_block_rm_kernel, syn::fused_pair_rm_kernel, syn::fused_chain_lb_kernel, syn::fused_chain_lb4_kernel (expand 1x1 -> dw 3x3 -> project 1x1 '
                           f'per block; {len(fam)} launches per forward, features.2-17 = {fam_fl / flops.sum() * 100:.1f}% of backbone FLOPs; '
                           f'features.2-6 row-marching (3 + 4 and 5 + 6 two blocks per launch), features.7-14 and 15-17 register-resident chains of blocks in one launch each (launch code '
                           f'100 * first + last), hidden activations never leave registers); fp32-accurate '
                           f'results on v_mfma_f32_{{32x32x16,16x16x32}}_f16 with every operand as two fp16 pieces (3 MFMAs per block product): '
                           f'algorithmic fp32 FLOPs priced against the dense fp16 MFMA peak / 3',
                    achieved=round(achieved, 3), peak=round(ceiling, 1), unit='TFLOP/s',
                    frac=round(achieved / ceiling, 4), traffic=traffic,
                    traffic_unit=f'HBM bytes (read + written) per LAUNCH of the family, average over its {len(fam)} launches -- the unit of '
                                 f'`achieved` (x {len(fam)} = the family per forward); the whole forward is backbone_traffic',
                    backbone_traffic=None if traffic_fwd is None else dict(
                        bytes_per_forward=traffic_fwd, faces=B,
                        algorithmic_bytes_per_forward=B * (120 * 120 * 3 + 62 * 4),
                        ratio=round((traffic_fwd['read'] + traffic_fwd['write']) / (B * (120 * 120 * 3 + 62 * 4)), 1),
                        what='stem + fused blocks + head, all launches of one 1024-face forward; algorithmic = the uint8 crops in and the '
                             '62 parameters out (SURVEY 8d); the excess is the fp32 block-boundary activations of the 60x60 / 30x30 / 15x15 stages'),
                    counters_source=counters_source,
                    # what the pipe sees: 3 fp16 MFMAs per fp32 block product; mfma_pipe_busy is the same share of the pipe from
                    # SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE (profiles/, separate PMC run).  Matrix and vector instructions of the waves of
                    # a SIMD do not overlap (tools/ubench/mfma_valu_kinds.hip), so frac = t_mfma / (t_mfma + t_valu + t_exposed).
                    mfma_issue_tflops=round(3 * achieved, 1), mfma_peak_fp16=PEAK_F16_MFMA_TFLOPS, mfma_pipe_busy=pipe_busy,
                    frac_of_fp32_mfma_peak=round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
                    flops_per_launch=round(fam_fl / len(fam)), ms_per_launch=round(fam_ms / len(fam), 5),
                    timing='per-launch median of 9 isolated forwards, HIP events after every launch on the launch stream (syn_backbone_profile)',
                    backbone=dict(ms=round(float(avg_ms.sum()), 4), launches=n,
                                  tflops=round(float(flops.sum()) / (float(avg_ms.sum()) * 1e-3) / 1e12, 3)),
                    per_launch=[dict(feature=int(f), ms=round(float(m), 4), tflops=round(float(x) / (float(m) * 1e-3) / 1e12, 2))
                                for f, m, x in zip(feats, avg_ms, flops)])

    # --- the other BASELINE configs and the reference-API variants of the headline step, briefly, on this box
    extra = None
    if args.full and rank == 0 and world == 1 and not args.no_extras and args.arch == 'mobilenet_v2' and not args.lmk_only:
        extra = {}
        sync = torch.cuda.synchronize

        def rate(Bx, fn, steps=20, warmup=3):
            ms_ = time_steps(fn, steps, warmup, sync) * 1e3
            return dict(faces_s=round(Bx / ms_ * 1e3, 1), ms_per_step=round(ms_, 4), faces_per_step=Bx, steps=steps)

        try:                                                    # an extra must never cost the headline line
            # configs[1]: B = 128, 68 landmarks (+ pose) only
            c128, r128 = crops[:128].contiguous(), rois[:128].contiguous()
            l128 = torch.empty((128, 3, 68), dtype=torch.float32, device=dev)
            p128 = OverlappedPipeline(model, overlap=True, rec_priority=args.rec_priority)
            extra['b128_lmk_only'] = dict(rate(128, lambda: p128.submit(c128, r128, lmk_out=l128, dense=False), steps=100, warmup=10),
                                          what='BASELINE configs[1]: uint8 crops -> MobileNetV2 -> 68 landmarks + pose, no mesh')
            p1 = OverlappedPipeline(model, overlap=False)
            extra['b128_lmk_only_one_stream'] = rate(128, lambda: p1.submit(c128, r128, lmk_out=l128, dense=False), steps=100, warmup=10)
            extra['b1_lmk_only_latency_ms'] = round(time_steps(lambda: p1.submit(crops[:1], rois[:1], dense=False), 200, 20, sync) * 1e3, 4)
            # the headline step through the reference's own entry points: fp32 NCHW crops into forward_test, packed [B,3,53215] output
            xf = torch.from_numpy(synth.normalize_crops(synth.make_crops(B, seed=1000))).to(dev)
            packed = torch.empty((B, 3, model._n_vert), dtype=torch.float32, device=dev)

            def ref_api_step():
                p = model.forward_test(xf)
                model.reconstruct(p, roi=rois, dense=False, out=lmk)
                model.reconstruct(p, roi=rois, dense=True, out=packed)
                model.predict_pose_batch(p, rois)
            # (50 + 20 steps: these follow the small-batch extras, and the first ~10 ms after light work run at lower clocks -- 10 + 2 steps
            # read 1.29 ms where tools/ref_api_time.py reads 1.11 on the same kind of box)
            extra['fp32_ingest_packed_output_one_stream'] = dict(rate(B, ref_api_step, steps=50, warmup=20),
                                                                 what='forward_test(fp32 [B,3,120,120]) + reconstruct into the packed [B,3,53215] layout '
                                                                      '(synergy3DMM.py:131-147), one stream: the step exactly as the reference API shapes it')
            # first-class alias: what a caller of the reference's own entry points gets, next to the headline `value` (uint8 crops, pitched rows, two replicas)
            extra['reference_api_step'] = dict(extra['fp32_ingest_packed_output_one_stream'], same_as='fp32_ingest_packed_output_one_stream')
            pk = OverlappedPipeline(model, overlap=bool(args.overlap), rec_priority=args.rec_priority)
            extra['packed_output'] = rate(B, lambda: pk.submit(crops, rois, lmk_out=lmk, mesh_out=packed), steps=50, warmup=20)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def ev_ms(fn, reps=10):
                fn(); sync(); e0.record()
                for _ in range(reps):
                    fn()
                e1.record(); sync()
                return e0.elapsed_time(e1) / reps
            pp = model.forward_crops_u8(crops)
            mesh_bytes = B * 3 * model._n_vert * 4
            t_pitch = ev_ms(lambda: model.reconstruct(pp, roi=rois, dense=True, out=mesh))
            t_pack = ev_ms(lambda: model.reconstruct(pp, roi=rois, dense=True, out=packed))
            # the kernel itself (HIP events inside the library, no prologue, no launch bubbles): the HBM-write-bound kernel of the path
            ms2 = (ctypes.c_float * 2)()
            kms = []
            for _ in range(5):
                abi.check(lib.syn_reconstruct_profile(model._h, pp.data_ptr(), B, rois.data_ptr(), mesh.data_ptr(), mesh.stride(1), 1, ms2))
                kms.append((ms2[0], ms2[1]))
            k_prep, k_main = float(np.median([k[0] for k in kms])), float(np.median([k[1] for k in kms]))
            extra['reconstruction_alone'] = dict(pitched_ms=round(t_pitch, 4), pitched_tb_s=round(mesh_bytes / t_pitch / 1e9, 3),
                                                 packed_ms=round(t_pack, 4), packed_tb_s=round(mesh_bytes / t_pack / 1e9, 3),
                                                 mesh_bytes=mesh_bytes, peak_tb_s=PEAK_HBM_GBS / 1e3,
                                                 what='pitched_ms / packed_ms: one reconstruct() call = prologue kernel + contraction kernel + the launch '
                                                      'bubbles between dependent kernels, back to back; kernel: the contraction kernel alone, event to event',
                                                 kernel=dict(bound='hbm', name='syn::recon_f16_kernel', ms=round(k_main, 4), prologue_ms=round(k_prep, 4),
                                                             timing='HIP events recorded by the library around the launch (syn_reconstruct_profile): INCLUDES the dispatch '
                                                                    'latency of the launch, i.e. an upper bound of the kernel time; the rocprofv3 kernel-trace average of the '
                                                                    'same kernel is rocprof_ms (from the committed bundle named in rocprof_source, another box / run)',
                                                             rocprof_ms=RECON_ROCPROF[0], rocprof_source=RECON_ROCPROF[1],
                                                             rocprof_tb_s=None if RECON_ROCPROF[0] is None else round(mesh_bytes / RECON_ROCPROF[0] / 1e9, 3),
                                                             achieved=round(mesh_bytes / k_main / 1e6, 1), peak=PEAK_HBM_GBS, unit='GB/s',
                                                             frac=round(mesh_bytes / k_main / 1e6 / PEAK_HBM_GBS, 4)))
            extra['fp32_ingest_backbone_ms'] = round(ev_ms(lambda: model.forward_test(xf), 5), 4)
            extra['u8_ingest_backbone_ms'] = round(ev_ms(lambda: model.forward_crops_u8(crops), 5), 4)
            del xf, packed
            if args.overlap == 2:
                two = OverlappedPipeline(model, overlap=True, rec_priority=args.rec_priority)
                extra['one_handle_two_streams'] = dict(rate(B, lambda: two.submit(crops, rois, lmk_out=lmk, mesh_out=mesh), steps=40, warmup=5),
                                                       what='rounds 1-3a headline mode: one handle, the reconstruction of batch i on a second stream beside the backbone of batch i+1')
            if args.overlap:
                one = OverlappedPipeline(model, overlap=False)
                extra['one_stream'] = rate(B, lambda: one.submit(crops, rois, lmk_out=lmk, mesh_out=mesh), steps=50, warmup=10)
        except Exception as e:
            extra['error'] = 'extras stopped at: ' + str(e)[:300]
            torch.cuda.synchronize()
        # a measured floor under arbitrary checkpoints: the headline runs the fp16x2 kernels because the synthetic weights pass
        # the load-time range proof; a checkpoint that fails it runs the exact fp32-MFMA kernels block by block (reference behaviour being
        # replaced: any checkpoint loads and answers, synergy3DMM.py:109-113,156-164).  Same step, one stream, B faces.
        try:
            one = OverlappedPipeline(model, overlap=False)
            prev = lib.syn_set_schedule(model._h, 1)
            try:
                extra['exact_schedule'] = dict(rate(B, lambda: one.submit(crops, rois, lmk_out=lmk, mesh_out=mesh), steps=20, warmup=5),
                                               what='syn_set_schedule(h, 1): EVERY block (and stem, head, reconstruction prologue) on the exact fp32-MFMA / fp32 kernels -- '
                                                    'the schedule check_numerics() compares the default one against', numerics_fallback_blocks='all (forced)')
            finally:
                lib.syn_set_schedule(model._h, prev)
            madv = SynergyNet(device=dev, pack=pack, backbone_state=synth.make_unprovable_backbone_state())
            n_fb, _ = madv.numerics_report()
            padv = OverlappedPipeline(madv, overlap=False)
            extra['all_blocks_fallback'] = dict(rate(B, lambda: padv.submit(crops, rois, lmk_out=lmk, mesh_out=mesh), steps=20, warmup=5),
                                                numerics_fallback_blocks=int(n_fb),
                                                what='an adversarial checkpoint (synth.make_unprovable_backbone_state: every block\'s expand rows spread over 8 decades) '
                                                     'whose blocks the load-time range proof rejects: default schedule, each rejected block on its exact kernel')
            del madv, padv
        except Exception as e:
            extra['exact_schedule_error'] = str(e)[:300]
            torch.cuda.synchronize()
        # the documented entry point (reference synergy3DMM.py:167-207): frames + detections in, numpy landmarks / meshes / poses out,
        # through get_all_outputs (1 frame) and get_all_outputs_batch (16 frames); detections are given (the detector is timed in
        # tools/bench_detector.py), the frame upload, crop + resize, forward, reconstruction and the DOWNLOAD of every mesh are inside
        try:
            # in a process of its own: what a caller's process sees (here the two replica streams, the reconstruction stream and the
            # other extras' leftovers would sit beside the call's download stream, and every stream costs all of them)
            q = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'gao_bench.py')],
                               capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get('HIP_VISIBLE_DEVICES', str(local))))
            extra['get_all_outputs'] = json.loads(q.stdout.strip().splitlines()[-1])
        except Exception as e:                                  # an extra must never cost the headline line
            extra['get_all_outputs'] = dict(error=str(e)[:200])
        # configs[4]: ResNet-50 B = 512 + full mesh
        try:
            rmodel = SynergyNet(device=dev, pack=pack, backbone_state=synth.make_resnet50_state(), arch='resnet50')
            Br = 512
            rc, rr = crops[:Br].contiguous(), rois[:Br].contiguous()
            rl, rm = torch.empty((Br, 3, 68), dtype=torch.float32, device=dev), rmodel.empty_vertices(Br, dense=True)
            rp = OverlappedPipeline(rmodel, overlap=bool(args.overlap), rec_priority=args.rec_priority)
            r = rate(Br, lambda: rp.submit(rc, rr, lmk_out=rl, mesh_out=rm), steps=20, warmup=3)
            bb = ev_ms(lambda: rmodel.forward_crops_u8(rc), 3)
            fl = lib.syn_resnet50_flops_per_face() * Br
            r.update(backbone_ms=round(bb, 4), backbone_tflops=round(fl / (bb * 1e-3) / 1e12, 2),
                     frac_of_fp32_mfma_peak=round(fl / (bb * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                     what='BASELINE configs[4]: ResNet-50 120x120 B=512 -> 62 params -> 68 landmarks + 53215-vertex mesh + pose')
            r['mode'] = 'in this process (one handle + reconstruction stream, beside the streams the other extras left behind)'
            del rmodel, rm
            try:
                # the same workload as a bench line of its own, in a fresh process: the default schedule (two replicas) and no other streams
                q = subprocess.run([sys.executable, os.path.abspath(__file__), '--arch', 'resnet50', '--steps', '40', '--warmup', '5', '--no-extras', '--no-cpu-baseline'],
                                   capture_output=True, text=True, timeout=240, env=dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get('HIP_VISIBLE_DEVICES', str(local))))
                ql = json.loads(q.stdout.strip().splitlines()[-1])
                r['in_process'] = dict(faces_s=r['faces_s'], ms_per_step=r['ms_per_step'], mode=r.pop('mode'))
                r.update(faces_s=ql['value'], ms_per_step=ql['ms_per_step'], steps=ql['steps'], mode='own process, default schedule: ' + ql['config']['streams'][:60])
            except Exception as e:
                r['own_process_error'] = str(e)[:200]
            extra['resnet50_b512'] = r
        except Exception as e:                                  # an extra must never cost the headline line
            extra['resnet50_b512'] = dict(error=str(e)[:200])
        # configs[1] with several batches in flight (ReplicaRing): in a process of its own -- extra HIP streams slow every later
        # measurement of the process that owns them (streams.py reconstruction_stream)
        try:
            r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'b128_streams.py'), '--json', '1', '2', '4'],
                               capture_output=True, text=True, timeout=240, env=dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get('HIP_VISIBLE_DEVICES', str(local))))
            extra['b128_lmk_only_batches_in_flight'] = dict(json.loads(r.stdout.strip().splitlines()[-1]),
                                                            what='BASELINE configs[1] batches submitted round-robin to N replicas (handle + stream each): throughput of a queue of small batches; latency per batch is b128_lmk_only')
        except Exception as e:
            extra['b128_lmk_only_batches_in_flight'] = dict(error=str(e)[:200])
        extra['sustained_2s'] = sustained

    if rank == 0:
        faces = B * world * args.steps
        n_fallback, _ = model.numerics_report()
        # fp32 in, fp32 out, fp32 accumulation; the GEMM operands are two fp16 pieces each (22-bit significand, 5-bit exponent behind a
        # load-time range proof: numerics.fallback_blocks = blocks the verdict sent to the exact fp32-MFMA kernels on these weights)
        dtype_label = 'f32 (fp16x2 split operands, fp32 accumulate)' if not (args.arch == 'resnet50' and n_fallback >= 53) else 'f32 (fp32 MFMA)'
        if args.lmk_only:
            metric = 'faces/sec (120x120, 68-lmk only)'
            what = 'MobileNetV2 120x120 uint8 crops -> 62 params -> 68 landmarks + pose, ROI affine, all on device (BASELINE configs[1])'
        else:
            metric = 'faces/sec (120x120, 68-lmk + 53215-vert)'
            what = (('ResNet-50 (BASELINE configs[4])' if args.arch == 'resnet50' else 'MobileNetV2') +
                    ' 120x120 uint8 crops -> 62 params -> 68 landmarks + 53215-vertex mesh + pose, ROI affine, all on device' +
                    ('' if args.arch == 'resnet50' else ' (BASELINE configs[2]/[3])'))
        out = dict(metric=metric, value=round(faces / el, 1), unit='faces/s',
                   n_gpus=world, steps=args.steps, warmup=args.warmup, prewarm_s=args.prewarm, ms_per_step=round(el / args.steps * 1e3, 4),
                   higher_is_better=True, scaling='weak', vs_baseline=None, dtype=dtype_label, data='synthetic',
                   config=dict(workload=what,
                               faces_per_gpu_per_step=B, global_batch=B * world, parallelism=f'face-shard x{world}',
                               collectives='one RCCL broadcast of packed constants at init, none in the timed region',
                               streams={2: '2 replicas (handle + HIP stream each) take the batches alternately: batch i+1 runs beside the tail of batch i; every batch does the whole pass into its own buffers', 1: '2: reconstruction of batch i beside the backbone of batch i+1', 0: '1'}[args.overlap],
                               ingest='uint8 NHWC crops resident in HBM (what cv2.resize hands over, synergy3DMM.py:188); the fp32 NCHW '
                                      'forward_test ingest is timed in extra.fp32_ingest_*',
                               mesh_layout=None if args.lmk_only else 'row-pitched [B,3,53248][:, :, :53215] view written in place (same shape / values '
                                           'as the reference tensor, rows 128-byte aligned; the in-repo renderer consumes it without a '
                                           'packed copy); the packed [B,3,53215] layout is timed in extra.packed_output'),
                   roofline=roof)
        out['numerics'] = dict(fallback_blocks=n_fallback, tolerance='<= 1e-4 relative vs the fp32 oracle per face (tests/), measured ~1e-6',
                               guard='load-time interval bounds per block (MobileNetV2), run-time per-tensor maxima (ResNet-50): DESIGN 5.3')
        if dist_info:
            out['distributed'] = dist_info
        if extra:
            out['extra'] = extra
        if args.full and not args.no_cpu_baseline and world == 1 and args.arch == 'mobilenet_v2':
            out['cpu_baseline'] = cpu_baseline(sd, pack)
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + '\n').encode())
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
