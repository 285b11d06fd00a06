"""What the packed backbones and the exact families' launch lists are pinned on: shared by tests/golden/make_backbone_blob_digests.py,
tests/golden/make_exact_profile_golden.py, tests/test_backbone_blobs_cpu.py and tests/test_gpu_exact_profile.py.

Both fixtures are records of what THIS project's library computed at the commit that introduced them (nothing from the reference): a
change of the host code that moves one offset, one rounding or one launch of a backbone shows up as another digest or another list."""
import ctypes as C
import hashlib
import os

import numpy as np

from synergynet_amd import abi, synth
from synergynet_amd.synergy3DMM import ARCH_IDS

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, 'golden', 'backbone_blob_digests.npz')
PROFILE = os.path.join(HERE, 'golden', 'exact_profile_golden.npz')
SEED = 3
ARCHS = tuple(ARCH_IDS)                                 # all nine
ARCH_ID_RANGE = range(13)                               # every id 0..12: 5, 7, 9 and 12 were never assigned and answer 0
WORKSPACE_BATCHES = (1, 1024)
MB1_WIDTH = {'mobilenet_1': 1.0, 'mobilenet_05': 0.5, 'mobilenet_2': 2.0}
EXACT_ARCHS = ('mobilenet_1', 'mobilenet_05', 'mobilenet_2', 'ghostnet', 'resnest50', 'resnet18', 'resnet34')
SCHEDULES = (0, 1)                                      # syn_set_schedule codes: per-layer, fused
PROFILE_BATCH = 2
PROFILE_CROPS_SEED = 5


def make_state(arch, seed=SEED):
    if arch == 'mobilenet_v2':
        return synth.make_backbone_state(seed)
    if arch == 'resnet50':
        return synth.make_resnet50_state(seed)
    if arch in MB1_WIDTH:
        return synth.make_mobilenet1_state(seed, MB1_WIDTH[arch])
    if arch == 'ghostnet':
        return synth.make_ghostnet_state(seed)
    if arch == 'resnest50':
        return synth.make_resnest50_state(seed)
    return synth.make_resnet_basic_state(arch, seed)


def blob_record(arch):
    """(bytes, backbone_floats of the header, sha256 hex digest) of the backbone-only constants blob of `arch`, packed without a device"""
    from synergynet_amd.dist import pack_constants_host
    from synergynet_amd.synergy3DMM import parse_constants_header
    blob = pack_constants_host(pack=None, backbone_state=make_state(arch), arch=arch)
    hd = parse_constants_header(blob[:256].tobytes())
    return int(blob.size), int(hd['backbone_floats']), hashlib.sha256(blob.tobytes()).hexdigest()


def abi_numbers():
    """dict name -> array over ARCH_ID_RANGE (or over WORKSPACE_BATCHES) of what the device-free size queries of the C ABI answer"""
    lib = abi.lib()
    ids = list(ARCH_ID_RANGE)
    return {
        'workspace_bytes': np.array([lib.syn_workspace_bytes(None, B) for B in WORKSPACE_BATCHES], dtype=np.uint64),
        'host_bytes_backbone': np.array([lib.syn_pack_constants_host_bytes(a, 1, 0, 0) for a in ids], dtype=np.uint64),
        'host_bytes_empty': np.array([lib.syn_pack_constants_host_bytes(a, 0, 0, 0) for a in ids], dtype=np.uint64),
        'host_bytes_both': np.array([lib.syn_pack_constants_host_bytes(a, 1, 700, 68) for a in ids], dtype=np.uint64),
        'mobilenet1_flat_count': np.array([lib.syn_mobilenet1_flat_count(a) for a in ids], dtype=np.uint64),
        'mobilenet1_flops_per_face': np.array([lib.syn_mobilenet1_flops_per_face(a) for a in ids], dtype=np.float64),
        'resnet_basic_flat_count': np.array([lib.syn_resnet_basic_flat_count(a) for a in ids], dtype=np.uint64),
        'resnet_basic_flops_per_face': np.array([lib.syn_resnet_basic_flops_per_face(a) for a in ids], dtype=np.float64),
        'flat_count_noarg': np.array([lib.syn_backbone_flat_count(), lib.syn_resnet50_flat_count(), lib.syn_ghostnet_flat_count(),
                                      lib.syn_resnest50_flat_count()], dtype=np.uint64),
        'flops_per_face_noarg': np.array([lib.syn_backbone_flops_per_face(), lib.syn_resnet50_flops_per_face(),
                                          lib.syn_ghostnet_flops_per_face(), lib.syn_resnest50_flops_per_face()], dtype=np.float64),
    }


def profile_crops():
    return synth.make_crops(PROFILE_BATCH, seed=PROFILE_CROPS_SEED)


def launch_profile(model, crops_cuda, sched):
    """(launch count by syn_backbone_launch_count, codes [n] int32, flops [n] float64) of one profiled forward of `crops_cuda` under
    syn_set_schedule(sched); the capacity handed to syn_backbone_profile is larger than any family's list, so n is the profile's own."""
    lib, h = model._lib, model._h
    prev = lib.syn_set_schedule(h, sched)
    assert prev >= 0, lib.syn_last_error()
    try:
        count = lib.syn_backbone_launch_count(h)
        cap = 256
        feat, ms, fl = np.full(cap, -1, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.float64)
        n = lib.syn_backbone_profile(h, crops_cuda.data_ptr(), crops_cuda.shape[0], cap, feat.ctypes.data_as(C.c_void_p),
                                     ms.ctypes.data_as(C.c_void_p), fl.ctypes.data_as(C.c_void_p))
        assert n > 0, lib.syn_last_error()
    finally:
        lib.syn_set_schedule(h, prev)
    return int(count), feat[:n].copy(), fl[:n].copy()
