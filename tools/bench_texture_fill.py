"""Needs a GPU.  The push-pull completion of UV textures (syn_texture_fill), device-resident, event-timed and ALTERNATING after warm-up
(all variants see the same clocks):
  fill_T8_256           T = 8 textures of 256 x 256 x 3 as texture_from_image leaves them (one texel per vertex, occlusion)
  fill_T1_1024          one 1024 x 1024 x 3 texture, 20 % of its texels valid
  merge_T8_256          the same 8 textures merged into one and filled
  texture_from_image    frame + meshes -> UV textures, F = 8 full-size meshes at 450 px, fill=False: the yardstick
  texture_from_image+f  the same with fill=True
After the timings: the bytes each variant needs and the bytes its three kernels move, computed from the shapes.
usage: python tools/bench_texture_fill.py [rounds] [once | launches]
  once      one pass of each variant, to be run under `rocprofv3 --kernel-trace --stats` for the time per kernel
  launches  only syn_texture_fill, one call with T = 1 and one with T = 300 (16 x 16), to be run under
            `rocprofv3 --kernel-trace --stats`: the trace then holds the launches of exactly two calls"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import abi, synth, sim3dr
from synergynet_amd.synergy3DMM import SynergyNet

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
mode = sys.argv[2] if len(sys.argv) > 2 else ''
F = 8
assets = synth.make_uv_assets(53215)
tri = synth.make_grid_topology(n_vert=53215)
m = SynergyNet(device='cuda:0', pack=dict(synth.make_3dmm(n_vert=640), tri=np.ascontiguousarray(tri.T + 1), **assets),
               backbone_state=synth.make_backbone_state())


def fill(tex, mask, out, merge=0):
    T, th, tw, ch = tex.shape
    abi.check(m._lib.syn_texture_fill(m._h, tex.data_ptr(), mask.data_ptr(), T, th, tw, ch, merge, out.data_ptr(), m._stream()))


if mode == 'launches':
    rng = np.random.default_rng(0)
    for T in (1, 300):
        tex = torch.from_numpy(rng.integers(0, 256, (T, 16, 16, 3), dtype=np.uint8)).cuda()
        mask = torch.from_numpy((rng.uniform(0, 1, (T, 16, 16)) < 0.2).astype(np.uint8)).cuda()
        fill(tex, mask, torch.empty_like(tex))
        torch.cuda.synchronize()
    sys.exit(0)

H = W = 450
img_t = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
store = torch.empty((F, 3, 53248), device='cuda')
mt = store[:, :, :53215]                                   # the pitched view reconstruct() returns
mt.copy_(torch.from_numpy(synth.make_face_meshes(F, n_vert=53215, height=H, width=W, seed=5)))
tex8, mask8 = sim3dr.texture_from_image(m, img_t, mt)     # uploads the topology and the UV map
out8, out1 = torch.empty_like(tex8), torch.empty_like(tex8[:1])
rng = np.random.default_rng(1)
texL = torch.from_numpy(rng.integers(0, 256, (1, 1024, 1024, 3), dtype=np.uint8)).cuda()
maskL = torch.from_numpy((rng.uniform(0, 1, (1, 1024, 1024)) < 0.2).astype(np.uint8) * 255).cuda()
outL = torch.empty_like(texL)

variants = {'fill_T8_256': lambda: fill(tex8, mask8, out8), 'fill_T1_1024': lambda: fill(texL, maskL, outL),
            'merge_T8_256': lambda: fill(tex8, mask8, out1, 1),
            'texture_from_image': lambda: sim3dr.texture_from_image(m, img_t, mt),
            'texture_from_image+f': lambda: sim3dr.texture_from_image(m, img_t, mt, fill=True)}
for _ in range(1 if mode == 'once' else 3):
    for fn in variants.values():
        fn()
torch.cuda.synchronize()
if mode == 'once':
    sys.exit(0)
us = {k: [] for k in variants}
for _ in range(rounds):
    for k, fn in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        us[k].append(a.elapsed_time(b) * 1e3)
for k, v in us.items():
    v = np.array(v)
    print(f'{k:22s}: median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({rounds} alternating rounds)')


def traffic(T, th, tw, ch, views=1):
    """Bytes per call: what the definition needs (texture and mask in, texture out) and what the three kernels read and write."""
    tiles = ((th + 63) // 64) * ((tw + 63) // 64)
    need = T * th * tw * (ch + 1) + (T // views) * th * tw * ch
    to = T // views
    pyr = to * tiles * 1365 * (ch + 1) * 4                                        # levels 1..6, written once by push
    ring = to * tiles * sum((n + 2) ** 2 for n in (32, 16, 8, 4, 2)) * (ch + 1) * 4   # read by pull (an upper bound: w == 0 skips the colours)
    moved = 2 * T * th * tw * (ch + 1) + pyr + ring + to * th * tw * ch + to * tiles * (2 * 4 + 9 * 4 + (ch + 1) * 4)
    return need, moved


for name, args in (('fill_T8_256', (8, 256, 256, 3)), ('fill_T1_1024', (1, 1024, 1024, 3)), ('merge_T8_256', (8, 256, 256, 3, 8))):
    need, moved = traffic(*args)
    t = np.median(us[name]) * 1e-6
    print(f'{name:22s}: needs {need / 1e6:6.2f} MB, kernels move {moved / 1e6:6.2f} MB ({moved / need:.1f}x) -> {moved / t / 1e9:7.1f} GB/s at the median')
print(f'valid texels per texture {[int(x) for x in (mask8 != 0).flatten(1).sum(1)]} of {256 * 256}; uploads {m._topology_uploads}')
