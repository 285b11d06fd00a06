"""GPU box: the visibility buffers on full-size meshes (F faces of 53215 vertices from the pitched tensor, 450x450 frame),
device-resident, event-timed and ALTERNATING after warm-up (all variants see the same clocks):
  rasterize            syn_rasterize (z-buffer + colours into one image), the yardstick
  rasterize_triangles  syn_rasterize_triangles into pre-initialised buffers (per face: depth, triangle, weights)
  texture_from_image   frame + meshes -> UV textures end to end (sample, buffers incl. their initialisation, visibility, scatter)
usage: python tools/bench_visibility.py [F] [rounds] [once]     (`once`: one pass of each variant, for a kernel trace)"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import abi, synth, sim3dr
from synergynet_amd.synergy3DMM import SynergyNet

F = int(sys.argv[1]) if len(sys.argv) > 1 else 8
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 30
once = len(sys.argv) > 3 and sys.argv[3] == 'once'
assets = synth.make_uv_assets(53215)
tri = synth.make_grid_topology(n_vert=53215)
m = SynergyNet(device='cuda:0', pack=dict(synth.make_3dmm(n_vert=640), tri=np.ascontiguousarray(tri.T + 1), **assets),
               backbone_state=synth.make_backbone_state())
H = W = 450
img_t = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
store = torch.empty((F, 3, 53248), device='cuda')
mt = store[:, :, :53215]                                   # the pitched view reconstruct() returns
mt.copy_(torch.from_numpy(synth.make_face_meshes(F, n_vert=53215, height=H, width=W, seed=5)))
planar = sim3dr._planar_arg(mt)
sim3dr.visibility_batch(m, mt, H, W)                       # uploads the topology, selects it
colors = torch.rand((F, 53215, 3), device='cuda')
canvas = img_t.clone()
depth = torch.full((F, H, W), -1e8, device='cuda')
tbuf = torch.full((F, H, W), -1, dtype=torch.int32, device='cuda')
bary = torch.zeros((F, H, W, 3), device='cuda')


def rasterize():
    abi.check(m._lib.syn_rasterize(m._h, mt.data_ptr(), colors.data_ptr(), F, planar, 3, canvas.data_ptr(), H, W, 0, m._stream()))


def rasterize_triangles():                                  # buffers keep the previous round's winners: same walk, same atomics,
    abi.check(m._lib.syn_rasterize_triangles(m._h, mt.data_ptr(), F, planar, depth.data_ptr(), tbuf.data_ptr(), bary.data_ptr(), H, W,
                                             m._stream()))  # so they are reset outside the timed region below


def reset():
    depth.fill_(-1e8); tbuf.fill_(-1); bary.zero_()


variants = dict(rasterize=rasterize, rasterize_triangles=rasterize_triangles,
                texture_from_image=lambda: sim3dr.texture_from_image(m, img_t, mt))
for _ in range(1 if once else 3):
    for fn in variants.values():
        reset(); fn()
torch.cuda.synchronize()
if once:
    sys.exit(0)
ms = {k: [] for k in variants}
for _ in range(rounds):
    for k, fn in variants.items():
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms[k].append(a.elapsed_time(b))
for k, v in ms.items():
    v = np.array(v) * 1e3
    print(f'F={F} {k:20s}: median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({rounds} alternating rounds)')
vis = sim3dr.visibility_batch(m, mt, H, W)
print(f'pixels won per face {[(int(x)) for x in (vis[1] >= 0).flatten(1).sum(1)]}; visible share {[round(float(x), 3) for x in vis[3].float().mean(1)]}; '
      f'uploads {m._topology_uploads}')
