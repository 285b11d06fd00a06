"""GPU box: render_batch textured against untextured on full-size meshes (53215 vertices before keeping, 450x450 frame),
device-resident, event-timed and ALTERNATING after warm-up (both variants see the same clocks).
usage: python tools/bench_texture.py [F] [rounds]"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synergynet_amd import synth, sim3dr
from synergynet_amd.synergy3DMM import SynergyNet

F = int(sys.argv[1]) if len(sys.argv) > 1 else 8
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 30
assets = synth.make_uv_assets(53215)
tri = synth.make_grid_topology(n_vert=53215)
m = SynergyNet(device='cuda:0', pack=dict(synth.make_3dmm(n_vert=640), tri=np.ascontiguousarray(tri.T + 1), **assets),
               backbone_state=synth.make_backbone_state())
H = W = 450
img_t = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
uv_tex = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (256, 256, 3), dtype=np.uint8)).cuda()
store = torch.empty((F, 3, 53248), device='cuda')
mt = store[:, :, :53215]                                   # the pitched view reconstruct() returns
mt.copy_(torch.from_numpy(synth.make_face_meshes(F, n_vert=53215, height=H, width=W, seed=5)))
variants = dict(untextured=lambda: sim3dr.render_batch(m, img_t, mt), textured=lambda: sim3dr.render_batch(m, img_t, mt, uv_tex=uv_tex))
for _ in range(3):
    for fn in variants.values(): fn()
torch.cuda.synchronize()
ms = {k: [] for k in variants}
for _ in range(rounds):
    for k, fn in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms[k].append(a.elapsed_time(b))
for k, v in ms.items():
    v = np.array(v) * 1e3
    print(f'F={F} {k:10s}: median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({rounds} alternating rounds)')
print(f'kept {assets["keep_ind"].size} of 53215 vertices, {assets["tri_deletion"].shape[1]} of {tri.shape[0]} triangles; uploads {m._topology_uploads}')
