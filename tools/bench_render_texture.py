"""GPU box: per-pixel texture mapping on full-size meshes (F faces of 53215 vertices from the pitched tensor), device-resident,
event-timed and ALTERNATING after warm-up (all variants see the same clocks), on 450x450 and 1024x1024 frames:
  rasterize_triangles     syn_rasterize_triangles into pre-initialised buffers, the yardstick: the same walk, 20 bytes per pixel per face
  render_texture_faces    syn_render_texture, shared = 0: every face its own float32 image + depth planes (16 bytes per pixel per face)
  render_texture_shared   syn_render_texture, shared = 1: all faces in ONE z-buffer, uint8 image
  render_batch_uv_tex     render_batch(uv_tex=): one texel per kept vertex, lit, interpolated and blended (what existed before)
usage: python tools/bench_render_texture.py [F] [rounds] [once]     (`once`: one pass of each variant, for a kernel trace)"""
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
tex = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (512, 512, 3), dtype=np.uint8)).cuda()
store = torch.empty((F, 3, 53248), device='cuda')
mt = store[:, :, :53215]                                   # the pitched view reconstruct() returns
planar = sim3dr._planar_arg(mt)

for H in (450, 1024):
    W = H
    mt.copy_(torch.from_numpy(synth.make_face_meshes(F, n_vert=53215, height=H, width=W, seed=5)))
    img_t = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    sim3dr.render_texture_batch(m, mt, tex, H, W)          # uploads the topology and the texture coordinates, selects slot 0
    depth = torch.empty((F, H, W), device='cuda')
    tbuf = torch.empty((F, H, W), dtype=torch.int32, device='cuda')
    bary = torch.empty((F, H, W, 3), device='cuda')
    image = torch.empty((F, H, W, 3), device='cuda')
    image8 = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')

    def reset():                                            # outside the timed region: every round walks against fresh buffers
        depth.fill_(-1e8); tbuf.fill_(-1); bary.zero_(); image.zero_(); image8.zero_()
        abi.check(m._lib.syn_select_topology(m._h, 0))

    def rasterize_triangles():
        abi.check(m._lib.syn_rasterize_triangles(m._h, mt.data_ptr(), F, planar, depth.data_ptr(), tbuf.data_ptr(), bary.data_ptr(), H, W,
                                                 m._stream()))

    def render_texture_faces():
        abi.check(m._lib.syn_render_texture(m._h, mt.data_ptr(), F, planar, tex.data_ptr(), 1, 1, 512, 512, 3, 1, image.data_ptr(), 0,
                                            depth.data_ptr(), H, W, 3, 0, m._stream()))

    def render_texture_shared():
        abi.check(m._lib.syn_render_texture(m._h, mt.data_ptr(), F, planar, tex.data_ptr(), 1, 1, 512, 512, 3, 1, image8.data_ptr(), 1,
                                            depth.data_ptr(), H, W, 3, 1, m._stream()))

    variants = dict(rasterize_triangles=rasterize_triangles, render_texture_faces=render_texture_faces,
                    render_texture_shared=render_texture_shared, render_batch_uv_tex=lambda: sim3dr.render_batch(m, img_t, mt, uv_tex=tex))
    for _ in range(1 if once else 3):
        for fn in variants.values():
            reset(); fn()
    torch.cuda.synchronize()
    if once:
        continue
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ms[k].append(a.elapsed_time(b))
    for k, v in ms.items():
        v = np.array(v) * 1e3
        print(f'{H}x{W} F={F} {k:22s}: median {np.median(v):8.1f} us  min {v.min():8.1f}  p90 {np.percentile(v, 90):8.1f}  ({rounds} alternating rounds)')
    reset(); render_texture_faces()
    print(f'{H}x{W} pixels drawn per face {[int(x) for x in (depth > -1e8).flatten(1).sum(1)]}; uploads {m._topology_uploads} {m._tex_coord_uploads}')
