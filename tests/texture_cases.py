"""Inputs of the textured-mesh tests, rebuilt from the seeds a fixture case stores (tests/golden/texture_golden.npz is written by
tests/golden/make_texture_golden.py from exactly these inputs): grid meshes, frame, UV assets and UV texture images."""
import numpy as np

CFG_FIELDS = ('rows', 'cols', 'n_vert', 'hw', 'n_faces', 'mesh_seed', 'img_seed', 'uv_seed', 'tex_seed', 'n_tex', 'smooth')
TEX_HW = 256          # the demos' UV texture images are 256 x 256 (coord = int(uv * 255))


def build(cfg):
    from synergynet_amd import params, synth
    c = dict(zip(CFG_FIELDS, (int(x) for x in cfg)))
    rows, cols, nv, hw = c['rows'], c['cols'], c['n_vert'], c['hw']
    sub = nv if rows * cols != nv else None
    assets = synth.make_uv_assets(sub, rows, cols, seed=c['uv_seed'])
    meshes = synth.make_face_meshes(c['n_faces'], rows, cols, n_vert=sub, height=hw, width=hw, seed=c['mesh_seed'])
    if c['smooth']:                                       # 1: a compressible frame, 2: and a compressible texture (small fixture)
        yy, xx = np.mgrid[0:hw, 0:hw]
        bx, by = xx // 16, yy // 16                       # 16-pixel blocks of flat colour
        img = np.stack([40 + 13 * ((bx + by) % 16), 200 - 11 * (bx % 16), 90 + 9 * (by % 16)], 2).astype(np.uint8)
    else:
        img = np.random.default_rng(c['img_seed']).integers(0, 256, (hw, hw, 3), dtype=np.uint8)
    uv_tex = np.random.default_rng(c['tex_seed']).integers(0, 256, (c['n_tex'], TEX_HW, TEX_HW, 3), dtype=np.uint8)
    if c['smooth'] == 2:
        ty, tx = np.mgrid[0:TEX_HW, 0:TEX_HW] / TEX_HW
        waves = [np.sin(7 * tx + 3 * ty), np.cos(5 * ty - 2 * tx), np.sin(9 * tx * ty)]
        uv_tex = np.repeat(np.stack([np.rint(150 + 100 * w) for w in waves], 2).astype(np.uint8)[None], c['n_tex'], 0)
    coord_u, coord_v = params.uv_pixel_coords(assets['uv_vert'])
    keep = assets['keep_ind']
    return dict(c, assets=assets, meshes=meshes, img=img, uv_tex=uv_tex, coord_u=coord_u, coord_v=coord_v, keep=keep,
                tri_full=synth.make_grid_topology(rows, cols, n_vert=sub),
                tri_kept=np.ascontiguousarray(assets['tri_deletion'].T - 1, dtype=np.int32),
                kept_meshes=np.ascontiguousarray(meshes[:, :, keep]))


def demo_colors(uv_tex_one, coord_u, coord_v):
    """uv_texture_realFaces.py:109-110 in numpy: one colour per vertex of one texture image, uint8 [n_vert,ch]."""
    return np.flip(uv_tex_one, axis=0)[coord_u, coord_v, :]


def demo_tex(case):
    """The `tex` argument of the demo (uv_texture_realFaces.py:115): [n_keep,3] for one texture image, [T,n_keep,3] for several."""
    t = np.stack([demo_colors(u, case['coord_u'], case['coord_v'])[case['keep'], :].astype(np.float32) / 255.0 for u in case['uv_tex']])
    return np.ascontiguousarray(t[0] if t.shape[0] == 1 else t)


def oracle_render(case, tex, impl='oracle', alpha=0.6):
    """utils/render.py:38-45 on the kept meshes with the checker's RenderPipeline: a shared [n,3] tex is multiplied in place by
    every face in turn (it IS mutated, as in the reference), a [F,n,3] one gives every face its own.  Returns per-face
    normals, light, colours, the solid overlay and the blend."""
    from oracle import sim3dr as osim
    app = osim.RenderPipeline(impl=impl, **osim.RENDER_CFG)
    overlap = case['img'].copy()
    normals, lights, colours = [], [], []
    for f in range(case['n_faces']):
        ver = np.ascontiguousarray(case['kept_meshes'][f].T)
        normals.append(osim.get_normal(ver, case['tri_kept'], impl=impl))
        lights.append(app.light(ver, case['tri_kept']))
        t = tex if tex.ndim == 2 else tex[f]
        overlap = app(ver, case['tri_kept'], overlap, texture=t)
        colours.append(t.copy())
    return dict(normal=np.stack(normals), light=np.stack(lights), colours=np.stack(colours), overlay=overlap,
                blend=osim.add_weighted(case['img'], 1 - alpha, overlap, alpha))
