"""GPU parity of the visibility buffers through the C ABI: syn_rasterize_triangles / syn_vertex_visibility /
syn_sample_vertex_colors / syn_uv_scatter and the Python entries built on them (Sim3DR.rasterize_triangles, visibility_batch,
vertex_colors_from_image, texture_from_image), against the fixture the reference's own compiled function produced
(tests/golden/visibility_golden.npz; tests/test_visibility_cpu.py pins the definitions of tests/visibility_cases.py to it).

Bars: depth, triangle and weight buffers BIT-identical (bytes, so the sign of zero counts); visibility, UV texture and mask exact;
sampled colours exact (same float32 expression, contraction off on both sides); a whole textured render within the project's
<= 1 grey level on <= 0.1 % of the pixels.  Every step runs once."""
import ctypes as C
import os

import numpy as np
import pytest

import texture_cases as tc
import visibility_cases as vc
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = [getattr(abi, '_SIGS')[s] for s in ('syn_rasterize_triangles', 'syn_vertex_visibility', 'syn_sample_vertex_colors',
                                          'syn_uv_scatter')]                  # KeyError without the feature


@pytest.fixture(scope='module')
def vgold():
    return dict(np.load(os.path.join(HERE, 'golden', 'visibility_golden.npz')))


@pytest.fixture(scope='module')
def small(vgold):
    case = vc.build_mesh_case(vgold['small_cfg'])
    return case, vc.model_for(case)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _pitched(meshes_np):
    """[F,3,pitch][:, :, :n] with NaN in the pad columns, like the tensor reconstruct() returns."""
    import torch
    F, _, n = meshes_np.shape
    store = torch.full((F, 3, (n + 127) // 128 * 128 + 128), float('nan'), device='cuda')
    view = store[:, :, :n]
    view.copy_(torch.from_numpy(meshes_np))
    assert not view.is_contiguous()
    return view


def _raster(m, verts_t, F, planar, init, hw):
    """syn_rasterize_triangles on copies of the caller's initial buffers; numpy (depth, tri, bary)."""
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in init]
    abi.check(m._lib.syn_rasterize_triangles(m._h, verts_t.data_ptr(), F, planar, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                             hw, hw, m._stream()))
    return tuple(d.cpu().numpy() for d in dev)


def test_soup_bit_identical_from_interleaved_packed_and_pitched_input(small, vgold):
    """Zero-area, duplicate, equal-depth, +0 / -0, NaN-corner, off-frame and box-edge triangles, non-default initial buffers."""
    import torch
    seed, hw, ntri = (int(x) for x in vgold['soup_cfg'])
    ver, tri, init = vc.build_soup(seed, hw, ntri)
    m = vc.model_for(small[0])                                           # a handle of its own: the soup replaces its topology
    abi.check(m._lib.syn_load_triangles(m._h, _ptr(tri), ntri, ver.shape[0]))
    want = (vgold['soup_depth'], vgold['soup_tri'], vgold['soup_bary'])
    planar_np = np.ascontiguousarray(ver.T)[None]
    pitched = _pitched(planar_np)
    for name, vt, planar in (('interleaved', torch.from_numpy(ver[None]).cuda(), 0), ('packed', torch.from_numpy(planar_np).cuda(), 1),
                             ('pitched', pitched, pitched.stride(1))):
        got = _raster(m, vt, 1, planar, [a[None] for a in init], hw)
        for g, w_, k in zip(got, want, ('depth', 'triangle', 'weight')):
            print('soup', name, k, 'differing elements', int((g[0].view(np.uint32) != w_.view(np.uint32)).sum()))
            assert _same(g[0], w_), (name, k)
    won = want[1] != init[1]
    assert won.any() and (~won).any() and _same(got[0][0][~won], init[0][~won]) and _same(got[2][0][~won], init[2][~won])
    # the binding's own signature, numpy arrays updated in place (Sim3DR/lib/rasterize.pyx:74-86)
    import Sim3DR
    from synergynet_amd import inference
    inference.set_default_model(m)
    d, t, b = (a.copy() for a in init)
    b2 = b.reshape(hw, hw * 3)                                           # the binding declares a 2-D weight array
    assert Sim3DR.rasterize_triangles(ver, tri, d, t, b2, ntri, hw, hw) is None
    assert _same(d, want[0]) and _same(t, want[1]) and _same(b, want[2])


def test_small_buffers_visibility_colours_and_texture_exact(small, vgold):
    import torch
    from synergynet_amd import sim3dr
    case, m = small
    hw, F, n = case['hw'], case['n_faces'], case['n_vert']
    for name, meshes in (('packed', torch.from_numpy(case['meshes']).cuda()), ('pitched', _pitched(case['meshes']))):
        depth, tri, bary, visible = sim3dr.visibility_batch(m, meshes, hw, hw)
        assert visible.dtype == torch.bool and tuple(visible.shape) == (F, n) and tuple(bary.shape) == (F, hw, hw, 3)
        for g, k in ((depth, 'depth'), (tri, 'tri'), (bary, 'bary')):
            g = g.cpu().numpy()
            print('small', name, k, 'differing elements', int((g.view(np.uint32) != vgold['small_' + k].view(np.uint32)).sum()))
            assert _same(g, vgold['small_' + k]), (name, k)
        vis = visible.cpu().numpy()
        assert np.array_equal(vis, vgold['small_visible'].astype(bool))
        col = sim3dr.vertex_colors_from_image(m, case['img'], meshes).cpu().numpy()
        print('small', name, 'colour max abs diff', float(np.abs(col - vgold['small_colours']).max()))
        assert _same(col, vgold['small_colours'])
        nrm = sim3dr.vertex_colors_from_image(m, torch.from_numpy(case['img']).cuda(), meshes, normalize=True).cpu().numpy()
        assert _same(nrm, vgold['small_colours'] / np.float32(255.0))
        tex, mask = sim3dr.texture_from_image(m, case['img'], meshes)
        assert tex.dtype == torch.uint8 and tuple(tex.shape) == (F, 256, 256, 3) and tuple(mask.shape) == (F, 256, 256)
        assert _same(tex.cpu().numpy(), vgold['small_uv_tex']) and _same(mask.cpu().numpy(), vgold['small_mask'])
    share = vis.mean(1)
    print('visible share', share)
    assert share[0] > 0.99 and 0.30 <= share[1] <= 0.90                 # the turned face hides a real part of itself
    # without occlusion every vertex writes; shared texels go to the highest vertex index
    tex_all, mask_all = sim3dr.texture_from_image(m, case['img'], meshes, occlusion=False)
    for f in range(F):
        wt, wm = vc.uv_scatter(vgold['small_colours'][f], None, case['coord_u'], case['coord_v'])
        assert _same(tex_all[f].cpu().numpy(), wt) and _same(mask_all[f].cpu().numpy(), wm)
    assert not _same(tex_all[1].cpu().numpy(), vgold['small_uv_tex'][1])
    # a non-square texture that is just large enough
    th, tw = int(case['coord_u'].max()) + 1, int(case['coord_v'].max()) + 3
    tex_r, mask_r = sim3dr.texture_from_image(m, case['img'], meshes, tex_hw=(th, tw))
    wt, wm = vc.uv_scatter(vgold['small_colours'][1], vgold['small_visible'][1], case['coord_u'], case['coord_v'], th, tw)
    assert _same(tex_r[1].cpu().numpy(), wt) and _same(mask_r[1].cpu().numpy(), wm)


def test_collision_rule_highest_vertex_index_wins(small):
    """Every vertex on ONE texel: the last visible vertex' colour is what the texel holds."""
    import torch
    case, _ = small
    m = vc.model_for(case)
    n = case['n_vert']
    cu, cv = np.full(n, 7, np.int32), np.full(n, 9, np.int32)
    keep, tri_k = np.arange(n, dtype=np.int32), case['tri_full']
    abi.check(m._lib.syn_load_uv_map(m._h, _ptr(cu), _ptr(cv), n, _ptr(keep), n, _ptr(tri_k), tri_k.shape[0]))
    rng = np.random.default_rng(5)
    col = rng.uniform(-20, 280, (2, n, 3)).astype(np.float32)           # below 0 and above 255: clipped
    col[0, :8] = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5, 300.0, -7.0], np.float32)[:, None]          # ties round to even
    vis = (rng.uniform(0, 1, (2, n)) < 0.5).astype(np.uint8)
    vis[0, -5:], vis[1, -1] = 0, 1
    ct, vt = torch.from_numpy(col).cuda(), torch.from_numpy(vis).cuda()
    tex = torch.full((2, 16, 12, 3), 77, dtype=torch.uint8, device='cuda')
    mask = torch.full((2, 16, 12), 77, dtype=torch.uint8, device='cuda')
    abi.check(m._lib.syn_uv_scatter(m._h, ct.data_ptr(), vt.data_ptr(), 2, 3, tex.data_ptr(), mask.data_ptr(), 16, 12, m._stream()))
    for f in range(2):
        last = int(np.flatnonzero(vis[f])[-1])
        wt, wm = vc.uv_scatter(col[f], vis[f], cu, cv, 16, 12)
        assert np.array_equal(wt[16 - 1 - 7, 9], np.clip(np.rint(col[f, last]), 0, 255).astype(np.uint8)) and wm.sum() == 255
        assert _same(tex[f].cpu().numpy(), wt) and _same(mask[f].cpu().numpy(), wm)
    # rounding and clipping of single vertices, one texel each
    cu2, cv2 = (np.arange(n) // 64).astype(np.int32), (np.arange(n) % 64).astype(np.int32)
    abi.check(m._lib.syn_load_uv_map(m._h, _ptr(cu2), _ptr(cv2), n, _ptr(keep), n, _ptr(tri_k), tri_k.shape[0]))
    tex = torch.empty((2, 64, 64, 3), dtype=torch.uint8, device='cuda')
    mask = torch.empty((2, 64, 64), dtype=torch.uint8, device='cuda')
    abi.check(m._lib.syn_uv_scatter(m._h, ct.data_ptr(), None, 2, 3, tex.data_ptr(), mask.data_ptr(), 64, 64, m._stream()))
    wt, _ = vc.uv_scatter(col[0], None, cu2, cv2, 64, 64)
    assert _same(tex[0].cpu().numpy(), wt)
    assert [int(x) for x in np.flip(wt, 0)[0, :8, 0]] == [0, 2, 2, 254, 255, 0, 255, 0]


def _kept_case(case, img):
    keep = case['assets']['keep_ind']
    return dict(img=img, n_faces=case['n_faces'], kept_meshes=np.ascontiguousarray(case['meshes'][:, :, keep]),
                tri_kept=np.ascontiguousarray(case['assets']['tri_deletion'].T - 1, dtype=np.int32))


def test_texture_feeds_the_textured_path_round_trip_render_and_obj(small, vgold, tmp_path):
    import torch
    from synergynet_amd import inference, sim3dr
    case, m = small
    F = case['n_faces']
    meshes = torch.from_numpy(case['meshes']).cuda()
    tex, mask = sim3dr.texture_from_image(m, case['img'], meshes)
    # round trip: the lookup of the scattered texture gives rint of the sampled colour on every visible vertex that owns its texel
    back = sim3dr.uv_vertex_colors(m, tex, kept=False).cpu().numpy()
    checked = 0
    for f in range(F):
        own = vc.texel_owner(vgold['small_visible'][f].astype(bool), case['coord_u'], case['coord_v'])
        assert np.array_equal(back[f][own], np.clip(np.rint(vgold['small_colours'][f][own]), 0, 255))
        checked += int(own.sum())
    assert checked == int(vgold['small_texel_count'].sum()) > 2000
    # straight into render_batch(uv_tex=) over ANOTHER frame, against the CPU pipeline on the fixture's texture
    other = np.random.default_rng(77).integers(0, 256, case['img'].shape, dtype=np.uint8)
    ov, res = sim3dr.render_batch(m, other, meshes, alpha=0.6, uv_tex=tex)
    kc = _kept_case(case, other)
    keep = case['assets']['keep_ind']
    cpu_tex = np.stack([tc.demo_colors(vgold['small_uv_tex'][f], case['coord_u'], case['coord_v'])[keep].astype(np.float32) / 255.0
                        for f in range(F)])
    live = tc.oracle_render(kc, cpu_tex, impl='oracle')
    for got, want in ((ov.cpu().numpy(), live['overlay']), (res.cpu().numpy(), live['blend'])):
        d = np.abs(got.astype(int) - want.astype(int))
        print('textured render from the photograph: max grey-level diff', int(d.max()), 'share', float((d > 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() <= 1e-3
    assert (live['overlay'] != other).any(2).mean() > 0.05
    # and, through uv_vertex_colors(kept=True), the colours of the coloured OBJ
    col = sim3dr.uv_vertex_colors(m, tex[1], kept=True).cpu().numpy()
    want_col = tc.demo_colors(vgold['small_uv_tex'][1], case['coord_u'], case['coord_v'])[keep].astype(np.float32)
    assert _same(col, want_col)
    inference.write_obj_with_colors(str(tmp_path / 'a.obj'), kc['kept_meshes'][1], case['assets']['tri_deletion'], col)
    inference.write_obj_with_colors(str(tmp_path / 'b.obj'), kc['kept_meshes'][1], case['assets']['tri_deletion'], want_col)
    assert (tmp_path / 'a.obj').read_bytes() == (tmp_path / 'b.obj').read_bytes()


def test_300_faces_in_one_call(small, vgold):
    """Beyond the 254 faces of syn_rasterize: no face field in the key."""
    import torch
    from synergynet_amd import sim3dr
    case, m = small
    hw = case['hw']
    meshes = torch.from_numpy(np.ascontiguousarray(np.tile(case['meshes'], (150, 1, 1)))).cuda()
    assert meshes.shape[0] == 300
    depth, tri, bary, visible = sim3dr.visibility_batch(m, meshes, hw, hw)
    for g, k in ((depth, 'depth'), (tri, 'tri'), (bary, 'bary'), (visible.view(torch.uint8), 'visible')):
        g = g.cpu().numpy()
        assert _same(g, np.tile(vgold['small_' + k], (150,) + (1,) * (g.ndim - 1))), k


def test_full_size_from_reconstructs_pitched_tensor_and_poisoned_workspace(vgold):
    """53215 vertices at 450 x 450 from the pitched tensor model.reconstruct(..., dense=True) returns, pad columns full of NaN."""
    import torch
    from synergynet_amd import sim3dr, synth
    case = vc.build_mesh_case(vgold['full_cfg'])
    m = vc.model_for(case)
    F, hw = case['n_faces'], case['hw']
    rec = m.reconstruct(torch.from_numpy(synth.make_params(F)).cuda(), roi=torch.from_numpy(synth.make_rois(F)).cuda(), dense=True)
    assert not rec.is_contiguous() and rec.shape == (F, 3, case['n_vert'])
    rec.as_strided((F, 3, rec.stride(1)), (rec.stride(0), rec.stride(1), 1)).fill_(float('nan'))
    rec.copy_(torch.from_numpy(case['meshes']))

    def run():
        depth, tri, bary, visible = sim3dr.visibility_batch(m, rec, hw, hw)
        col = sim3dr.vertex_colors_from_image(m, case['img'], rec)
        tex, mask = sim3dr.texture_from_image(m, case['img'], rec)
        return dict(depth=depth, tri=tri, bary=bary, visible=visible.view(torch.uint8), colours=col, uv_tex=tex, mask=mask)

    got = {k: v.cpu().numpy() for k, v in run().items()}
    want_vis = np.unpackbits(vgold['full_visible_bits'], axis=1)[:, :case['n_vert']]
    print('full: visible', got['visible'].sum(1), 'pixels', (got['tri'] >= 0).reshape(F, -1).sum(1), 'texels', (got['mask'] != 0).reshape(F, -1).sum(1))
    assert np.array_equal(got['visible'], want_vis)
    assert np.array_equal((got['tri'] >= 0).reshape(F, -1).sum(1), vgold['full_pixel_count'])
    assert np.array_equal((got['mask'] != 0).reshape(F, -1).sum(1), vgold['full_texel_count'])
    for k, v in got.items():
        assert np.array_equal(vc.sha(v), vgold[f'full_{k}_sha256']), k
    share = got['visible'].mean(1)
    assert share[0] > 0.99 and 0.30 <= share[1] <= 0.90
    uploads = list(m._topology_uploads)
    abi.check(abi.lib().syn_debug_poison_workspace(m._h, 4, 0xFF))
    again = {k: v.cpu().numpy() for k, v in run().items()}
    assert all(_same(again[k], got[k]) for k in got)
    assert m._topology_uploads == uploads                                # the topology and the UV map went up once


def test_alternating_with_rasterize_and_the_kept_topology(small, vgold):
    import torch
    from synergynet_amd import sim3dr
    case, m = small
    hw = case['hw']
    meshes = torch.from_numpy(case['meshes']).cuda()
    first = [x.cpu().numpy() for x in sim3dr.visibility_batch(m, meshes, hw, hw)]
    tex, _ = sim3dr.texture_from_image(m, case['img'], meshes)
    uploads = list(m._topology_uploads)
    assert uploads[0] >= 1 and uploads[1] >= 1
    plain = sim3dr.render_batch(m, case['img'], meshes)[0].cpu().numpy()                  # syn_rasterize shares the key scratch
    texd = sim3dr.render_batch(m, case['img'], meshes, uv_tex=tex)[0].cpu().numpy()       # leaves the kept topology selected
    assert not np.array_equal(plain, texd)
    second = [x.cpu().numpy() for x in sim3dr.visibility_batch(m, meshes, hw, hw)]
    assert all(_same(a, b) for a, b in zip(first, second)) and _same(first[1], vgold['small_tri'])
    assert np.array_equal(sim3dr.render_batch(m, case['img'], meshes)[0].cpu().numpy(), plain)
    assert m._topology_uploads == uploads
    # on the kept topology itself (slot 1): the buffers of the kept meshes, against the order-free rule on the CPU
    kc = _kept_case(case, case['img'])
    abi.check(m._lib.syn_select_topology(m._h, 1))
    got = _raster(m, torch.from_numpy(kc['kept_meshes']).cuda(), 2, 1, vc.fresh_buffers(hw, hw, lead=(2,)), hw)
    want = vc.fresh_buffers(hw, hw, lead=(2,))
    for f in range(2):
        vc.winner_rule(np.ascontiguousarray(kc['kept_meshes'][f].T), kc['tri_kept'], want[0][f], want[1][f], want[2][f], hw, hw)
    assert all(_same(a, b) for a, b in zip(got, want)) and (want[1] >= 0).sum() > 1000
    abi.check(m._lib.syn_select_topology(m._h, 0))


def test_non_finite_and_out_of_frame_vertices_sample_safely(small):
    import torch
    from synergynet_amd import sim3dr
    case, m = small
    hw = case['hw']
    mesh = case['meshes'][:1].copy()
    mesh[0, 0, :6] = [np.nan, np.inf, -np.inf, -5.0, hw + 9.0, hw - 1.0]
    mesh[0, 1, 6:12] = [np.nan, np.inf, -np.inf, -5.0, hw + 9.0, hw - 1.0]
    mesh[0, 0, 12], mesh[0, 1, 12] = 17.0, 23.0                          # exactly on a pixel
    got = sim3dr.vertex_colors_from_image(m, case['img'], torch.from_numpy(mesh).cuda()).cpu().numpy()[0]
    want = vc.sample_colors(case['img'], mesh[0, 0], mesh[0, 1])
    assert _same(got, want)
    assert (got[[0, 1, 2, 6, 7, 8]] == 0).all() and np.array_equal(got[12], case['img'][23, 17].astype(np.float32))


def test_visibility_errors(small):
    import torch
    case, _ = small
    m = vc.model_for(case)
    lib, h = m._lib, m._h
    n = case['n_vert']
    v = torch.zeros((1, 3, n), device='cuda')
    d = torch.zeros((1, 8, 8), device='cuda')
    t = torch.zeros((1, 8, 8), dtype=torch.int32, device='cuda')
    b = torch.zeros((1, 8, 8, 3), device='cuda')
    vis = torch.zeros((1, n), dtype=torch.uint8, device='cuda')
    u8 = torch.zeros((1, 256, 256, 3), dtype=torch.uint8, device='cuda')
    col = torch.zeros((1, n, 3), device='cuda')
    # before any topology / UV map
    assert lib.syn_rasterize_triangles(h, v.data_ptr(), 1, 1, d.data_ptr(), t.data_ptr(), b.data_ptr(), 8, 8, None) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_vertex_visibility(h, t.data_ptr(), 1, 8, 8, vis.data_ptr(), None) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_uv_scatter(h, col.data_ptr(), None, 1, 3, u8.data_ptr(), u8.data_ptr(), 256, 256, None) == abi.SYN_ERR_NOT_LOADED
    tri = case['tri_full']
    abi.check(lib.syn_load_triangles(h, _ptr(tri), tri.shape[0], n))
    assert lib.syn_rasterize_triangles(h, v.data_ptr(), 1, 1, None, t.data_ptr(), b.data_ptr(), 8, 8, None) == abi.SYN_ERR_INVALID
    assert lib.syn_rasterize_triangles(h, v.data_ptr(), 1 << 11, 1, d.data_ptr(), t.data_ptr(), b.data_ptr(), 1 << 10, 1 << 10, None) == abi.SYN_ERR_INVALID
    assert lib.syn_rasterize_triangles(h, v.data_ptr(), 1, n - 1, d.data_ptr(), t.data_ptr(), b.data_ptr(), 8, 8, None) == abi.SYN_ERR_INVALID
    assert lib.syn_sample_vertex_colors(h, v.data_ptr(), 1, 1, u8.data_ptr(), 256, 256, 5, 0, col.data_ptr(), None) == abi.SYN_ERR_INVALID
    # a triangle buffer that holds values that are no triangle marks nothing
    junk = torch.full((1, 8, 8), tri.shape[0], dtype=torch.int32, device='cuda')
    junk[0, 0, 0], junk[0, 0, 1] = -1, -2147483648
    vis.fill_(9)
    abi.check(lib.syn_vertex_visibility(h, junk.data_ptr(), 1, 8, 8, vis.data_ptr(), None))
    assert int(vis.sum()) == 0
    # a texture smaller than the table needs
    cu, cv = np.ascontiguousarray(case['coord_u'], np.int32), np.ascontiguousarray(case['coord_v'], np.int32)
    keep = np.ascontiguousarray(case['assets']['keep_ind'], np.int32)
    tk = np.ascontiguousarray(case['assets']['tri_deletion'].T - 1, dtype=np.int32)
    abi.check(lib.syn_load_uv_map(h, _ptr(cu), _ptr(cv), n, _ptr(keep), keep.size, _ptr(tk), tk.shape[0]))
    need_h, need_w = int(cu.max()) + 1, int(cv.max()) + 1
    assert lib.syn_uv_scatter(h, col.data_ptr(), None, 1, 3, u8.data_ptr(), u8.data_ptr(), need_h - 1, need_w, None) == abi.SYN_ERR_INVALID
    assert lib.syn_uv_scatter(h, col.data_ptr(), None, 1, 3, u8.data_ptr(), u8.data_ptr(), need_h, need_w - 1, None) == abi.SYN_ERR_INVALID
    mk = torch.zeros((1, 256, 256), dtype=torch.uint8, device='cuda')
    assert lib.syn_uv_scatter(h, col.data_ptr(), None, 1, 3, u8.data_ptr(), mk.data_ptr(), need_h, need_w, None) == 0
    from synergynet_amd import sim3dr
    with pytest.raises(ValueError, match='vertices'):
        sim3dr.texture_from_image(m, case['img'], torch.zeros((1, 3, n - 1), device='cuda'))
    with pytest.raises(TypeError):
        sim3dr.vertex_colors_from_image(m, case['img'].astype(np.float32), torch.from_numpy(case['meshes']).cuda())
    torch.cuda.synchronize()
