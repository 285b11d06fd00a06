"""GPU parity of the textured-mesh path (the reference's uv_texture_realFaces.py / artistic.py) through the C ABI:
syn_load_uv_map / syn_uv_colors / syn_gather_vertices / syn_mesh_shade_textured + syn_select_topology, syn_rasterize and
syn_add_weighted, against the fixture the real reference produced (tests/golden/texture_golden.npz) and the live CPU oracle
(oracle/sim3dr.py, pinned to that fixture by tests/test_texture_cpu.py).

Bars, as in tests/test_gpu_render.py: lookups, gathers, normals and rasterised images are BIT-exact; light and colours agree
to 1e-6 absolute (numpy's float32 power against the kernel's exactly rounded product), hence <= 1 grey level on <= 0.1 % of
the pixels for a whole pipeline, whose blend is exact given its overlay.  Every step runs once."""
import ctypes as C
import os

import numpy as np
import pytest

import texture_cases as tc
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = [getattr(abi, '_SIGS')[s] for s in ('syn_load_uv_map', 'syn_select_topology', 'syn_uv_colors', 'syn_gather_vertices',
                                          'syn_mesh_shade_textured')]          # KeyError without the feature


@pytest.fixture(scope='module')
def tgold():
    return dict(np.load(os.path.join(HERE, 'golden', 'texture_golden.npz')))


def _model(case, n_vert=None):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    pack = dict(synth.make_3dmm(n_vert=n_vert or case['n_vert']), **case['assets'])
    pack['tri'] = np.ascontiguousarray(case['tri_full'].T + 1)
    return SynergyNet(device='cuda:0', pack=pack, backbone_state=synth.make_backbone_state())


@pytest.fixture(scope='module')
def small(tgold):
    case = tc.build(tgold['small_cfg'])
    return case, _model(case)


@pytest.fixture(scope='module')
def perface(tgold):
    case = tc.build(tgold['perface_cfg'])
    return case, _model(case)


def _close_images(a, b):
    d = np.abs(a.astype(int) - b.astype(int))
    print('image diff: max', int(d.max()), 'share', float((d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _load_uv(m, case):
    cu, cv = np.ascontiguousarray(case['coord_u'], np.int32), np.ascontiguousarray(case['coord_v'], np.int32)
    keep = np.ascontiguousarray(case['keep'], np.int32)
    return m._lib.syn_load_uv_map(m._h, _ptr(cu), _ptr(cv), cu.size, _ptr(keep), keep.size, _ptr(case['tri_kept']), case['tri_kept'].shape[0])


def test_uv_colours_kept_and_full_raw_and_normalised(small, perface):
    import torch
    from synergynet_amd import sim3dr
    for case, m in (small, perface):
        for uv_tex in (case['uv_tex'], case['uv_tex'][0]):               # [T,H,W,3] and [H,W,3]
            imgs = uv_tex if uv_tex.ndim == 4 else uv_tex[None]
            want_all = np.stack([tc.demo_colors(u, case['coord_u'], case['coord_v']) for u in imgs])
            for kept in (True, False):
                want = want_all[:, case['keep'], :] if kept else want_all
                raw = sim3dr.uv_vertex_colors(m, uv_tex, kept=kept, normalize=False).cpu().numpy()
                nrm = sim3dr.uv_vertex_colors(m, torch.from_numpy(uv_tex).cuda(), kept=kept, normalize=True).cpu().numpy()
                if uv_tex.ndim == 3:
                    raw, nrm = raw[None], nrm[None]
                assert raw.dtype == np.float32 and np.array_equal(raw, want.astype(np.float32))
                assert np.array_equal(nrm, want.astype(np.float32) / 255.0)
    assert np.array_equal(sim3dr.uv_vertex_colors(small[1], small[0]['uv_tex'][0], kept=True, normalize=True).cpu().numpy(), tc.demo_tex(small[0]))


def test_gather_from_packed_and_pitched_with_nan_pads(small):
    import torch
    from synergynet_amd import sim3dr
    case, m = small
    meshes = case['meshes']
    F, _, n = meshes.shape
    got = sim3dr.gather_kept(m, torch.from_numpy(meshes).cuda()).cpu().numpy()
    assert np.array_equal(got, case['kept_meshes'])
    store = torch.full((F, 3, (n + 127) // 128 * 128), float('nan'), device='cuda')
    pitched = store[:, :, :n]
    pitched.copy_(torch.from_numpy(meshes))
    assert not pitched.is_contiguous()
    got = sim3dr.gather_kept(m, pitched).cpu().numpy()
    assert np.array_equal(got, case['kept_meshes']) and not np.isnan(got).any()


def _shade_kept(m, case, tex, shared):
    """syn_select_topology(1) + syn_mesh_shade_textured on the kept meshes; returns normal, light, colours, tex afterwards."""
    import torch
    from synergynet_amd import sim3dr
    abi.check(_load_uv(m, case))
    abi.check(m._lib.syn_select_topology(m._h, 1))
    km = torch.from_numpy(case['kept_meshes']).cuda()
    tex_t = torch.from_numpy(tex.copy()).cuda()
    normal, light, colours = sim3dr._shade_textured(m, km, 1, sim3dr._cfg16(sim3dr.RenderPipeline(**sim3dr.RENDER_CFG)), tex_t, shared, want_light=True)
    return normal.cpu().numpy(), light.cpu().numpy(), colours.cpu().numpy(), tex_t.cpu().numpy()


def test_kept_topology_normals_bit_exact_light_and_colours_close(small, perface, tgold):
    for name, (case, m) in (('small', small), ('perface', perface)):
        tex = tc.demo_tex(case)
        normal, light, colours, tex_after = _shade_kept(m, case, tex, shared=tex.ndim == 2)
        assert np.array_equal(normal, tgold[name + '_normal'])
        print(name, 'light err', np.abs(light - tgold[name + '_light']).max(), 'colour err', np.abs(colours - tgold[name + '_colours']).max())
        np.testing.assert_allclose(light, tgold[name + '_light'], rtol=0, atol=1e-6)
        np.testing.assert_allclose(colours, tgold[name + '_colours'], rtol=0, atol=1e-6)
        if name == 'small':
            np.testing.assert_allclose(tex_after, tgold['small_tex_final'], rtol=0, atol=1e-6)
            assert np.array_equal(tex_after, colours[-1])
            assert np.array_equal(colours[1], (tex * light[0]) * light[1])      # float32 products, left to right
        else:
            assert np.array_equal(tex_after, tex) and np.array_equal(colours, tex * light)


def test_rasteriser_on_kept_topology_bit_exact_given_fixture_colours(small, perface, tgold):
    import torch
    for name, (case, m) in (('small', small), ('perface', perface)):
        abi.check(_load_uv(m, case))
        abi.check(m._lib.syn_select_topology(m._h, 1))
        km = torch.from_numpy(case['kept_meshes']).cuda()
        col = torch.from_numpy(tgold[name + '_colours']).cuda()
        img = torch.from_numpy(case['img']).cuda()
        hw = case['hw']
        abi.check(m._lib.syn_rasterize(m._h, km.data_ptr(), col.data_ptr(), km.shape[0], 1, 3, img.data_ptr(), hw, hw, 0, m._stream()))
        assert np.array_equal(img.cpu().numpy(), tgold[name + '_overlay'])


def _check_pipeline(case, overlay, blend, gold_overlay, tex):
    from oracle import sim3dr as osim
    _close_images(overlay, gold_overlay)
    live = tc.oracle_render(case, tex, impl='oracle')
    _close_images(overlay, live['overlay'])
    assert np.array_equal(blend, osim.add_weighted(case['img'], 1 - 0.6, overlay, 0.6))
    return live


def test_render_with_tex_and_connectivity_like_the_demo(small, tgold):
    """utils/render.py:31-50 as uv_texture_realFaces.py:115-116 calls it: kept meshes, tex per kept vertex, connectivity =
    tri_deletion - 1; the caller's tex is left multiplied."""
    from synergynet_amd import inference, sim3dr
    case, m = small
    inference.set_default_model(m)
    tex = tc.demo_tex(case)
    tex0 = tex.copy()
    # the overlay is not returned by render(): take it from the device entry the same call goes through
    res = sim3dr.render(case['img'], [case['kept_meshes'][f] for f in range(case['n_faces'])], alpha=0.6, tex=tex,
                        connectivity=case['assets']['tri_deletion'] - 1)
    np.testing.assert_allclose(tex, tgold['small_tex_final'], rtol=0, atol=1e-6)
    assert not np.array_equal(tex, tex0)
    import torch
    ov, res2 = sim3dr._render_textured(m, case['img'], torch.from_numpy(case['kept_meshes']).cuda(), tex0.copy(), 0.6,
                                       sim3dr.RenderPipeline(**sim3dr.RENDER_CFG))
    assert np.array_equal(res2.cpu().numpy(), res)
    _check_pipeline(case, ov.cpu().numpy(), res, tgold['small_overlay'], tex0.copy())
    _close_images(res, tgold['small_blend'])


def test_render_batch_uv_tex_shared_and_per_face(small, perface, tgold):
    import torch
    from synergynet_amd import sim3dr
    for name, (case, m) in (('small', small), ('perface', perface)):
        uv_tex = case['uv_tex'][0] if name == 'small' else case['uv_tex']
        ov, res = sim3dr.render_batch(m, case['img'], torch.from_numpy(case['meshes']).cuda(), alpha=0.6, uv_tex=uv_tex)
        _check_pipeline(case, ov.cpu().numpy(), res.cpu().numpy(), tgold[name + '_overlay'], tc.demo_tex(case))
        # the same through tex= : a device tensor is updated in place when shared, a numpy array likewise
        tex_t = torch.from_numpy(tc.demo_tex(case)).cuda()
        ov2, res2 = sim3dr.render_batch(m, case['img'], torch.from_numpy(case['meshes']).cuda(), alpha=0.6, tex=tex_t)
        assert np.array_equal(ov2.cpu().numpy(), ov.cpu().numpy()) and np.array_equal(res2.cpu().numpy(), res.cpu().numpy())
        if name == 'small':
            np.testing.assert_allclose(tex_t.cpu().numpy(), tgold['small_tex_final'], rtol=0, atol=1e-6)
            tex_np = tc.demo_tex(case)
            sim3dr.render_batch(m, case['img'], torch.from_numpy(case['meshes']).cuda(), alpha=0.6, tex=tex_np)
            assert np.array_equal(tex_np, tex_t.cpu().numpy())
        else:
            assert np.array_equal(tex_t.cpu().numpy(), tc.demo_tex(case))


def test_render_pipeline_call_with_texture_runs_on_device_and_mutates(small, tgold):
    from synergynet_amd import inference, sim3dr
    case, m = small
    inference.set_default_model(m)
    tex = tc.demo_tex(case)
    app = sim3dr.RenderPipeline(**sim3dr.RENDER_CFG)
    overlap = case['img'].copy()
    for f in range(case['n_faces']):
        overlap = app(np.ascontiguousarray(case['kept_meshes'][f].T), case['tri_kept'], overlap, texture=tex)
    _close_images(overlap, tgold['small_overlay'])
    np.testing.assert_allclose(tex, tgold['small_tex_final'], rtol=0, atol=1e-6)


def test_full_size_from_reconstructs_pitched_tensor(tgold):
    """53215 vertices before keeping, 450 x 450: the meshes sit in the pitched tensor model.reconstruct(..., dense=True) returns
    (empty_vertices: [F,3,53248][:, :, :53215], pad columns full of NaN) and are consumed in place."""
    import torch
    from synergynet_amd import sim3dr, synth
    case = tc.build(tgold['full_cfg'])
    assert [case['keep'].size, case['tri_kept'].shape[0]] == [int(x) for x in tgold['full_kept']]
    m = _model(case)
    F = case['n_faces']
    rec = m.reconstruct(torch.from_numpy(synth.make_params(F)).cuda(), roi=torch.from_numpy(synth.make_rois(F)).cuda(), dense=True)
    assert not rec.is_contiguous() and rec.shape == (F, 3, case['n_vert'])
    rec.as_strided((F, 3, rec.stride(1)), (rec.stride(0), rec.stride(1), 1)).fill_(float('nan'))       # pads (and all) NaN ...
    rec.copy_(torch.from_numpy(case['meshes']))                                                          # ... then the fixture's meshes
    uv_tex = case['uv_tex'][0]
    ov, res = sim3dr.render_batch(m, case['img'], rec, alpha=0.6, uv_tex=uv_tex)
    ov, res = ov.cpu().numpy(), res.cpu().numpy()
    _check_pipeline(case, ov, res, tgold['full_overlay'], tc.demo_tex(case))
    abi.check(abi.lib().syn_debug_poison_workspace(m._h, 4, 0xFF))
    ov2, res2 = sim3dr.render_batch(m, case['img'], rec, alpha=0.6, uv_tex=uv_tex)
    assert np.array_equal(ov2.cpu().numpy(), ov) and np.array_equal(res2.cpu().numpy(), res)


def test_alternating_untextured_and_textured_on_one_handle(small):
    import torch
    from synergynet_amd import sim3dr
    case, m = small
    meshes = torch.from_numpy(case['meshes']).cuda()
    uv_tex = case['uv_tex'][0]
    plain = [x.cpu().numpy() for x in sim3dr.render_batch(m, case['img'], meshes, alpha=0.6)]
    texd = [x.cpu().numpy() for x in sim3dr.render_batch(m, case['img'], meshes, alpha=0.6, uv_tex=uv_tex)]
    assert not np.array_equal(plain[0], texd[0])
    before = list(m._topology_uploads)
    assert before[0] >= 1 and before[1] >= 1
    for _ in range(2):
        a = [x.cpu().numpy() for x in sim3dr.render_batch(m, case['img'], meshes, alpha=0.6)]
        b = [x.cpu().numpy() for x in sim3dr.render_batch(m, case['img'], meshes, alpha=0.6, uv_tex=uv_tex)]
        assert all(np.array_equal(x, y) for x, y in zip(a, plain)) and all(np.array_equal(x, y) for x, y in zip(b, texd))
    assert m._topology_uploads == before                                  # neither adjacency was uploaded again
    # stand-alone results on a fresh handle
    m2 = _model(case)
    t2 = [x.cpu().numpy() for x in sim3dr.render_batch(m2, case['img'], meshes, alpha=0.6, uv_tex=uv_tex)]
    assert all(np.array_equal(x, y) for x, y in zip(t2, texd)) and m2._topology_uploads == [0, 1]
    m3 = _model(case)
    p3 = [x.cpu().numpy() for x in sim3dr.render_batch(m3, case['img'], meshes, alpha=0.6)]
    assert all(np.array_equal(x, y) for x, y in zip(p3, plain)) and m3._topology_uploads == [1, 0]


def test_kept_vertex_without_triangle_is_nan_and_image_unaffected(small):
    """A kept vertex no kept triangle uses: NaN normal, light and colour, as in the reference; nothing draws it."""
    import torch
    from oracle import sim3dr as osim
    from synergynet_amd import sim3dr
    case, m0 = small
    m = _model(case)
    lone = int(np.setdiff1d(np.arange(case['n_vert']), case['keep'])[0])
    keep = np.concatenate([case['keep'], [lone]])                        # appended: the kept topology's indices stay valid
    case2 = dict(case, keep=keep, kept_meshes=np.ascontiguousarray(case['meshes'][:, :, keep]))
    tex = tc.demo_tex(case2)
    normal, light, colours, tex_after = _shade_kept(m, case2, tex, shared=True)
    assert np.isnan(normal[:, -1]).all() and np.isnan(light[:, -1]).all() and np.isnan(colours[:, -1]).all() and np.isnan(tex_after[-1]).all()
    assert not np.isnan(normal[:, :-1]).any()
    live = tc.oracle_render(case2, tex.copy(), impl='oracle')
    assert np.array_equal(normal, live['normal'], equal_nan=True)
    np.testing.assert_allclose(light, live['light'], rtol=0, atol=1e-6, equal_nan=True)
    np.testing.assert_allclose(colours, live['colours'], rtol=0, atol=1e-6, equal_nan=True)
    km = torch.from_numpy(case2['kept_meshes']).cuda()
    ov, _ = sim3dr._draw_and_blend(m, case['img'], km, torch.from_numpy(colours).cuda(), 1, 0.6)
    _close_images(ov.cpu().numpy(), live['overlay'])
    # the lone vertex changes the bounding box of norm_vertices at most; the image of the kept triangles is what the
    # rasteriser gives for these colours without it
    app_img = case['img'].copy()
    for f in range(case['n_faces']):
        app_img = osim.rasterize(np.ascontiguousarray(case2['kept_meshes'][f].T), case['tri_kept'], colours[f], bg=app_img)
    assert np.array_equal(ov.cpu().numpy(), app_img)


def test_texture_errors(small):
    import torch
    from synergynet_amd import sim3dr
    case, _ = small
    m = _model(case)
    lib, h = m._lib, m._h
    out = torch.empty((1, case['keep'].size, 3), device='cuda')
    u8 = torch.zeros((1, 256, 256, 3), dtype=torch.uint8, device='cuda')
    # before syn_load_uv_map
    assert lib.syn_select_topology(h, 1) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_uv_colors(h, u8.data_ptr(), 1, 256, 256, 3, 1, 1, out.data_ptr(), None) == abi.SYN_ERR_NOT_LOADED
    assert lib.syn_gather_vertices(h, out.data_ptr(), 1, 1, out.data_ptr(), None) == abi.SYN_ERR_NOT_LOADED
    m_no = _model(dict(case, assets={}))
    with pytest.raises(RuntimeError, match='Missing data'):
        sim3dr.render_batch(m_no, case['img'], torch.from_numpy(case['meshes']).cuda(), uv_tex=case['uv_tex'][0])
    # keep_ind / triangle / UV indices out of range
    cu, cv = np.ascontiguousarray(case['coord_u'], np.int32), np.ascontiguousarray(case['coord_v'], np.int32)
    keep, tri = np.ascontiguousarray(case['keep'], np.int32), case['tri_kept']
    bad = keep.copy(); bad[3] = case['n_vert']
    assert lib.syn_load_uv_map(h, _ptr(cu), _ptr(cv), cu.size, _ptr(bad), bad.size, _ptr(tri), tri.shape[0]) == abi.SYN_ERR_INVALID
    bad = keep.copy(); bad[0] = -1
    assert lib.syn_load_uv_map(h, _ptr(cu), _ptr(cv), cu.size, _ptr(bad), bad.size, _ptr(tri), tri.shape[0]) == abi.SYN_ERR_INVALID
    bad_t = tri.copy(); bad_t[5, 1] = keep.size
    assert lib.syn_load_uv_map(h, _ptr(cu), _ptr(cv), cu.size, _ptr(keep), keep.size, _ptr(bad_t), tri.shape[0]) == abi.SYN_ERR_INVALID
    bad_u = cu.copy(); bad_u[7] = -2
    assert lib.syn_load_uv_map(h, _ptr(bad_u), _ptr(cv), cu.size, _ptr(keep), keep.size, _ptr(tri), tri.shape[0]) == abi.SYN_ERR_INVALID
    assert lib.syn_select_topology(h, 1) == abi.SYN_ERR_NOT_LOADED        # nothing was loaded by the refused calls
    with pytest.raises(abi.SynergyHipError):
        sim3dr.render_batch(_model(dict(case, assets=dict(case['assets'], keep_ind=np.append(case['keep'], case['n_vert'])))), case['img'],
                            torch.from_numpy(case['meshes']).cuda(), uv_tex=case['uv_tex'][0])
    # a texture smaller than the table needs
    abi.check(_load_uv(m, case))
    need_h, need_w = int(case['coord_u'].max()) + 1, int(case['coord_v'].max()) + 1
    small_tex = torch.zeros((1, need_h - 1, need_w, 3), dtype=torch.uint8, device='cuda')
    out_all = torch.empty((1, case['n_vert'], 3), device='cuda')
    assert lib.syn_uv_colors(h, small_tex.data_ptr(), 1, need_h - 1, need_w, 3, 0, 0, out_all.data_ptr(), None) == abi.SYN_ERR_INVALID
    assert lib.syn_uv_colors(h, small_tex.data_ptr(), 1, need_w, need_w - 1, 3, 0, 0, out_all.data_ptr(), None) == abi.SYN_ERR_INVALID
    with pytest.raises(abi.SynergyHipError, match='smaller'):
        sim3dr.uv_vertex_colors(m, np.zeros((need_h - 1, need_w, 3), np.uint8), kept=False)
    exact = torch.zeros((1, need_h, need_w, 3), dtype=torch.uint8, device='cuda')
    assert lib.syn_uv_colors(h, exact.data_ptr(), 1, need_h, need_w, 3, 0, 0, out_all.data_ptr(), None) == 0
    # a tex of the wrong length / type
    meshes = torch.from_numpy(case['meshes']).cuda()
    with pytest.raises(ValueError, match='one colour per vertex'):
        sim3dr.render_batch(m, case['img'], meshes, tex=np.zeros((case['keep'].size - 1, 3), np.float32))
    with pytest.raises(ValueError, match='one colour per vertex'):
        sim3dr.render_batch(m, case['img'], meshes, tex=np.zeros((case['n_faces'] + 1, case['keep'].size, 3), np.float32))
    with pytest.raises(TypeError):
        sim3dr.render_batch(m, case['img'], meshes, tex=np.zeros((case['keep'].size, 3), np.float64))
    from synergynet_amd import inference
    inference.set_default_model(m)
    with pytest.raises(ValueError, match='one colour per vertex'):
        sim3dr.render(case['img'], [case['kept_meshes'][0]], tex=np.zeros((5, 3), np.float32), connectivity=case['assets']['tri_deletion'] - 1)
    with pytest.raises(ValueError):
        sim3dr.gather_kept(m, meshes[:, :, :-1].contiguous())
    torch.cuda.synchronize()
