"""GPU parity of per-pixel texture mapping through the C ABI (syn_load_tex_coords / syn_render_texture) and the Python entries built
on it (Sim3DR.render_texture_core, sim3dr.render_texture_batch, sim3dr.uv_tex_coords), against the fixture the reference's own compiled
`_render_texture_core` produced (tests/golden/render_texture_golden.npz; tests/test_render_texture_cpu.py pins the numpy statement
tests/render_texture_cases.texture_rule to it and to the live function).

Bar: image and depth BIT-identical (compared as bytes, so the sign of zero counts) for float32 textures and images; a uint8 texture
equals the float32 texture of the same values; a uint8 image equals uint8(clip(rint(float result), 0, 255)) exactly.  Every step runs
once."""
import ctypes as C
import os

import numpy as np
import pytest

import render_texture_cases as rc
import visibility_cases as vc
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = [getattr(abi, '_SIGS')[s] for s in ('syn_load_tex_coords', 'syn_render_texture')]        # KeyError without the feature


@pytest.fixture(scope='module')
def tgold():
    return dict(np.load(os.path.join(HERE, 'golden', 'render_texture_golden.npz')))


@pytest.fixture(scope='module')
def small(tgold):
    case = vc.build_mesh_case(tgold['small_cfg'])
    return case, vc.model_for(case), rc.small_variants(case)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _pitched(meshes_np):
    """[F,3,pitch][:, :, :n] with NaN in the pad columns, like the tensor reconstruct() returns."""
    import torch
    F, _, n = meshes_np.shape
    store = torch.full((F, 3, (n + 127) // 128 * 128 + 128), float('nan'), device='cuda')
    view = store[:, :, :n]
    view.copy_(torch.from_numpy(meshes_np))
    assert not view.is_contiguous()
    return view


def _to_u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _render(m, verts_t, F, planar, texture, mt, image, depth, shared, expect=0):
    """syn_render_texture on copies of the caller's numpy image / depth (float32 or uint8 image, float32 or uint8 texture [T,..])."""
    import torch
    tex = torch.from_numpy(np.ascontiguousarray(texture)).cuda()
    img, dep = torch.from_numpy(np.ascontiguousarray(image)).cuda(), torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    T, th, tw, tc = tex.shape
    H, W, c = image.shape[-3:]
    rc_ = m._lib.syn_render_texture(m._h, verts_t.data_ptr(), F, planar, tex.data_ptr(), int(tex.dtype == torch.uint8), T, th, tw, tc, mt,
                                    img.data_ptr(), int(img.dtype == torch.uint8), dep.data_ptr(), H, W, c, int(shared), m._stream())
    assert rc_ == expect, (rc_, expect)
    return img.cpu().numpy(), dep.cpu().numpy()


def test_soup_bit_identical_from_interleaved_packed_and_pitched_input(small, tgold):
    """The border rule, zero-area, duplicate, equal-depth, +0 / -0, NaN-corner and off-frame triangles, a non-default initial depth, a
    pre-filled image, coordinates outside the texture, tex_triangles that differ from the triangles."""
    import torch
    seed, hw, ntri, tex_seed = (int(x) for x in tgold['soup_cfg'])
    case = rc.build_soup_case(seed, hw, ntri, tex_seed)
    ver, tri = case['vertices'], case['triangles']
    m = vc.model_for(small[0])                                            # a handle of its own: the soup replaces its topology
    abi.check(m._lib.syn_load_triangles(m._h, _ptr(tri), ntri, ver.shape[0]))
    abi.check(m._lib.syn_load_tex_coords(m._h, _ptr(case['tex_coords']), case['tex_coords'].shape[0], _ptr(case['tex_triangles'])))
    planar_np = np.ascontiguousarray(ver.T)[None]
    pitched = _pitched(planar_np)
    layouts = (('interleaved', torch.from_numpy(ver[None]).cuda(), 0), ('packed', torch.from_numpy(planar_np).cuda(), 1),
               ('pitched', pitched, pitched.stride(1)))
    won = tgold['soup_depth'].view(np.uint32) != case['depth'].view(np.uint32)
    assert won.sum() > 2000 and (~won).sum() > 500
    for c, mt in rc.SOUP_VARIANTS:
        want = tgold[f'soup_image_c{c}_m{mt}']
        for name, vt, planar in layouts:
            img, dep = _render(m, vt, 1, planar, case['texture'][None], mt, rc.soup_image(case, c), case['depth'], 1)
            print('soup', name, 'c', c, 'mapping', mt, 'differing elements', int((img.view(np.uint32) != want.view(np.uint32)).sum()),
                  int((dep.view(np.uint32) != tgold['soup_depth'].view(np.uint32)).sum()))
            assert _same(img, want) and _same(dep, tgold['soup_depth']), (name, c, mt)
        assert (img[~won] == rc.SOUP_FILL).all() and _same(dep[~won], case['depth'][~won])        # untouched pixels keep the caller's values
        # shared = 0 with one face is the same thing
        img0, dep0 = _render(m, layouts[1][1], 1, 1, case['texture'][None], mt, rc.soup_image(case, c)[None], case['depth'][None], 0)
        assert _same(img0[0], want) and _same(dep0[0], tgold['soup_depth'])
        # a uint8 texture is read as (float)byte: the rule on the rounded texture, which the float path reproduces too
        tex8 = _to_u8(case['texture'])
        want8 = (rc.soup_image(case, c), case['depth'].copy())
        rc.texture_rule(want8[0], want8[1], ver, tri, tex8, case['tex_coords'], case['tex_triangles'], mt)
        for tex in (tex8, tex8.astype(np.float32)):
            img8, dep8 = _render(m, layouts[2][1], 1, layouts[2][2], tex[None], mt, rc.soup_image(case, c), case['depth'], 1)
            assert _same(img8, want8[0]) and _same(dep8, want8[1]) and not _same(img8, want)


def test_small_per_face_and_shared_both_orders_and_uint8_image(small, tgold):
    import torch
    from synergynet_amd import sim3dr
    case, m, variants = small
    hw = case['hw']
    sim3dr._texc_keys(m)
    before = list(m._tex_coord_uploads)
    for name, (meshes, tex, coords, c, mt, shared) in variants.items():
        want_i, want_d = tgold[f'small_{name}_image'], tgold[f'small_{name}_depth']
        th = tex.shape[0]
        mapping = 'bilinear' if mt == rc.BILINEAR else 'nearest'
        for layout, mesh_t in (('packed', torch.from_numpy(meshes).cuda()), ('pitched', _pitched(meshes))):
            bg = np.zeros((hw, hw, c), np.float32)
            img, dep = sim3dr.render_texture_batch(m, mesh_t, tex, background=bg, mapping=mapping, shared=shared)
            img, dep = img.cpu().numpy(), dep.cpu().numpy()
            print('small', name, layout, 'differing elements', int((img.view(np.uint32) != want_i.view(np.uint32)).sum()),
                  int((dep.view(np.uint32) != want_d.view(np.uint32)).sum()))
            assert _same(img, want_i) and _same(dep, want_d), (name, layout)
        assert _same(sim3dr.uv_tex_coords(m, th, th), coords)
        # uint8 texture (what texture_from_image produces) and a uint8 image: uint8(clip(rint(float result)))
        tex8 = tex.astype(np.uint8)
        assert _same(tex8.astype(np.float32), tex)
        img8, dep8 = sim3dr.render_texture_batch(m, mesh_t, torch.from_numpy(tex8).cuda(), background=np.zeros((hw, hw, c), np.uint8),
                                                 mapping=mapping, shared=shared)
        assert img8.dtype == torch.uint8 and _same(img8.cpu().numpy(), _to_u8(want_i)) and _same(dep8.cpu().numpy(), want_d)
    # the default image: zeros float32 with the texture's channels; one texture per face
    meshes, tex, coords, c, mt, _ = variants['faces64']
    img, dep = sim3dr.render_texture_batch(m, torch.from_numpy(meshes).cuda(), np.stack([tex, tex[::-1]]), hw, hw, shared=False)
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, hw, hw, 3) and _same(img[0].cpu().numpy(), tgold['small_faces64_image'][0])
    assert not _same(img[1].cpu().numpy(), tgold['small_faces64_image'][1]) and _same(dep.cpu().numpy(), tgold['small_faces64_depth'])
    sizes = [v[1].shape[0] for v in variants.values()] + [64]
    changes = sum(a != b for a, b in zip(sizes, sizes[1:])) + 1          # uploaded when the texture size changes, not per call
    assert changes < len(sizes) and m._tex_coord_uploads[0] - before[0] in (changes - 1, changes) and m._tex_coord_uploads[1] == before[1]


def test_binding_signature_updates_numpy_arrays_in_place(small, tgold):
    import Sim3DR
    from synergynet_amd import inference
    seed, hw, ntri, tex_seed = (int(x) for x in tgold['soup_cfg'])
    case = rc.build_soup_case(seed, hw, ntri, tex_seed)
    m = vc.model_for(small[0])
    inference.set_default_model(m)
    th, tw, tc = case['texture'].shape
    for c, mt in rc.SOUP_VARIANTS[1:3]:
        image, depth = rc.soup_image(case, c), case['depth'].copy()
        assert Sim3DR.render_texture_core(image, case['vertices'], case['triangles'], case['texture'], case['tex_coords'],
                                          case['tex_triangles'], depth, case['vertices'].shape[0], case['tex_coords'].shape[0], ntri, hw,
                                          hw, c, th, tw, tc, mt) is None
        assert _same(image, tgold[f'soup_image_c{c}_m{mt}']) and _same(depth, tgold['soup_depth'])
    assert m._tex_coord_uploads == [1, 0] and m._topology_uploads[0] == 1


def test_texture_from_image_to_per_pixel_render_over_a_second_frame(small):
    """texture_from_image(fill=True) -> render_texture_batch against the CPU pipeline (texture_rule on the downloaded texture)."""
    import torch
    from synergynet_amd import sim3dr
    case, m, _ = small
    hw = case['hw']
    meshes = torch.from_numpy(case['meshes']).cuda()
    tex, mask = sim3dr.texture_from_image(m, case['img'], meshes, tex_hw=256, fill=True)
    assert tex.dtype == torch.uint8 and tuple(tex.shape) == (2, 256, 256, 3)
    other = np.random.default_rng(78).integers(0, 256, case['img'].shape, dtype=np.uint8)
    pair = rc.overlapping_pair(case['meshes'])
    img, dep = sim3dr.render_texture_batch(m, torch.from_numpy(pair).cuda(), tex, background=other, shared=True)
    coords, tri, tex_np = rc.uv_coords(case['assets'], 256, 256), case['tri_full'], tex.cpu().numpy()
    want_i, want_d = other.astype(np.float32), np.full((hw, hw), rc.INIT_DEPTH, np.float32)
    state = None
    for f in (1, 0):                                                      # one z-buffer, a texture per face
        state = rc.texture_rule(want_i, want_d, rc.interleaved(pair)[f], tri, tex_np[f], coords, tri, rc.BILINEAR, state)
    diff = int((img.cpu().numpy() != _to_u8(want_i)).sum())
    print('photograph -> texture -> per-pixel render: differing image elements', diff, 'pixels drawn', int(state[1].sum()))
    assert diff == 0 and _same(dep.cpu().numpy(), want_d) and state[1].sum() > 5000
    assert (img.cpu().numpy()[~state[1]] == other[~state[1]]).all()
    res = torch.empty_like(img)                                           # and straight into the blend
    abi.check(m._lib.syn_add_weighted(m._h, torch.from_numpy(other).cuda().data_ptr(), C.c_float(0.4), img.data_ptr(), C.c_float(0.6),
                                      res.data_ptr(), img.numel(), m._stream()))
    assert (res.cpu().numpy()[~state[1]] == other[~state[1]]).all()


def test_full_size_pitched_300_faces_poison_and_alternation(tgold):
    import torch
    from synergynet_amd import sim3dr, synth
    case = vc.build_mesh_case(tgold['full_cfg'])
    m = vc.model_for(case)
    F, hw = case['n_faces'], case['hw']
    rec = m.reconstruct(torch.from_numpy(synth.make_params(F)).cuda(), roi=torch.from_numpy(synth.make_rois(F)).cuda(), dense=True)
    assert not rec.is_contiguous() and rec.shape == (F, 3, case['n_vert'])
    rec.as_strided((F, 3, rec.stride(1)), (rec.stride(0), rec.stride(1), 1)).fill_(float('nan'))
    rec.copy_(torch.from_numpy(case['meshes']))
    tex = torch.from_numpy(rc.byte_texture(rc.SMALL_TEX_SEED + 2, rc.FULL_TEX_HW, rc.FULL_TEX_HW)).cuda()

    def run():
        return [x.cpu().numpy() for x in sim3dr.render_texture_batch(m, rec, tex, hw, hw, shared=False)]

    img, dep = run()
    print('full: pixels drawn', (dep != rc.INIT_DEPTH).reshape(F, -1).sum(1))
    assert np.array_equal((dep != rc.INIT_DEPTH).reshape(F, -1).sum(1), tgold['full_pixel_count'])
    assert np.array_equal(vc.sha(img), tgold['full_image_sha256']) and np.array_equal(vc.sha(dep), tgold['full_depth_sha256'])
    uploads, tcu = list(m._topology_uploads), list(m._tex_coord_uploads)
    abi.check(abi.lib().syn_debug_poison_workspace(m._h, 4, 0xFF))
    assert all(_same(a, b) for a, b in zip(run(), (img, dep)))
    # 300 faces, each in its own planes, in one call (64 x 64 frame)
    few = rc.scaled(case['meshes'], hw, rc.FULL_SMALL_FRAME)
    many = torch.from_numpy(np.ascontiguousarray(np.tile(few, (150, 1, 1)))).cuda()
    i300, d300 = (x.cpu().numpy() for x in sim3dr.render_texture_batch(m, many, tex, rc.FULL_SMALL_FRAME, rc.FULL_SMALL_FRAME, shared=False))
    assert i300.shape[0] == 300 and np.array_equal(vc.sha(i300[:2]), tgold['full_image64_sha256'])
    assert np.array_equal(vc.sha(d300[:2]), tgold['full_depth64_sha256'])
    assert _same(i300, np.tile(i300[:2], (150, 1, 1, 1))) and _same(d300, np.tile(d300[:2], (150, 1, 1)))
    # alternating with syn_rasterize, syn_rasterize_triangles and the kept topology (all share the key scratch)
    frame = np.random.default_rng(3).integers(0, 256, (hw, hw, 3), dtype=np.uint8)
    sim3dr.render_batch(m, frame, rec)
    sim3dr.visibility_batch(m, rec, hw, hw)
    sim3dr.render_batch(m, frame, rec, uv_tex=tex)                        # leaves the kept topology selected
    kept_i, kept_d = sim3dr.render_texture_batch(m, rec, tex, hw, hw, shared=False, kept=True)
    assert 0 < int((kept_d != rc.INIT_DEPTH).sum()) < int((torch.from_numpy(dep) != rc.INIT_DEPTH).sum())
    assert all(_same(a, b) for a, b in zip(run(), (img, dep)))
    assert m._topology_uploads == [uploads[0], uploads[1] + (0 if uploads[1] else 1)] and m._tex_coord_uploads == [tcu[0], tcu[1] + 1]
    sim3dr.render_texture_batch(m, rec, tex, hw, hw, shared=False, kept=True)
    assert m._tex_coord_uploads == [tcu[0], tcu[1] + 1]
    # 65535 faces of either topology do not fit the 32-bit index field of the key.  The limit is judged on the SELECTED topology, so the
    # full one is selected first and the product is checked for both here: a call that were not refused would walk 65535 meshes
    n_kept_tri = case['assets']['tri_deletion'].shape[1]
    assert min(case['tri_full'].shape[0], n_kept_tri) * 65535 >= 1 << 32
    abi.check(m._lib.syn_select_topology(m._h, 0))
    z = torch.zeros(8, device='cuda')
    assert m._lib.syn_render_texture(m._h, rec.data_ptr(), 65535, rec.stride(1), tex.data_ptr(), 1, 1, 256, 256, 3, 1, z.data_ptr(), 0,
                                     z.data_ptr(), 1, 1, 3, 1, None) == abi.SYN_ERR_INVALID


def test_nan_texture_coordinate_samples_coordinate_zero(small):
    """The defined safe path (the reference converts NaN to int there): compared with texture_rule only."""
    import torch
    from synergynet_amd import synth
    case = small[0]
    m = vc.model_for(case)
    tri = synth.make_grid_topology(6, 7)
    mesh = synth.make_face_meshes(1, 6, 7, height=40, width=40, seed=4)
    coords = np.ascontiguousarray(np.random.default_rng(2).uniform(1, 10, (42, 3)), dtype=np.float32)
    clean = coords.copy()
    coords[tri[20, 0], 0], coords[tri[31, 1], 1] = np.nan, np.nan         # x of one triangle's corner, y of another's
    tex = rc.byte_texture(11, 12, 12).astype(np.float32)
    abi.check(m._lib.syn_load_triangles(m._h, _ptr(tri), tri.shape[0], 42))
    got = {}
    for name, tcs in (('nan', coords), ('clean', clean)):
        abi.check(m._lib.syn_load_tex_coords(m._h, _ptr(tcs), 42, None))
        for mt in (rc.NEAREST, rc.BILINEAR):
            want = rc.fresh(40, 40, 3)
            rc.texture_rule(want[0], want[1], rc.interleaved(mesh)[0], tri, tex, tcs, tri, mt)
            img, dep = _render(m, torch.from_numpy(mesh).cuda(), 1, 1, tex[None], mt, *rc.fresh(40, 40, 3), 1)
            assert _same(img, want[0]) and _same(dep, want[1]) and np.isfinite(img).all()
            got[name, mt] = img, dep
    for mt in (rc.NEAREST, rc.BILINEAR):
        changed = (got['nan', mt][0] != got['clean', mt][0]).any(2)
        drawn = got['clean', mt][1] != rc.INIT_DEPTH
        assert _same(got['nan', mt][1], got['clean', mt][1])
        assert 0 < changed.sum() < drawn.sum() / 2 and not (changed & ~drawn).any()      # the triangles around the two corners only


def test_render_texture_errors_leave_image_and_depth_untouched(small):
    import torch
    case = small[0]
    m = vc.model_for(case)
    lib, h = m._lib, m._h
    n, tri = case['n_vert'], case['tri_full']
    v = torch.from_numpy(case['meshes']).cuda()
    tex = np.zeros((2, 8, 8, 3), np.float32)
    image, depth = np.full((2, 16, 16, 3), 7, np.float32), np.full((2, 16, 16), -3, np.float32)
    coords = np.zeros((n, 3), np.float32)

    def refused(expect, F=2, texture=tex, mt=1, img=image, shared=0, T=None):
        t = texture if T is None else texture[:1].repeat(T, 0)
        i, d = _render(m, v, F, 1, t, mt, img, depth, shared, expect=expect)
        assert _same(i, img) and _same(d, depth)

    refused(abi.SYN_ERR_NOT_LOADED)                                       # no topology
    assert lib.syn_load_tex_coords(h, _ptr(coords), n, None) == abi.SYN_ERR_NOT_LOADED
    abi.check(lib.syn_load_triangles(h, _ptr(tri), tri.shape[0], n))
    refused(abi.SYN_ERR_NOT_LOADED)                                       # no texture coordinates
    bad = tri.copy()
    bad[5, 1] = n
    assert lib.syn_load_tex_coords(h, _ptr(coords), n, _ptr(bad)) == abi.SYN_ERR_INVALID          # a tex_triangles index out of range
    bad[5, 1] = -1
    assert lib.syn_load_tex_coords(h, _ptr(coords), n, _ptr(bad)) == abi.SYN_ERR_INVALID
    assert lib.syn_load_tex_coords(h, _ptr(coords), int(tri.max()), _ptr(np.zeros_like(tri))) == abi.SYN_ERR_INVALID   # a mesh index >= tex_nver
    assert lib.syn_load_tex_coords(h, None, n, None) == abi.SYN_ERR_INVALID
    refused(abi.SYN_ERR_NOT_LOADED)                                       # the refused loads stored nothing
    abi.check(lib.syn_load_tex_coords(h, _ptr(coords), n, None))
    refused(abi.SYN_ERR_INVALID, img=np.full((2, 16, 16, 4), 7, np.float32))                      # c > tex_c
    refused(abi.SYN_ERR_INVALID, T=3)                                     # T outside {1, F}
    refused(abi.SYN_ERR_INVALID, mt=2)
    refused(abi.SYN_ERR_INVALID, mt=-1)
    z = torch.zeros(8, device='cuda')
    assert lib.syn_render_texture(h, v.data_ptr(), 2, 1, None, 0, 1, 8, 8, 3, 1, z.data_ptr(), 0, z.data_ptr(), 1, 1, 3, 0, None) == abi.SYN_ERR_INVALID
    assert lib.syn_render_texture(h, v.data_ptr(), 1 << 11, 1, z.data_ptr(), 0, 1, 8, 8, 3, 1, z.data_ptr(), 0, z.data_ptr(), 1 << 10, 1 << 10, 3, 0,
                                  None) == abi.SYN_ERR_INVALID            # F*H*W >= 2^31
    abi.check(lib.syn_load_triangles(h, _ptr(tri), tri.shape[0], n))      # replacing the topology drops the slot's coordinates
    refused(abi.SYN_ERR_NOT_LOADED)
    torch.cuda.synchronize()
