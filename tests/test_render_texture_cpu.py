"""CPU-side tests of per-pixel texture mapping (no GPU): the order-free numpy statement the GPU tests lean on
(tests/render_texture_cases.texture_rule) against the fixture the reference's own compiled `_render_texture_core` produced
(tests/golden/render_texture_golden.npz, written by tests/golden/make_render_texture_golden.py) and, where oracle/_ref exists, against
that function live on fresh seeds; the texture coordinates of the UV asset; header / ctypes table / library agreeing on the two new
entry points."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import render_texture_cases as rc
import visibility_cases as vc
from conftest import ROOT

NEW_SYMBOLS = ('syn_load_tex_coords', 'syn_render_texture')


@pytest.fixture(scope='module')
def tgold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'render_texture_golden.npz')))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()          # bytes: the sign of zero counts


def test_new_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import build_library
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    for s in NEW_SYMBOLS:
        assert s in abi.EXPORTED_SYMBOLS and hasattr(l, s), s
        decl = re.search(r'\bint ' + s + r'\(([^;]*)\);', hdr)
        assert decl, s
        assert len(decl.group(1).split(',')) == len(abi._SIGS[s][1]), s         # the header's argument count
    l.syn_abi_version.restype = ctypes.c_int
    assert l.syn_abi_version() == 1
    import Sim3DR
    from synergynet_amd import sim3dr
    assert Sim3DR.render_texture_core is sim3dr.render_texture_core
    assert callable(sim3dr.render_texture_batch) and callable(sim3dr.uv_tex_coords)


def test_fixture_is_small_and_holds_data_only(tgold):
    path = os.path.join(ROOT, 'tests', 'golden', 'render_texture_golden.npz')
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'render_golden.npz'))
    assert all(v.dtype.kind in 'iuf' for v in tgold.values())


def test_soup_rule_reproduces_the_reference_byte_for_byte(tgold):
    seed, hw, ntri, tex_seed = (int(x) for x in tgold['soup_cfg'])
    case = rc.build_soup_case(seed, hw, ntri, tex_seed)
    x, y = case['tex_coords'][:, 0], case['tex_coords'][:, 1]
    th, tw, _ = case['texture'].shape
    assert (x < 0).any() and (x > tw - 1).any() and (y < 0).any() and (y > th - 1).any()      # outside the texture on every side
    assert (case['tex_coords'][:, :2] == np.rint(case['tex_coords'][:, :2])).all(1).mean() > 0.3
    for c, mt in rc.SOUP_VARIANTS:
        image, depth = rc.soup_image(case, c), case['depth'].copy()
        rc.texture_rule(image, depth, case['vertices'], case['triangles'], case['texture'], case['tex_coords'], case['tex_triangles'], mt)
        assert _same(depth, tgold['soup_depth']) and _same(image, tgold[f'soup_image_c{c}_m{mt}']), (c, mt)
    won = depth.view(np.uint32) != case['depth'].view(np.uint32)
    # the same walk without the border rule (the visibility fixture): where its depth differs, the winner does not contain the pixel
    border_only = won & (depth.view(np.uint32) != np.load(os.path.join(ROOT, 'tests', 'golden', 'visibility_golden.npz'))['soup_depth'].view(np.uint32))
    ring = np.ones((hw, hw), bool)
    ring[2:-2, 2:-2] = False
    print('soup: won', int(won.sum()), 'border only', int(border_only.sum()))
    assert won.sum() > 2000 and border_only.sum() > 200 and not (border_only & ~ring).any()
    assert ((depth == 0) & np.signbit(depth) & won).any() and ((depth == 0) & ~np.signbit(depth) & won).any()
    assert (image[~won] == rc.SOUP_FILL).all() and _same(depth[~won], case['depth'][~won])      # untouched pixels keep the caller's values
    # the index quirk is pinned: with tex_triangles == triangles the picture differs
    image2, depth2 = rc.soup_image(case, 1), case['depth'].copy()
    rc.texture_rule(image2, depth2, case['vertices'], case['triangles'], case['texture'], case['tex_coords'], case['triangles'], rc.BILINEAR)
    assert _same(depth2, depth) and not _same(image2, image)


def test_small_rule_reproduces_the_reference_per_face_and_shared(tgold):
    case = vc.build_mesh_case(tgold['small_cfg'])
    hw, tri = case['hw'], case['tri_full']
    for name, (meshes, tex, coords, c, mt, shared) in rc.small_variants(case).items():
        ver = rc.interleaved(meshes)
        image, depth = rc.fresh(hw, hw, c, lead=() if shared else (2,))
        if shared:
            rc.rule_shared(image, depth, ver, tri, tex, coords, tri, mt)
        else:
            for f in range(2):
                rc.texture_rule(image[f], depth[f], ver[f], tri, tex, coords, tri, mt)
        assert _same(image, tgold[f'small_{name}_image']) and _same(depth, tgold[f'small_{name}_depth']), name
    # one z-buffer: the result depends on depth, not on the order of the faces (no two faces tie at a pixel here) ...
    assert _same(tgold['small_shared256_image'], tgold['small_shared256_swapped_image'])
    assert _same(tgold['small_shared256_depth'], tgold['small_shared256_swapped_depth'])
    # ... and both faces are in the picture: it is neither face's own
    pair = rc.overlapping_pair(case['meshes'])
    own = [rc.fresh(hw, hw, 3) for _ in range(2)]
    for f in range(2):
        rc.texture_rule(own[f][0], own[f][1], rc.interleaved(pair)[f], tri, *rc.small_variants(case)['shared256'][1:3], tri, rc.BILINEAR)
    sh = tgold['small_shared256_depth']
    from0, from1 = (sh == own[0][1]) & (sh != rc.INIT_DEPTH), (sh == own[1][1]) & (sh != rc.INIT_DEPTH)
    assert from0.sum() > 500 and from1.sum() > 500 and ((own[0][1] != rc.INIT_DEPTH) & (own[1][1] != rc.INIT_DEPTH)).sum() > 500
    assert _same(sh, np.maximum(own[0][1], own[1][1]))


def test_equal_depths_between_faces_go_to_the_earlier_face():
    """Two identical meshes with different textures in one z-buffer: the first face keeps every pixel."""
    from synergynet_amd import synth
    tri = synth.make_grid_topology(6, 7)
    mesh = synth.make_face_meshes(1, 6, 7, height=24, width=24, seed=3)
    ver = rc.interleaved(np.concatenate([mesh, mesh]))
    coords = np.ascontiguousarray(np.random.default_rng(1).uniform(0, 7, (42, 3)), dtype=np.float32)
    tex = rc.byte_texture(9, 8, 8).astype(np.float32)
    image, depth = rc.fresh(24, 24, 3)
    rc.rule_shared(image, depth, ver, tri, tex, coords, tri, rc.NEAREST)
    one = rc.fresh(24, 24, 3)
    rc.texture_rule(one[0], one[1], ver[0], tri, tex, coords, tri, rc.NEAREST)
    assert _same(image, one[0]) and _same(depth, one[1]) and (depth != rc.INIT_DEPTH).sum() > 50


def test_uv_tex_coords_is_the_continuous_counterpart_of_uv_pixel_coords():
    from synergynet_amd import params, sim3dr, synth
    assets = synth.make_uv_assets(40 * 44, 40, 44, seed=31)
    stub = types.SimpleNamespace(param_pack=types.SimpleNamespace(uv_vert=assets['uv_vert'], keep_ind=assets['keep_ind']))
    tc = sim3dr.uv_tex_coords(stub, 256, 256)
    cu, cv = params.uv_pixel_coords(assets['uv_vert'])
    assert tc.dtype == np.float32 and tc.shape == (40 * 44, 3) and tc.flags.c_contiguous and (tc[:, 2] == 0).all()
    # uv_colors_kernel reads row tex_h-1-coord_u, column coord_v: within one texel of the continuous coordinate
    assert np.abs(tc[:, 0] - cv).max() < 1 and np.abs(tc[:, 1] - (255 - cu)).max() < 1
    assert (tc[:, 0] >= cv).all() and (tc[:, 1] <= 255 - cu).all()                      # the integer tables truncate
    kept = sim3dr.uv_tex_coords(stub, 64, 48, kept=True)
    assert _same(kept, sim3dr.uv_tex_coords(stub, 64, 48)[assets['keep_ind']]) and kept[:, 0].max() <= 47 and kept[:, 1].max() <= 63


@pytest.mark.skipif(not vc.ref_available(), reason='oracle/_ref (the reference compiled where it lies) is not on this machine')
@pytest.mark.parametrize('seed', [21, 22, 23])
def test_rule_against_the_reference_function_on_fresh_seeds(seed):
    hw = 40 + seed
    case = rc.build_soup_case(seed, hw, 300, tex_seed=seed + 100)
    for c, mt in ((3, rc.BILINEAR), (2, rc.NEAREST)):
        ref = (rc.soup_image(case, c), case['depth'].copy())
        mine = (rc.soup_image(case, c), case['depth'].copy())
        args = (case['vertices'], case['triangles'], case['texture'], case['tex_coords'], case['tex_triangles'])
        rc.ref_render_texture(ref[0], *args, ref[1], hw, hw, c, mt)
        rc.texture_rule(mine[0], mine[1], *args, mt)
        assert (ref[1] != case['depth']).sum() > 500
        assert _same(mine[0], ref[0]) and _same(mine[1], ref[1])


@pytest.mark.skipif(not vc.ref_available(), reason='oracle/_ref (the reference compiled where it lies) is not on this machine')
def test_fixture_arrays_are_the_reference_functions(tgold):
    seed, hw, ntri, tex_seed = (int(x) for x in tgold['soup_cfg'])
    case = rc.build_soup_case(seed, hw, ntri, tex_seed)
    image, depth = rc.soup_image(case, 3), case['depth'].copy()
    rc.ref_render_texture(image, case['vertices'], case['triangles'], case['texture'], case['tex_coords'], case['tex_triangles'], depth, hw, hw,
                          3, rc.BILINEAR)
    assert _same(image, tgold['soup_image_c3_m1']) and _same(depth, tgold['soup_depth'])
    full = vc.build_mesh_case(tgold['full_cfg'])
    tex = rc.byte_texture(rc.SMALL_TEX_SEED + 2, rc.FULL_TEX_HW, rc.FULL_TEX_HW).astype(np.float32)
    coords = rc.uv_coords(full['assets'], rc.FULL_TEX_HW, rc.FULL_TEX_HW)
    image, depth = rc.ref_per_face(full['meshes'], full['tri_full'], tex, coords, full['hw'], full['hw'], 3, rc.BILINEAR)
    assert np.array_equal(vc.sha(image), tgold['full_image_sha256']) and np.array_equal(vc.sha(depth), tgold['full_depth_sha256'])
    assert np.array_equal((depth != rc.INIT_DEPTH).reshape(2, -1).sum(1), tgold['full_pixel_count'])
