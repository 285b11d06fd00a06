"""CPU-side tests of the visibility-buffer feature (no GPU): the definitions the GPU tests compare against
(tests/visibility_cases.py) against the fixture the reference's own compiled `_rasterize_triangles` produced
(tests/golden/visibility_golden.npz, written by tests/golden/make_visibility_golden.py), the order-free winner rule against that
function's buffers (fixture, and live on fresh seeds where oracle/_ref exists), and header / ctypes table / library agreeing on the
four new entry points."""
import ctypes
import os

import numpy as np
import pytest

import visibility_cases as vc
from conftest import ROOT

NEW_SYMBOLS = ('syn_rasterize_triangles', 'syn_vertex_visibility', 'syn_sample_vertex_colors', 'syn_uv_scatter')


@pytest.fixture(scope='module')
def vgold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'visibility_golden.npz')))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()          # bytes: the sign of zero counts


def test_new_symbols_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import build_library
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    for s in NEW_SYMBOLS:
        assert s + '(' in hdr and s in abi.EXPORTED_SYMBOLS and hasattr(l, s), s
    l.syn_abi_version.restype = ctypes.c_int
    assert l.syn_abi_version() == 1
    import Sim3DR
    from synergynet_amd import sim3dr
    assert Sim3DR.rasterize_triangles is sim3dr.rasterize_triangles
    for name in ('visibility_batch', 'vertex_colors_from_image', 'texture_from_image'):
        assert callable(getattr(sim3dr, name))


def test_fixture_is_small_and_holds_data_only(vgold):
    path = os.path.join(ROOT, 'tests', 'golden', 'visibility_golden.npz')
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'render_golden.npz'))
    assert all(v.dtype.kind in 'iuf' for v in vgold.values())


def test_soup_holds_every_special_case_and_the_winner_rule_reproduces_the_reference(vgold):
    seed, hw, ntri = (int(x) for x in vgold['soup_cfg'])
    ver, tri, (depth, tb, bw) = vc.build_soup(seed, hw, ntri)
    init = (depth.copy(), tb.copy(), bw.copy())
    p = ver[tri]                                                        # [ntri,3,3]
    area2 = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])
    assert (area2 == 0).sum() >= 2 and np.isnan(p[:, :, 0]).any() and np.isnan(p[:, :, 2]).any()
    assert np.unique(np.nan_to_num(p.reshape(ntri, 9)), axis=0).shape[0] < ntri                       # duplicates
    assert (np.nanmax(p[:, :, 0], 1) < 0).any() and (np.nanmin(p[:, :, 0], 1) > hw - 1).any()          # off the frame
    assert ((p[:, :, :2] == np.rint(p[:, :, :2])).all((1, 2))).sum() > ntri // 4                       # corners exactly on pixels
    zero = (p[:, :, 2] == 0).all(1)
    assert (zero & np.signbit(p[:, :, 2]).all(1)).any() and (zero & ~np.signbit(p[:, :, 2]).any(1)).any()
    vc.winner_rule(ver, tri, depth, tb, bw, hw, hw)
    assert _same(depth, vgold['soup_depth']) and _same(tb, vgold['soup_tri']) and _same(bw, vgold['soup_bary'])
    won = tb != init[1]
    assert 0.3 < won.mean() < 0.95                                      # winners and untouched pixels both
    assert _same(depth[~won], init[0][~won]) and _same(bw[~won], init[2][~won])                       # untouched keep the caller's values
    assert (tb[:, hw // 2:] == -7).any() and (depth[:, hw // 2:][tb[:, hw // 2:] >= 0] > 0.5).all()   # the plane hides what is behind it
    # +0 / -0: between two planes of equal depth over the same pixels the EARLIER triangle wins and its own sign is stored
    z = np.flatnonzero(zero & (area2 != 0))
    pairs = [(a, b) for a in z for b in z if a < b and np.array_equal(p[a, :, :2], p[b, :, :2]) and
             np.signbit(p[a, 0, 2]) != np.signbit(p[b, 0, 2])]
    assert len(pairs) >= 2 and {bool(np.signbit(p[a, 0, 2])) for a, _ in pairs} == {True, False}
    for a, b in pairs:
        assert (tb == a).any() and not (tb == b).any()
        assert (np.signbit(depth[tb == a]) == np.signbit(p[a, 0, 2])).all() and (depth[tb == a] == 0).all()
    # equal positive depths: of identical triangles only the first appears
    first_of = {}
    for i in range(ntri):
        first_of.setdefault(np.nan_to_num(p[i]).tobytes(), i)
    dup = [i for i in range(ntri) if first_of[np.nan_to_num(p[i]).tobytes()] != i]
    assert dup and not np.isin(tb, dup).any()


@pytest.mark.parametrize('name', ['small', 'full'])
def test_definitions_reproduce_the_fixture(vgold, name):
    case = vc.build_mesh_case(vgold[name + '_cfg'])
    hw, F = case['hw'], case['n_faces']
    assert case['meshes'].shape == (2, 3, case['n_vert']) and case['meshes'].dtype == np.float32
    if name == 'small':
        buf = (vgold['small_depth'], vgold['small_tri'], vgold['small_bary'])
        mine = vc.fresh_buffers(hw, hw, lead=(F,))
        for f in range(F):                                              # the winner rule on the meshes, against the reference's buffers
            vc.winner_rule(np.ascontiguousarray(case['meshes'][f].T), case['tri_full'], mine[0][f], mine[1][f], mine[2][f], hw, hw)
        assert all(_same(a, b) for a, b in zip(mine, buf))
        r = vc.mesh_pipeline(case, buf)
        for k, v in r.items():
            assert _same(v.astype(np.uint8) if v.dtype == bool else v, vgold[f'small_{k}']), k
        # the scatter is the inverse of the lookup wherever a vertex owns its texel; the highest index owns a shared one
        for f in range(F):
            own = vc.texel_owner(r['visible'][f], case['coord_u'], case['coord_v'])
            back = np.flip(r['uv_tex'][f], 0)[case['coord_u'], case['coord_v'], :]
            assert np.array_equal(back[own], np.clip(np.rint(r['colours'][f][own]), 0, 255).astype(np.uint8))
            assert own.sum() == (r['mask'][f] != 0).sum() == int(vgold['small_texel_count'][f])
        vis = r['visible']
    else:
        vis = np.unpackbits(vgold['full_visible_bits'], axis=1)[:, :case['n_vert']].astype(bool)
        col = np.stack([vc.sample_colors(case['img'], case['meshes'][f, 0], case['meshes'][f, 1]) for f in range(F)])
        assert np.array_equal(vc.sha(col), vgold['full_colours_sha256'])
        tm = [vc.uv_scatter(col[f], vis[f], case['coord_u'], case['coord_v']) for f in range(F)]
        assert np.array_equal(vc.sha(np.stack([t for t, _ in tm])), vgold['full_uv_tex_sha256'])
        assert np.array_equal(vc.sha(np.stack([m for _, m in tm])), vgold['full_mask_sha256'])
        assert np.array_equal(vc.sha(vis.astype(np.uint8)), vgold['full_visible_sha256'])
        # shared texels exist at this size, so the collision rule is exercised
        assert (vis[0].sum() > int(vgold['full_texel_count'][0]))
    assert np.array_equal(vis.sum(1), vgold[name + '_visible_count'])
    share = vis.mean(1)
    print(name, 'visible share', share)
    assert share[0] > 0.99 and 0.30 <= share[1] <= 0.90                # the turned face must hide a real part of itself


@pytest.mark.skipif(not vc.ref_available(), reason='oracle/_ref (the reference compiled where it lies) is not on this machine')
@pytest.mark.parametrize('seed', [11, 12, 13])
def test_winner_rule_against_the_reference_function_on_fresh_seeds(seed):
    ver, tri, (depth, tb, bw) = vc.build_soup(seed, 48 + seed, 300)
    hw = 48 + seed
    ref = (depth.copy(), tb.copy(), bw.copy())
    vc.ref_rasterize_triangles(ver, tri, ref[0], ref[1], ref[2], hw, hw)
    vc.winner_rule(ver, tri, depth, tb, bw, hw, hw)
    assert (ref[1] >= 0).sum() > 500
    assert _same(depth, ref[0]) and _same(tb, ref[1]) and _same(bw, ref[2])


@pytest.mark.skipif(not vc.ref_available(), reason='oracle/_ref (the reference compiled where it lies) is not on this machine')
def test_fixture_buffers_are_the_reference_functions(vgold):
    seed, hw, ntri = (int(x) for x in vgold['soup_cfg'])
    ver, tri, (depth, tb, bw) = vc.build_soup(seed, hw, ntri)
    vc.ref_rasterize_triangles(ver, tri, depth, tb, bw, hw, hw)
    assert _same(depth, vgold['soup_depth']) and _same(tb, vgold['soup_tri']) and _same(bw, vgold['soup_bary'])
    case = vc.build_mesh_case(vgold['full_cfg'])
    d, t, b = vc.fresh_buffers(450, 450, lead=(2,))
    for f in range(2):
        vc.ref_rasterize_triangles(np.ascontiguousarray(case['meshes'][f].T), case['tri_full'], d[f], t[f], b[f], 450, 450)
    for k, a in (('depth', d), ('tri', t), ('bary', b)):
        assert np.array_equal(vc.sha(a), vgold[f'full_{k}_sha256']), k
    assert np.array_equal((t >= 0).reshape(2, -1).sum(1), vgold['full_pixel_count'])
