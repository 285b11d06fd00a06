"""CPU-side tests of the textured-mesh feature (no GPU): the coloured OBJ writer against the reference's own bytes, the UV
assets in ParamsPack and synth, the host-side pixel tables, and the checker the GPU tests compare against
(oracle.sim3dr.RenderPipeline(impl='oracle', texture=...)) against the fixture the REAL reference produced
(tests/golden/texture_golden.npz, written by tests/golden/make_texture_golden.py with impl='ref')."""
import ctypes
import os

import numpy as np
import pytest

import texture_cases as tc
from conftest import ROOT

NEW_SYMBOLS = ('syn_load_uv_map', 'syn_select_topology', 'syn_uv_colors', 'syn_gather_vertices', 'syn_mesh_shade_textured')


@pytest.fixture(scope='module')
def tgold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'texture_golden.npz')))


@pytest.mark.parametrize('which', [0, 1])
def test_write_obj_with_colors_bytes_equal_the_reference(tgold, tmp_path, which):
    from synergynet_amd.inference import write_obj_with_colors
    arg, name = str(tgold[f'obj{which}_arg']), str(tgold[f'obj{which}_name'])
    assert (which == 0) == (not arg.endswith('.obj'))                  # one of the two names lacks the extension
    write_obj_with_colors(str(tmp_path / arg), tgold[f'obj{which}_vertices'], tgold[f'obj{which}_triangles'], tgold[f'obj{which}_colors'])
    got = (tmp_path / name).read_bytes()
    assert got == tgold[f'obj{which}_bytes'].tobytes()
    lines = got.decode().splitlines()
    v, c = tgold[f'obj{which}_vertices'], tgold[f'obj{which}_colors']
    assert lines[0] == 'v {:.4f} {:.4f} {:.4f} {} {} {}'.format(v[0, 0], v[1, 0], v[2, 0], c[0, 2], c[0, 1], c[0, 0])      # colour reversed
    t = tgold[f'obj{which}_triangles']
    assert lines[v.shape[1]] == f'f {t[0, 0]} {t[1, 0]} {t[2, 0]}'                                                          # rows as given


def test_params_pack_uv_assets_optional(pack, tmp_path):
    from synergynet_amd import synth
    from synergynet_amd.params import ParamsPack
    pp = ParamsPack(pack=pack)
    assert pp.uv_vert is None and pp.keep_ind is None and pp.tri_deletion is None
    small = synth.make_3dmm(n_vert=30 * 30)
    assets = synth.make_uv_assets(None, 30, 30, seed=3)
    pp = ParamsPack(pack=dict(small, **assets))
    assert pp.uv_vert.shape == (900, 2) and pp.keep_ind.ndim == 1 and pp.tri_deletion.shape[0] == 3
    assert np.array_equal(pp.keep_ind, assets['keep_ind']) and np.array_equal(pp.tri_deletion, assets['tri_deletion'])
    # from the files, with and without the three UV files
    import pickle
    d = tmp_path / '3dmm'
    d.mkdir()
    for k, fn in (('keypoints', 'keypoints_sim.npy'), ('w_shp', 'w_shp_sim.npy'), ('w_exp', 'w_exp_sim.npy'), ('u_shp', 'u_shp.npy'), ('u_exp', 'u_exp.npy')):
        np.save(d / fn, small[k])
    with open(d / 'param_whitening.pkl', 'wb') as f:
        pickle.dump(dict(param_mean=small['param_mean'], param_std=small['param_std']), f)
    assert ParamsPack(data_dir=str(d)).uv_vert is None
    np.save(d / 'BFM_UV.npy', assets['uv_vert']); np.save(d / 'keptInd.npy', assets['keep_ind']); np.save(d / 'deletedTri.npy', assets['tri_deletion'])
    pp = ParamsPack(data_dir=str(d))
    assert np.array_equal(pp.uv_vert, assets['uv_vert']) and np.array_equal(pp.keep_ind, assets['keep_ind']) and np.array_equal(pp.tri_deletion, assets['tri_deletion'])
    with pytest.raises(RuntimeError, match='Missing data'):            # still raised for what it is raised for today
        ParamsPack(data_dir=str(tmp_path / 'nowhere'))


def test_uv_pixel_coords_dtype_and_truncation():
    from synergynet_amd.params import uv_pixel_coords
    # column 0 is v, column 1 is u (uv_texture_realFaces.py:48-49); truncation toward zero, in the asset's own dtype
    uv = np.array([[0.0, 0.999], [0.5, 0.25], [0.99999, 0.0039215], [0.0039216, 1 / 255], [254.9999 / 255, 0.7]])
    for dt in (np.float32, np.float64):
        a = uv.astype(dt)
        u, v = uv_pixel_coords(a)
        assert u.dtype == np.int32 and v.dtype == np.int32
        assert np.array_equal(u, (a[:, 1] * 255.0).astype(np.int32)) and np.array_equal(v, (a[:, 0] * 255.0).astype(np.int32))
        assert (a[:, 1] * 255.0).dtype == dt                            # the product stays in the asset's dtype
        assert u[0] == 254 and v[1] == 127 and v[2] == 254 and u.max() <= 254 and v.max() <= 254


@pytest.mark.parametrize('rows,cols,n_vert', [(24, 24, None), (40, 44, None), (48, 31, 1400), (231, 231, 53215)])
def test_make_uv_assets_invariants(rows, cols, n_vert):
    from synergynet_amd import synth
    a = synth.make_uv_assets(n_vert, rows, cols, seed=5)
    n = n_vert or rows * cols
    uv, keep, td = a['uv_vert'], a['keep_ind'], a['tri_deletion']
    assert uv.shape == (n, 2) and uv.dtype == np.float32 and uv.min() >= 0 and uv.max() < 1
    assert keep.ndim == 1 and np.issubdtype(keep.dtype, np.integer) and keep.min() >= 0 and keep.max() < n
    assert np.array_equal(keep, np.unique(keep)) and 0.5 * n < keep.size < n
    assert td.shape[0] == 3 and td.dtype == np.int32 and td.min() == 1 and td.max() == keep.size       # 1-based, into the kept list
    assert np.array_equal(np.unique(td - 1), np.arange(keep.size))                                    # every kept vertex is used
    # consistent with make_grid_topology: the kept triangles are the grid's triangles whose corners all survive, in order
    full = synth.make_grid_topology(rows, cols, n_vert=n_vert)
    surv = np.isin(full, keep).all(1)
    assert np.array_equal(keep[td.T - 1], full[surv])
    # a band of the grid is gone, so the bounding box of the kept vertices differs from the full mesh's
    m = synth.make_face_meshes(1, rows, cols, n_vert=n_vert, height=100, width=100, seed=1)[0]
    assert not np.allclose(m[:, keep].min(1), m.min(1)) or not np.allclose(m[:, keep].max(1), m.max(1))
    assert np.array_equal(synth.make_uv_assets(n_vert, rows, cols, seed=5)['keep_ind'], keep)           # seeded


@pytest.mark.parametrize('name', ['small', 'perface', 'full'])
def test_oracle_textured_path_reproduces_reference_fixture(tgold, name):
    """Pins the checker of the GPU tests: impl='oracle' (C restatement + numpy lighting) on the rebuilt inputs gives the images
    the reference's own C++ gave (impl='ref', recorded in the fixture), byte for byte."""
    case = tc.build(tgold[name + '_cfg'])
    assert [case['keep'].size, case['tri_kept'].shape[0]] == [int(x) for x in tgold[name + '_kept']]
    tex = tc.demo_tex(case)
    assert tex.ndim == (3 if name == 'perface' else 2) and tex.dtype == np.float32
    r = tc.oracle_render(case, tex, impl='oracle')
    assert np.array_equal(r['overlay'], tgold[name + '_overlay'])
    assert (r['overlay'] != case['img']).any(2).mean() > 0.05                                        # something was drawn
    if name != 'full':
        assert np.array_equal(r['normal'], tgold[name + '_normal']) and not np.isnan(r['normal']).any()
        assert np.array_equal(r['light'], tgold[name + '_light']) and np.array_equal(r['colours'], tgold[name + '_colours'])
        assert np.array_equal(r['blend'], tgold[name + '_blend'])
    if name == 'small':
        assert np.array_equal(tex, tgold['small_tex_final'])           # the shared array was multiplied in place, face after face
        assert np.array_equal(tgold['small_colours'][-1], tgold['small_tex_final'])
        l = tgold['small_light']
        t0 = tc.demo_tex(case)
        assert np.array_equal(((t0 * l[0]) * l[1]) * l[2], tgold['small_tex_final'])


def test_new_symbols_in_header_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import build_library
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    for s in NEW_SYMBOLS:
        assert s + '(' in hdr and s in abi.EXPORTED_SYMBOLS and hasattr(l, s), s
    l.syn_abi_version.restype = ctypes.c_int
    assert l.syn_abi_version() == 1


def test_render_rejects_file_output_only():
    """render(tex=...) no longer raises NotImplementedError by itself; `wfp` still does (cv2.imwrite is out of scope)."""
    from synergynet_amd import sim3dr
    with pytest.raises(NotImplementedError, match='file output'):
        sim3dr.render(np.zeros((4, 4, 3), np.uint8), [], wfp='x.jpg', tex=np.zeros((1, 3), np.float32))
