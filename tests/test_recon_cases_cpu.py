"""The reconstruction edge cases without a GPU (tests/recon_cases.py): the float64 reference against the float32 oracle on every
case's inputs (a condition on the INPUTS: a quarter of the 2e-6 bar, so three quarters stay the kernel's), the packs' own shape, and
-- through expected_path, the restatement of launch_reconstruct_f16's selection -- that the tables reach the store schedules,
residues and tile counts they are named for."""
import numpy as np
import pytest

import recon_cases as rc


def _check(pack, param, roi, dense, transform, what):
    want = rc.reference(pack, param, roi, dense=dense, transform=transform)
    got = rc.oracle(pack, param, roi, dense=dense, transform=transform)
    assert got.shape == want.shape and np.isfinite(want).all()
    e = rc.per_face_err(got, want)
    assert e.max() < rc.REF_BAR, f'{what}: face {e.argmax()} oracle vs float64 {e.max():.3e}'
    return float(e.max())


@pytest.mark.parametrize('n', rc.VERTEX_COUNTS)
def test_reference_agrees_with_the_oracle_at_every_vertex_count(n):
    pack = rc.small_pack(n)
    assert pack['w_shp'].shape == (3 * n, 40) and pack['w_exp'].shape == (3 * n, 10) and pack['u_shp'].shape == (3 * n, 1)
    assert pack['tri'].min() >= 1 and pack['tri'].max() <= n and pack['keypoints'].max() < 3 * n
    assert pack['keypoints'].size == 3 * min(68, n)
    for B in rc.BATCH_SIZES:
        param, roi = rc.inputs(n, B)
        for transform in (True, False):
            for r in (None, roi):
                if B == 33 or (transform and r is None):
                    _check(pack, param, r, True, transform, f'n={n} B={B} transform={transform} roi={r is not None}')


@pytest.mark.parametrize('k', rc.LANDMARK_COUNTS)
def test_reference_agrees_with_the_oracle_at_every_landmark_count(k):
    v = rc.landmark_vertices(k)
    assert v.size == k and v.min() >= 0 and v.max() < rc.LMK_N_VERT
    if k >= 3:
        assert 0 in v and rc.LMK_N_VERT - 1 in v
        assert np.unique(v).size == k - 1                                  # exactly one vertex twice
        assert np.any(np.diff(v) < 0)                                      # unsorted
    pack = rc.landmark_pack(k)
    assert np.array_equal(pack['keypoints'].reshape(-1, 3), np.stack([3 * v, 3 * v + 1, 3 * v + 2], axis=1))
    for B in rc.BATCH_SIZES:
        param, roi = rc.inputs(k, B, tag=1)
        _check(pack, param, None, False, True, f'n_lmk={k} B={B}')
        _check(pack, param, roi, False, True, f'n_lmk={k} B={B} roi')
        _check(pack, param, roi, True, True, f'n_lmk={k} B={B} dense roi')
        # the landmarks ARE the keypoint columns of the mesh (to float64 rounding: the two products are blocked differently)
        assert rc.per_face_err(rc.reference(pack, param, roi, dense=False), rc.reference(pack, param, roi, dense=True)[:, :, v]).max() < 1e-13


@pytest.mark.parametrize('n,layout,B', rc.LARGE_B_CASES)
def test_reference_agrees_with_the_oracle_on_the_large_batches(pack, n, layout, B):
    p = pack if n == rc.FULL_N_VERT else rc.small_pack(n)
    assert p['w_shp'].shape[0] == 3 * n
    param, _ = rc.inputs(n, B, tag=2)
    _check(p, param, None, True, True, f'n={n} B={B}')


def test_reference_pose_is_the_oracles():
    from oracle import recon_numpy
    pack = rc.small_pack(129)
    param, roi = rc.inputs(129, 5)
    ang, t3d = rc.reference_pose(pack, param, roi)
    a0, t0 = recon_numpy.predict_pose(recon_numpy.Basis(pack), param[3], roi[3])
    assert ang.dtype == np.float64 and ang[3].tolist() == list(a0) and np.array_equal(t3d[3], t0)
    _, t_none = rc.reference_pose(pack, param, None)                       # the unit box leaves t3d alone, bit for bit
    pr = param * pack['param_std'][:62] + pack['param_mean'][:62]
    assert np.array_equal(t_none, pr[:, [3, 7, 11]])


@pytest.mark.parametrize('sign', [1, -1])
def test_locked_faces_are_locked_exactly(sign):
    """the conditions of the gimbal-lock test: the float32 matrix has R[2,0] == +-1 EXACTLY, every entry is 0 or +-1, and the
    reference's own branch gives the angles the test will ask the device for"""
    from oracle import recon_numpy
    pack = rc.lock_pack()
    assert np.all(pack['param_mean'][:12] == 0) and np.all(pack['param_std'][:12] == 1)
    param, _ = rc.lock_inputs(sign)
    base, _ = rc.lock_inputs(0)
    for lane in range(rc.LOCK_B):
        R = rc.rotation_f32(pack, param[lane])
        assert R.dtype == np.float32
        if lane in rc.LOCK_LANES:
            assert R[2, 0] == sign and set(np.abs(R).reshape(-1).tolist()) == {0.0, 1.0}
            want = [-90.0, -90.0, 0.0] if sign > 0 else [90.0, 0.0, 0.0]
            assert np.abs(np.array(recon_numpy.matrix2angle_corr(R)) - want).max() < 1e-12
        else:
            assert abs(R[2, 0]) < 0.999 and np.array_equal(param[lane], base[lane])


# ---- the tables hit what they name ----

def _small_paths():
    """every (vertex count, layout, batch size) the GPU layout test runs -> Path"""
    out = {}
    for n in rc.VERTEX_COUNTS:
        for lay in [rc.default_layout(n)] + rc.layouts(n):
            for B in rc.BATCH_SIZES:
                out[(n, lay.name, B)] = (lay, rc.expected_path(n, lay.pitch, lay.pad_writable, lay.offset % 32 == 0, B))
    return out


def test_layout_table():
    for n in rc.VERTEX_COUNTS:
        names = [l.name for l in rc.layouts(n)]
        assert len(names) == len(set(names)) == (8 if n % 128 == 0 else 9)
        for l in rc.layouts(n):
            assert l.pitch >= n and l.offset in (0, 1, 4, 16)
    assert rc.default_layout(1023) == ('default', 1023, 0, 0) and rc.default_layout(1024) == ('default', 1024, 0, 0)
    assert rc.default_layout(4097) == ('default', 4224, 1, 0)


def test_small_cases_reach_every_schedule_with_one_face_tile_per_workgroup():
    paths = _small_paths()
    kinds = {p.kind for _, p in paths.values() if p.per == 1}
    assert kinds == {'FAST', 'PK', 'guarded'}
    assert all(p.per == 1 and p.tail_per in (0, 1) for _, p in paths.values())        # B <= 65: never more than one
    # FAST on packed rows (pitch == n): n a multiple of 128 with pad_writable
    assert {n for (n, _, _), (lay, p) in paths.items() if p.kind == 'FAST' and lay.pitch == n} == {128, 1024, 4096}
    # PK at every residue named, and at each of them with whole tiles only, a ragged tile only (B < 32) and both
    pk = {(n % 32, B) for (n, _, B), (_, p) in paths.items() if p.kind == 'PK'}
    assert {r for r, _ in pk} == {0, 1, 5, 16, 31}
    assert all({(r, B) for B in rc.BATCH_SIZES} <= pk for r in (0, 1, 5, 16, 31))
    # PK switches on AT 4096, and the default buffer of a 4096-vertex pack is packed rows
    assert paths[(4095, 'packed', 32)][1].kind == 'guarded' and paths[(4096, 'packed', 32)][1].kind == 'PK'
    assert paths[(4096, 'default', 32)][1].kind == 'PK' and paths[(4097, 'default', 32)][1].kind == 'FAST'
    # pitch = roundup128 - 1 == n at 4479: pad_writable without room for whole runs stays off FAST
    assert paths[(4479, 'pitch roundup128-1, pad_writable', 33)][1].kind == 'PK'
    # an unaligned base, an odd pitch and everything below 4096 vertices run guarded
    for (n, name, B), (lay, p) in paths.items():
        if lay.offset or (lay.pitch != n and not lay.pad_writable) or (n < 4096 and p.kind != 'FAST'):
            assert p.kind == 'guarded', (n, name, B)


def test_large_batches_walk_several_face_tiles_per_workgroup():
    got = {}
    for n, name, B in rc.LARGE_B_CASES:
        lay = rc.layout_by_name(n, name)
        got[(n, B)] = p = rc.expected_path(n, lay.pitch, lay.pad_writable, True, B)
        assert p.per >= 2 and p.ragged, (n, name, B, p)
    assert got[(4097, 1701)].kind == 'FAST' and got[(4097, 1701)].tail_per == 1          # FAST, then a guarded tail
    assert got[(4485, 1445)].kind == 'PK' and got[(rc.FULL_N_VERT, 161)].kind == 'PK'
    # the chunks of 32 faces they are compared with are one whole tile on the same schedule
    for n, name, B in rc.LARGE_B_CASES:
        lay = rc.layout_by_name(n, name)
        assert rc.expected_path(n, lay.pitch, lay.pad_writable, True, 32) == (got[(n, B)].kind, 1, False, 0)


def test_expected_path_mirrors_the_launcher_source():
    """the constants expected_path restates are the ones in the launcher (a changed target or window must be restated here)"""
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, 'synergynet_amd', 'csrc', 'recon_kernels.hip')).read()
    assert 'test_knob("recon_wgs", %d)' % rc.WG_TARGET in src
    assert 'test_knob("recon_pk_wpg", 8)' in src and '(pk_wpg == 8 ? 7 : 3) * 32' in src and rc.PK_WINDOW == 7 * 32
    assert 'n_vert >= %d' % rc.PK_MIN_VERT in src and 'wg_target / 2' in src
