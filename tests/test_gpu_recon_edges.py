"""GPU tests of the 3DMM reconstruction away from the default pack (run with `-m gpu`): every store schedule of recon_kernels.hip
-- the straight-line FAST kernel, the packed-row whole-line schedule PK, the guarded instantiation, and the fp32 kernel of
SYNERGY_HIP_FUSION=1 -- across vertex counts (n mod 32 = 0 / 1 / 5 / 16 / 31, below one tile, around 4096 where PK switches on, whole
and nearly empty PK windows), output layouts (packed / pitched, aligned or not, pad columns writable or not), several face tiles per
workgroup, landmark counts up to 300 (lmk_pose_kernel's `v += 256` loop; the pose lane owning a landmark) and the two gimbal-lock
branches of pose_of_face.  Yardstick: the float64 reference of tests/recon_cases.py (held to the oracle by
tests/test_recon_cases_cpu.py) on per_face_err, bar 2e-6; layouts and batch splits are equality of bits.

Every output buffer is carved out of a flat allocation prefilled with a NaN sentinel, with guard zones of a row + 256 floats on
both sides, and read back as int32: an overrun or a store into pad columns the caller did not release shows as a changed sentinel,
an unwritten vertex as a NaN.

Largest per_face_err measured on an MI355X (bar 2e-6; 1e-5 for the one-launch landmarks):
  SYNERGY_HIP_FUSION=2   meshes 6.3e-07 (n_vert = 1, B = 65)     large batches 4.6e-07 (n_vert = 4485, B = 1445)
                         landmarks 3.6e-07 (n_lmk = 300, B = 33)  one launch 1.8e-07 (n_lmk = 300, B = 33)
  SYNERGY_HIP_FUSION=1   meshes 2.0e-07 (n_vert = 1, B = 31)     large batches 2.0e-07 (n_vert = 4097, B = 1701)
                         landmarks 1.8e-07 (n_lmk = 300, B = 33)  one launch 1.8e-07 (n_lmk = 300, B = 33)
No kernel or launcher change was needed: every case passed on the kernels as they were.
"""
import ctypes as C
import contextlib

import numpy as np
import pytest

import recon_cases as rc
from conftest import rel_max
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD                   # a quiet NaN no kernel produces
SCHEDULES = (2, 1)                      # SYNERGY_HIP_FUSION: 2 = recon_f16_kernel (FAST / PK / guarded), 1 = recon_kernel (0 shares it)
VIA_ABI = ('packed+pad_writable', 'pitch roundup128, pad_writable', 'pitch roundup128-1, pad_writable')      # (b), (e), (f): syn_reconstruct_pitched itself


@pytest.fixture(scope='module')
def handles(backbone_sd):
    """one handle per pack, cached for the module: get(key, make_pack) -> (pack, SynergyNet)"""
    from synergynet_amd.synergy3DMM import SynergyNet
    cache = {}

    def get(key, make_pack):
        if key not in cache:
            pack = make_pack()
            cache[key] = (pack, SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd))
        return cache[key]
    yield get
    cache.clear()


@contextlib.contextmanager
def schedule(model, fusion):
    """the handle on SYNERGY_HIP_FUSION = fusion (include/synergy_hip.h syn_set_schedule: the same switch on a live handle)"""
    prev = model._lib.syn_set_schedule(model._h, fusion)
    assert prev >= 0
    try:
        yield
    finally:
        model._lib.syn_set_schedule(model._h, prev)


class Carved:
    """[B,3,pitch][:, :, :n] float32 inside a flat sentinel-filled allocation; base `offset` floats past a 128-byte boundary"""

    def __init__(self, B, n, pitch, offset=0):
        import torch
        guard = (pitch + 256 + 31) // 32 * 32
        body = B * 3 * pitch
        self.flat = torch.full((guard + 32 + offset + body + guard,), SENTINEL, dtype=torch.int32, device='cuda')
        base = self.flat.data_ptr()
        assert base % 4 == 0
        lo = guard + (-(base // 4 + guard)) % 32 + offset
        self.B, self.n, self.pitch, self.lo, self.hi = B, n, pitch, lo, lo + body
        self.view = self.flat[lo:lo + body].view(torch.float32).view(B, 3, pitch)[:, :, :n]
        assert self.view.data_ptr() % 128 == 4 * offset and lo >= pitch + 256 and self.flat.numel() - self.hi >= pitch + 256

    def bits(self, pad_writable, what=''):
        """the [B,3,n] result as int32, after the guards (and the pad columns the caller kept) were seen untouched"""
        h = self.flat.cpu().numpy()
        assert (h[:self.lo] == SENTINEL).all(), f'{what}: store in front of the buffer'
        assert (h[self.hi:] == SENTINEL).all(), f'{what}: store behind the buffer'
        body = h[self.lo:self.hi].reshape(self.B, 3, self.pitch)
        if not pad_writable:
            assert (body[:, :, self.n:] == SENTINEL).all(), f'{what}: store into pad columns the caller did not release'
        return np.ascontiguousarray(body[:, :, :self.n])


def f32(bits):
    return bits.view(np.float32)


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(model, param_d, roi_d, lay, n, dense=True, transform=True, via_abi=False, what=''):
    """one reconstruction into a carved buffer of layout `lay`, through the class or through syn_reconstruct_pitched -> int32 bits"""
    B = param_d.shape[0]
    c = Carved(B, n, lay.pitch, lay.offset)
    if via_abi:
        abi.check(model._lib.syn_reconstruct_pitched(model._h, param_d.data_ptr(), B, 62, int(dense), int(transform),
                                                     roi_d.data_ptr() if roi_d is not None else None, c.view.data_ptr(), lay.pitch,
                                                     lay.pad_writable, model._stream()))
    else:
        c.view._syn_pad_writable = bool(lay.pad_writable)
        assert model.reconstruct(param_d, roi=roi_d, dense=dense, transform=transform, out=c.view) is c.view
    return c.bits(lay.pad_writable, what)


def check_ref(bits, want, what):
    got = f32(bits)
    assert np.isfinite(got).all(), f'{what}: {np.count_nonzero(~np.isfinite(got))} elements not finite (sentinel left: {np.count_nonzero(bits == SENTINEL)})'
    e = rc.per_face_err(got, want)
    print(f'recon-edge {what} err={e.max():.3e}')
    assert e.max() < rc.BAR, f'{what}: face {e.argmax()} rel err {e.max():.3e}'


# ---- 1. against the float64 reference, every vertex count, the default buffer ----

@pytest.mark.parametrize('n', rc.VERTEX_COUNTS)
@pytest.mark.parametrize('fusion', SCHEDULES)
def test_every_vertex_count_against_the_float64_reference(handles, fusion, n):
    pack, m = handles(('n', n), lambda: rc.small_pack(n))
    lay = rc.default_layout(n)
    ev = m.empty_vertices(3, dense=True)                                  # the carved default buffer IS empty_vertices' layout
    assert (ev.stride(1), int(ev._syn_pad_writable), ev.data_ptr() % 128) == (lay.pitch, lay.pad_writable, 0) and tuple(ev.shape) == (3, 3, n)
    with schedule(m, fusion):
        for B in rc.BATCH_SIZES:
            param, roi = rc.inputs(n, B)
            pd, rd = dev(param), dev(roi)
            for transform in (True, False):
                for r in (None, roi):
                    if B == 33 or (transform and r is None):
                        what = f'fusion={fusion} n={n} B={B} transform={int(transform)} roi={int(r is not None)}'
                        bits = run(m, pd, None if r is None else rd, lay, n, transform=transform, what=what)
                        check_ref(bits, rc.reference(pack, param, r, dense=True, transform=transform), what)


# ---- 2. layouts are one result ----

@pytest.mark.parametrize('n', rc.VERTEX_COUNTS)
@pytest.mark.parametrize('fusion', SCHEDULES)
def test_every_layout_is_bit_identical_to_the_default_buffer(handles, fusion, n):
    """packed / pitched, 128-byte aligned or 1, 4, 16 floats past, pad columns released or kept: the launcher picks FAST, PK or the
    guarded kernel from them (rc.expected_path) and the mesh must not notice"""
    pack, m = handles(('n', n), lambda: rc.small_pack(n))
    with schedule(m, fusion):
        for B in rc.BATCH_SIZES:
            param, roi = rc.inputs(n, B)
            pd, rd = dev(param), dev(roi)
            base = run(m, pd, rd, rc.default_layout(n), n, what=f'fusion={fusion} n={n} B={B} default')
            assert np.isfinite(f32(base)).all()
            for lay in rc.layouts(n):
                what = f'fusion={fusion} n={n} B={B} {lay.name} ({rc.expected_path(n, lay.pitch, lay.pad_writable, lay.offset % 32 == 0, B).kind})'
                got = run(m, pd, rd, lay, n, via_abi=lay.name in VIA_ABI, what=what)
                bad = np.argwhere(got != base)
                assert bad.size == 0, f'{what}: {bad.shape[0]} elements differ from the default buffer, first at (face, coord, vertex) {bad[0].tolist()}'


# ---- 3. several face tiles per workgroup ----

@pytest.mark.parametrize('n,layout,B', rc.LARGE_B_CASES)
@pytest.mark.parametrize('fusion', SCHEDULES)
def test_several_face_tiles_per_workgroup(handles, pack, fusion, n, layout, B):
    """a workgroup walks two face tiles through its double-buffered operand tile (FAST with a guarded tail, PK twice), the last one
    ragged: against the reference, and bitwise against the same faces in chunks of 32 -- a face's mesh must not depend on the batch"""
    p, m = handles(('n', n), (lambda: pack) if n == rc.FULL_N_VERT else (lambda: rc.small_pack(n)))
    lay = rc.layout_by_name(n, layout)
    param, _ = rc.inputs(n, B, tag=2)
    pd = dev(param)
    with schedule(m, fusion):
        what = f'fusion={fusion} n={n} B={B} {layout}'
        big = run(m, pd, None, lay, n, what=what)
        check_ref(big, rc.reference(p, param, None, dense=True), what)
        for lo in range(0, B, 32):
            part = run(m, pd[lo:lo + 32], None, lay, n, what=f'{what} faces {lo}..')
            assert np.array_equal(part, big[lo:lo + 32]), f'{what}: faces {lo}.. differ from the same faces run alone'


# ---- 4. landmark counts ----

@pytest.mark.parametrize('k', rc.LANDMARK_COUNTS)
@pytest.mark.parametrize('fusion', SCHEDULES)
def test_every_landmark_count(handles, fusion, k):
    pack, m = handles(('k', k), lambda: rc.landmark_pack(k))
    v = rc.landmark_vertices(k)
    assert m._n_lmk == k and m._n_vert == rc.LMK_N_VERT
    packed, pitched = rc.Layout('packed', k, 0, 0), rc.Layout('pitch k+5', k + 5, 0, 0)
    with schedule(m, fusion):
        for B in rc.BATCH_SIZES:
            param, roi = rc.inputs(k, B, tag=1)
            pd, rd = dev(param), dev(roi)
            what = f'fusion={fusion} n_lmk={k} B={B}'
            want = rc.reference(pack, param, roi, dense=False)
            lmk = run(m, pd, rd, packed, k, dense=False, what=what + ' lmk')
            check_ref(lmk, want, what + ' lmk')
            mesh = run(m, pd, rd, rc.default_layout(rc.LMK_N_VERT), rc.LMK_N_VERT, what=what + ' mesh')
            assert rel_max(f32(mesh)[:, :, v], f32(lmk)) < 1e-6, what
            # one launch: landmarks + pose
            c = Carved(B, k, k)
            assert c.view.is_contiguous()
            out, (ang, t3d) = m.landmarks_and_pose(pd, roi=rd, out=c.view)
            one = c.bits(0, what + ' one launch')
            assert np.isfinite(f32(one)).all(), what
            e = rc.per_face_err(f32(one), want)
            print(f'recon-edge {what} one-launch err={e.max():.3e}')
            assert e.max() < 1e-5, f'{what}: one launch, face {e.argmax()} rel err {e.max():.3e}'
            a2, t2 = m.predict_pose_batch(pd, rd)
            assert np.array_equal(t3d.cpu().numpy().view(np.int32), t2.cpu().numpy().view(np.int32)), what
            assert float((ang - a2).abs().max()) < 1e-4, what
            a_ref, t_ref = rc.reference_pose(pack, param, roi)
            assert np.abs(ang.cpu().numpy() - a_ref).max() < 1e-3 and rel_max(t3d.cpu().numpy(), t_ref) < 1e-4, what      # (the bounds of test_gpu_parity.py)
            # ... and into a pitched view of the caller's
            cp = Carved(B, k, k + 5)
            assert not cp.view.is_contiguous() or B * k == 1
            out2, (a3, t3) = m.landmarks_and_pose(pd, roi=rd, out=cp.view)
            two = cp.bits(0, what + ' pitched view')
            assert out2 is cp.view and rel_max(f32(two), f32(one)) < 1e-6, what
            assert np.array_equal(t3.cpu().numpy().view(np.int32), t2.cpu().numpy().view(np.int32)) and float((a3 - a2).abs().max()) < 1e-4, what
            assert np.array_equal(run(m, pd, rd, pitched, k, dense=False, what=what + ' lmk pitched'), lmk), what


def test_refine_landmarks_refuses_a_landmark_count_other_than_68(handles):
    import torch
    from synergynet_amd import synth
    state = synth.make_synergy_state(5)
    param, _ = rc.inputs(33, 3, tag=1)
    pd = dev(param)
    pool = torch.zeros((3, 1280), dtype=torch.float32, device='cuda')
    for k in (33, 257):
        _, m = handles(('k', k), lambda: rc.landmark_pack(k))
        m.load_synergy_state(state)
        with pytest.raises(abi.SynergyHipError) as err:
            m.refine_landmarks(pd, pool)
        assert err.value.code == abi.SYN_ERR_INVALID and f'{k} points' in err.value.msg
        out = torch.full((3, 3, 68), float('nan'), dtype=torch.float32, device='cuda')
        assert m._lib.syn_refine_landmarks(m._h, pd.data_ptr(), pool.data_ptr(), 3, 1, None, None, out.data_ptr(), None, m._stream()) == abi.SYN_ERR_INVALID
        assert torch.isnan(out).all()                                      # nothing was written by the refused call
    _, m = handles(('k', 68), lambda: rc.landmark_pack(68))              # 68 points, unsorted with a duplicate: accepted
    m.load_synergy_state(state)
    refined, coarse = m.refine_landmarks(pd, pool, return_coarse=True)
    assert tuple(refined.shape) == (3, 3, 68) and torch.isfinite(refined).all()
    assert torch.equal(coarse, m.landmarks_and_pose(pd)[0])


# ---- 5. gimbal lock ----

@pytest.mark.parametrize('sign', [1, -1])
def test_gimbal_lock_branches_of_pose_of_face(handles, sign):
    """R[2,0] == +-1 exactly (rows (0, s, 0), (0, 0, s) and swapped, s = 2^-11, on a pack whose pose entries de-whiten exactly): both
    pose kernels take matrix2angle_corr's gimbal branch, and the ordinary faces around them do not notice"""
    from oracle import recon_numpy
    pack, m = handles('lock', rc.lock_pack)
    param, roi = rc.lock_inputs(sign)
    base, _ = rc.lock_inputs(0)
    pd, bd, rd = dev(param), dev(base), dev(roi)
    want = {lane: np.array(recon_numpy.matrix2angle_corr(rc.rotation_f32(pack, param[lane]))) for lane in rc.LOCK_LANES}
    assert all(abs(w[0]) == 90.0 for w in want.values())
    others = np.setdiff1d(np.arange(rc.LOCK_B), rc.LOCK_LANES)
    bits = lambda t: t.cpu().numpy().view(np.int64 if t.dtype.itemsize == 8 else np.int32)
    for call in ('predict_pose_batch', 'landmarks_and_pose'):
        if call == 'predict_pose_batch':
            (ang, t3d), (ang0, t0) = m.predict_pose_batch(pd, rd), m.predict_pose_batch(bd, rd)
        else:
            (lmk, (ang, t3d)), (lmk0, (ang0, t0)) = m.landmarks_and_pose(pd, roi=rd), m.landmarks_and_pose(bd, roi=rd)
            assert np.isfinite(lmk.cpu().numpy()).all()
            assert np.array_equal(bits(lmk)[others], bits(lmk0)[others])
            e = rc.per_face_err(lmk.cpu().numpy(), rc.reference(pack, param, roi, dense=False))
            assert e.max() < 1e-5, (call, e.argmax(), e.max())
        a = ang.cpu().numpy()
        for lane, w in want.items():
            assert np.abs(a[lane] - w).max() <= 1e-9, (call, sign, lane, a[lane].tolist(), w.tolist())
        assert np.array_equal(bits(ang)[others], bits(ang0)[others]) and np.array_equal(bits(t3d)[others], bits(t0)[others]), call
        _, t_ref = rc.reference_pose(pack, param, roi)
        assert rel_max(t3d.cpu().numpy(), t_ref) < 1e-6, call
