"""GPU parity of the mesh consumers at their edges (cases: tests/mesh_edge_cases.py): syn_rasterize at zero depths of either sign,
at the empty-buffer threshold, with 1 / 3 / 4 channels, colours outside [0, 1] and 3 / 254 / 255 faces in one call; every branch of
the Phong vertex colours; render_batch with 300 faces; syn_add_weighted at its ties and both saturations.  The device is held to the
fixture made by the reference's own code (tests/golden/mesh_edges_golden.npz) AND to the live CPU oracle (oracle/sim3dr.py);
tests/test_mesh_edges_cpu.py shows on the oracle that every case meets the edge it is there for.

Bars (those of tests/test_gpu_render.py): images, normals and the blend byte for byte; vertex colours to 1e-6 absolute -- numpy
raises to the exponent with a float32 power, the kernel with an exactly rounded double product: no difference for exponents 1 and 2,
one float32 ulp (6e-8) on a tenth of the values for 3, 5 and 8.  Every effect a configuration is there for is 1e-4 or more.
Every frame is random bytes and every other output buffer is filled with a sentinel before the call."""
import os

import numpy as np
import pytest

import mesh_edge_cases as mc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 12345.0


@pytest.fixture(scope='module')
def emodel():
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    return SynergyNet(device='cuda:0', pack=synth.make_3dmm(n_vert=640), backbone_state=synth.make_backbone_state())


@pytest.fixture(scope='module')
def mgold():
    return dict(np.load(os.path.join(HERE, 'golden', 'mesh_edges_golden.npz')))


@pytest.fixture(scope='module')
def oracle_img():
    from oracle import sim3dr as osim
    return mc.expected_images(osim)


@pytest.fixture(scope='module')
def oracle_lit():
    from oracle import sim3dr as osim
    return mc.expected_lights(osim)


def _same_image(got, key, mgold, oracle_img):
    """Byte for byte against the reference's image and the oracle's (which test_mesh_edges_cpu.py holds equal)."""
    for name, want in (('fixture', mgold[key]), ('oracle', oracle_img[key])):
        bad = (got != want).any(2)
        assert got.shape == want.shape and not bad.any(), (f'{key} vs {name}: {int(bad.sum())} pixels differ, first at '
                                                            f'{tuple(np.argwhere(bad)[0])}: got {got[bad][0]}, want {want[bad][0]}')


def _draw_faces(m, tri, meshes, colors, img, reverse=False):
    """ONE syn_rasterize call on F meshes in the [F,3,N] layout, colours [F,N,c].  Returns (status, the image after the call)."""
    import torch
    from synergynet_amd import sim3dr
    F, _, n = meshes.shape
    H, W, c = img.shape
    sim3dr._ensure_topology(m, tri, n)
    m._tri_obj = None                                          # slot 0 no longer holds the model's own topology
    vt, ct, it = (torch.from_numpy(np.ascontiguousarray(a)).to(m.device) for a in (meshes, colors, img))
    with torch.cuda.device(m.device):
        rc = m._lib.syn_rasterize(m._h, vt.data_ptr(), ct.data_ptr(), F, 1, c, it.data_ptr(), H, W, int(reverse), m._stream())
    torch.cuda.synchronize()
    return rc, it.cpu().numpy()


def _poison_scratch(m):
    from synergynet_amd import abi
    abi.check(abi.lib().syn_debug_poison_workspace(m._h, 4, 0xFF))


# ---- A. depth rule ----
@pytest.mark.parametrize('order', list(mc.PAIR_ORDERS))
def test_zero_depths_of_either_sign_tie_and_the_first_triangle_wins(emodel, mgold, oracle_img, order):
    """Two coincident triangles, red at -0.0 and green at +0.0: `+0 > -0` is false, so the one listed first keeps every pixel.
    A z-key taken from the raw depth bits orders -0 below +0 and lets green win in both orders: before raster_depth_kernel keyed a
    zero depth as +0, `neg_first` gave (0, 255, 0) on all 36 covered pixels where the reference gives (255, 0, 0)."""
    from synergynet_amd import sim3dr
    ver, tris, col, bg = mc.coincident_pair()
    _poison_scratch(emodel)
    for rev in (0, 1):
        got = sim3dr.rasterize(ver, tris[order], col, bg=bg.copy(), reverse=bool(rev))
        y, x = mc.PAIR_PROBE
        print(f'{order} reverse={rev}: pixel {tuple(got[11 - y if rev else y, x])}, fixture {tuple(mgold[f"a1_{order}_rev{rev}"][11 - y if rev else y, x])}')
        _same_image(got, f'a1_{order}_rev{rev}', mgold, oracle_img)


def test_signed_zero_soup_is_resolved_by_order_alone(emodel, mgold, oracle_img):
    from synergynet_amd import sim3dr
    ver, tri, col, bg = mc.zero_soup()
    for rev in (0, 1):
        _same_image(sim3dr.rasterize(ver, tri, col, bg=bg.copy(), reverse=bool(rev)), f'a2_rev{rev}', mgold, oracle_img)
    for z in (0.0, -0.0):                                      # the signs alone change nothing
        same = ver.copy()
        same[:, 2] = z
        _same_image(sim3dr.rasterize(same, tri, col, bg=bg.copy()), 'a2_rev0', mgold, oracle_img)


def test_empty_buffer_threshold_pixel_for_pixel(emodel, mgold, oracle_img):
    """Depths at -1e8 and one float32 step above it: drawn exactly where the rounded interpolation ends above -1e8."""
    from synergynet_amd import sim3dr
    ver, tri, col, bg = mc.threshold_pair()
    _same_image(sim3dr.rasterize(ver, tri, col, bg=bg.copy()), 'a3', mgold, oracle_img)


def test_a_later_face_overwrites_an_earlier_nearer_one_in_one_call(emodel, mgold, oracle_img):
    meshes, tri, col, bg = mc.stacked_faces()
    _poison_scratch(emodel)
    rc, got = _draw_faces(emodel, tri, meshes, col, bg)
    assert rc == 0
    _same_image(got, 'a4', mgold, oracle_img)


# ---- B. channels and colour conversion ----
@pytest.mark.parametrize('c', mc.CHANNELS)
def test_channels_and_colours_outside_the_unit_interval(emodel, mgold, oracle_img, c):
    from synergynet_amd import sim3dr
    ver, tri, col, bg = mc.channel_case(c)
    assert col.shape == (ver.shape[0], c) and (col < 0).any() and (col > 1).any()
    _same_image(sim3dr.rasterize(ver, tri, col, bg=bg.copy()), f'b_c{c}', mgold, oracle_img)


def test_flat_colours_keep_the_low_byte_of_a_32_bit_integer(emodel, mgold, oracle_img):
    from synergynet_amd import sim3dr
    for k, (value, byte) in enumerate(mc.FLAT_COLOURS):
        ver, tri, col, bg = mc.flat_case(value)
        got = sim3dr.rasterize(ver, tri, col, bg=bg.copy())
        assert int(got[mc.PAIR_PROBE][0]) == byte, (value, got[mc.PAIR_PROBE])
        _same_image(got, f'b_flat{k}', mgold, oracle_img)


def test_five_channels_are_refused_and_the_frame_is_left_alone(emodel):
    from synergynet_amd import abi, sim3dr
    ver, tri, _, _ = mc.channel_case(4)
    col = np.random.default_rng(1).uniform(0, 1, (ver.shape[0], 5)).astype(np.float32)
    bg = mc.image(mc.HW, mc.HW, 5, 2)
    before = bg.copy()
    with pytest.raises(abi.SynergyHipError) as e:
        sim3dr.rasterize(ver, tri, col, bg=bg)
    assert e.value.code == abi.SYN_ERR_INVALID and np.array_equal(bg, before)


# ---- C. every branch of the Phong vertex colours ----
def _light_on_device(name):
    from synergynet_amd import sim3dr
    if name == 'base':
        cfg, moved = dict(mc.RENDER_CFG), None
    elif name == 'grazing':
        cfg, moved = dict(mc.GRAZING_CFG), None
    else:
        cfg, moved = mc.light_cfg(name)
    pipe = sim3dr.RenderPipeline(**cfg)
    if moved is not None:
        pipe.update_light_pos(moved)
    ver, tri = mc.light_mesh(flat=name == 'grazing')
    return pipe.light(ver, tri), sim3dr.get_normal(ver, tri)


@pytest.mark.parametrize('name', ['base'] + list(mc.LIGHT_CASES) + ['grazing'])
def test_every_lighting_branch(emodel, mgold, oracle_lit, name):
    _poison_scratch(emodel)
    got, normal = _light_on_device(name)
    nkey = 'c_flat_normal' if name == 'grazing' else 'c_normal'
    assert normal.tobytes() == mgold[nkey].tobytes() == oracle_lit[nkey].tobytes()              # NaN row and zero signs included
    for what, want in (('fixture', mgold['c_light_' + name]), ('oracle', oracle_lit['c_light_' + name])):
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, what)
        err = np.nanmax(np.abs(got - want))
        print(f'{name} vs {what}: max abs error {err:.3g}')
        np.testing.assert_allclose(got, want, rtol=0, atol=mc.LIGHT_ATOL, equal_nan=True, err_msg=f'{name} vs {what}')
    want = oracle_lit['c_light_' + name]
    assert np.isnan(got[-1]).all() == (name != 'no_directional')                                # the isolated vertex
    if name == 'no_directional':
        assert (got == np.float32(0.75)).all()                  # no Lambert term and no specular term either
    if name == 'no_ambient':
        assert (want == 0).sum() >= 5 and (got[want == 0] == 0).all()                          # clipped away: exactly 0
    if name == 'off_axis':
        assert (want == 1).sum() >= 5 and (got[want == 1] == 1).all()                          # saturated: exactly 1
    if name == 'grazing':                                       # Lambert term exactly 0: np.where(cos != 0, ...) drops the specular sum
        np.testing.assert_allclose(got[:-1], 0.1, rtol=0, atol=mc.LIGHT_ATOL)


# ---- D. more than 254 faces; the face field at its limit ----
def test_render_batch_with_300_faces(emodel):
    import torch
    from oracle import sim3dr as osim
    from synergynet_amd import abi, sim3dr
    meshes, tri, _, img = mc.many_faces()
    F, _, n = meshes.shape
    assert F == mc.MANY_FACES > mc.FACE_LIMIT
    emodel.triangles = torch.from_numpy(np.ascontiguousarray(tri.T).astype(np.int64))
    mt = torch.from_numpy(meshes).cuda()
    # the device's own light, from ONE batched shade call into sentinel-filled buffers
    sim3dr._ensure_model_topology(emodel, n)
    _poison_scratch(emodel)
    normal = torch.full((F, n, 3), SENTINEL, dtype=torch.float32, device='cuda')
    light = torch.full((F, n, 3), SENTINEL, dtype=torch.float32, device='cuda')
    pipe = sim3dr.RenderPipeline(**mc.RENDER_CFG)
    with torch.cuda.device(emodel.device):
        abi.check(emodel._lib.syn_mesh_shade(emodel._h, mt.data_ptr(), F, 1, sim3dr._cfg16(pipe), normal.data_ptr(), light.data_ptr(),
                                             emodel._stream()))
    torch.cuda.synchronize()
    normal, light = normal.cpu().numpy(), light.cpu().numpy()
    assert np.isfinite(light).all() and (light != SENTINEL).all() and (normal != SENTINEL).all()
    assert np.array_equal(normal, np.stack([osim.get_normal(np.ascontiguousarray(m.T), tri) for m in meshes]))
    np.testing.assert_allclose(light, mc.oracle_lights(osim, meshes, tri, mc.RENDER_CFG), rtol=0, atol=mc.LIGHT_ATOL)
    # all 300 faces in order, byte for byte given those colours; the blend byte for byte
    overlay, res = sim3dr.render_batch(emodel, img, mt, alpha=mc.ALPHA)
    overlay, res = overlay.cpu().numpy(), res.cpu().numpy()
    want = mc.sequential(osim, meshes, tri, light, img)
    assert np.array_equal(overlay, want), f'{int((overlay != want).any(2).sum())} pixels differ'
    late = (want != mc.sequential(osim, meshes[:mc.FACE_LIMIT], tri, light[:mc.FACE_LIMIT], img)).any(2).mean()
    print(f'pixels the faces beyond the {mc.FACE_LIMIT}th change: {late:.3f}')
    assert late >= 0.05
    assert np.array_equal(res, osim.add_weighted(img, 1 - mc.ALPHA, overlay, mc.ALPHA))
    # the same picture from two calls: faces 0..253, then faces 254..299 onto the first overlay
    first, _ = sim3dr.render_batch(emodel, img, mt[:mc.FACE_LIMIT], alpha=mc.ALPHA)
    second, _ = sim3dr.render_batch(emodel, first, mt[mc.FACE_LIMIT:], alpha=mc.ALPHA)
    assert np.array_equal(second.cpu().numpy(), overlay)


def test_254_faces_in_one_call_and_255_refused(emodel, mgold, oracle_img):
    from synergynet_amd import abi
    meshes, tri, col, img = mc.many_faces()
    _poison_scratch(emodel)
    rc, got = _draw_faces(emodel, tri, meshes[:mc.FACE_LIMIT], col[:mc.FACE_LIMIT], img)
    assert rc == 0
    _same_image(got, 'd_f254', mgold, oracle_img)
    rc, got = _draw_faces(emodel, tri, meshes[:mc.FACE_LIMIT + 1], col[:mc.FACE_LIMIT + 1], img)
    assert rc == abi.SYN_ERR_INVALID and np.array_equal(got, img)


# ---- E. syn_add_weighted ----
@pytest.mark.parametrize('alpha,beta', mc.BLEND_WEIGHTS)
def test_add_weighted_ties_and_saturations(emodel, alpha, beta):
    import ctypes as C
    import torch
    from oracle import sim3dr as osim
    from synergynet_amd import abi
    assert mc.blend_edge_share(alpha, beta) >= 0.1
    for n in mc.BLEND_SIZES:
        a, b = mc.blend_inputs(n)
        at, bt = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        out = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device='cuda')                 # room behind the end: nothing may land there
        with torch.cuda.device(emodel.device):
            abi.check(emodel._lib.syn_add_weighted(emodel._h, at.data_ptr(), C.c_float(alpha), bt.data_ptr(), C.c_float(beta),
                                                   out.data_ptr(), n, emodel._stream()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = osim.add_weighted(a, alpha, b, beta)
        assert np.array_equal(got[:n], want), (n, alpha, beta, int((got[:n] != want).sum()))
        assert (got[n:] == 0xA5).all()
