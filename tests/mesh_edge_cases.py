"""Inputs, expected-output recipe and non-vacuity conditions of the mesh-consumer edge tests: syn_rasterize at zero depths, at the
empty-buffer threshold, with 1 / 3 / 4 channels, colours outside [0, 1] and up to 254 faces in one call; every branch of the Phong
vertex colours; render_batch beyond 254 faces; syn_add_weighted at its ties and its two saturations.  Everything is rebuilt from the
seeds below.  tests/golden/mesh_edges_golden.npz holds what the reference's own code gives on these inputs (written by
tests/golden/make_mesh_edges_golden.py); tests/test_mesh_edges_cpu.py holds the oracle to it and asserts the conditions of
`check_nonvacuity` on the oracle's output; tests/test_gpu_mesh_edges.py holds the device to both.  No test functions here."""
import numpy as np

from synergynet_amd import synth

F32 = np.float32
GRID_ROWS, GRID_COLS, HW = 9, 9, 48                            # 81 vertices, 128 triangles on a 48 x 48 frame
MANY_ROWS, MANY_COLS, MANY_HW = 4, 4, 32                       # 16 vertices, 18 triangles on a 32 x 32 frame
FACE_LIMIT = 254                                               # syn_rasterize's face field: 8 bits, 0 = nothing drawn
MANY_FACES = 300
ALPHA = 0.6

RENDER_CFG = dict(intensity_ambient=0.75, color_ambient=(1, 1, 1), intensity_directional=0.7, color_directional=(1, 1, 1),
                  intensity_specular=0.2, specular_exp=5, light_pos=(0, 0, 5), view_pos=(0, 0, 5))


def image(h, w, c, seed):
    """A frame of random bytes: what a draw leaves alone must still be there afterwards."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def grid_triangles():
    return synth.make_grid_topology(GRID_ROWS, GRID_COLS)


def grid_meshes(n_faces, seed):
    return synth.make_face_meshes(n_faces, GRID_ROWS, GRID_COLS, height=HW, width=HW, seed=seed)


def sequential(osim, meshes, tri, colors, bg, impl='oracle', reverse=False):
    """The reference's way with several faces (utils/render.py:39-42): one call per face, each with a fresh depth buffer, onto the
    same image.  meshes [F,3,N], colors [F,N,c]."""
    out = bg.copy()
    for f in range(meshes.shape[0]):
        out = osim.rasterize(np.ascontiguousarray(meshes[f].T), tri, np.ascontiguousarray(colors[f]), bg=out, reverse=reverse, impl=impl)
    return out


# ---- A. depth rule of syn_rasterize ----
PAIR_XY = ((1, 1), (9, 1), (1, 9))
PAIR_ORDERS = {'neg_first': ((0, 1, 2), (3, 4, 5)), 'pos_first': ((3, 4, 5), (0, 1, 2))}
PAIR_PROBE = (3, 3)                                            # (y, x) of a pixel well inside the triangle
RED, GREEN = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)


def coincident_pair():
    """Two triangles on the same three points: vertices 0-2 at depth -0.0 in red, vertices 3-5 at +0.0 in green.  `+0 > -0` is false,
    so whichever triangle is listed first keeps the pixels."""
    ver = np.array([(x, y, -0.0) for x, y in PAIR_XY] + [(x, y, 0.0) for x, y in PAIR_XY], dtype=F32)
    col = np.array([RED] * 3 + [GREEN] * 3, dtype=F32)
    tris = {k: np.array(v, dtype=np.int32) for k, v in PAIR_ORDERS.items()}
    return ver, tris, col, image(12, 12, 3, 5101)


def zero_soup(seed=5201, nv=300, nt=600, hw=HW):
    """600 triangles whose depths are all zero, signs drawn per vertex: every overlap is a tie, resolved by the order alone."""
    rng = np.random.default_rng(seed)
    ver = np.zeros((nv, 3), dtype=F32)
    ver[:, :2] = rng.uniform(-6, hw + 6, (nv, 2))
    ver[:, 2] = np.where(rng.random(nv) < 0.5, -0.0, 0.0)
    tri = rng.integers(0, nv, (nt, 3))
    near = rng.integers(0, nv - 2, nt // 2)
    tri[:nt // 2] = np.stack([near, near + 1, near + 2], 1)   # half from neighbouring vertex ids
    third = tri[::3]
    tri[::3] = rng.integers(0, nv, third.shape)               # every third fully random
    col = rng.uniform(0, 1, (nv, 3)).astype(F32)
    return ver, np.ascontiguousarray(tri, dtype=np.int32), col, image(hw, hw, 3, seed + 1)


EMPTY = F32(-1e8)                                              # what a fresh depth buffer holds (Sim3DR.py:23)


def threshold_pair():
    """One triangle exactly AT the empty buffer's depth and one a single float32 step above it.  The interpolated depth
    w0*d + w1*d + w2*d rounds to either side of -1e8 from pixel to pixel, and only `> -1e8` is drawn."""
    above = np.nextafter(EMPTY, F32(0))
    ver = np.array([(2.3, 1.7, EMPTY), (21.6, 3.2, EMPTY), (4.1, 20.9, EMPTY),
                    (25.2, 24.4, above), (45.7, 27.1, above), (28.3, 46.2, above)], dtype=F32)
    tri = np.array([(0, 1, 2), (3, 4, 5)], dtype=np.int32)
    col = np.array([RED] * 3 + [GREEN] * 3, dtype=F32)
    return ver, tri, col, image(HW, HW, 3, 5301)


def inside_mask(ver, tri_row, h, w):
    """Pixels the rasteriser's inside test accepts for one triangle (rasterize_kernel.cpp:26-82 in float32)."""
    (p0x, p0y), (p1x, p1y), (p2x, p2y) = (ver[i, :2] for i in tri_row)
    ys, xs = np.mgrid[0:h, 0:w]
    px, py = xs.astype(F32), ys.astype(F32)
    v0x, v0y, v1x, v1y, v2x, v2y = p2x - p0x, p2y - p0y, p1x - p0x, p1y - p0y, px - p0x, py - p0y
    dot00, dot01, dot02 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v0x * v2x + v0y * v2y
    dot11, dot12 = v1x * v1x + v1y * v1y, v1x * v2x + v1y * v2y
    den = dot00 * dot11 - dot01 * dot01
    inv = F32(0) if den == 0 else F32(1) / den
    u, v = (dot11 * dot02 - dot01 * dot12) * inv, (dot00 * dot12 - dot01 * dot02) * inv
    return (u >= 0) & (v >= 0) & (u + v < 1)


STACK_SEED = 5403


def stacked_faces():
    """Three faces for ONE syn_rasterize call.  synth.make_face_meshes puts face f 20 f deeper than face 0, so face 2 lies entirely
    behind face 0; it still overwrites face 0 wherever it covers, because every face starts from a fresh depth buffer."""
    meshes = grid_meshes(3, STACK_SEED)
    col = np.random.default_rng(STACK_SEED + 1).uniform(0, 1, (3, meshes.shape[2], 3)).astype(F32)
    return meshes, grid_triangles(), col, image(HW, HW, 3, STACK_SEED + 2)


def cover(osim, mesh, tri, h, w):
    """bool [h,w]: the pixels one face draws."""
    ver = np.ascontiguousarray(mesh.T)
    one = np.ones((ver.shape[0], 1), dtype=F32)
    return osim.rasterize(ver, tri, one, bg=np.zeros((h, w, 1), np.uint8))[:, :, 0] != 0      # 254 or 255


# ---- B. channels and colour conversion ----
CHANNELS = (1, 3, 4)
FLAT_COLOURS = ((-0.3, 180), (1.2, 50), (1.7, 177), (-1.01, 255), (2.5, 125))     # (255 * p) through int32, low byte kept


def channel_case(c):
    """One grid face with colours from [-0.6, 1.9) and a frame of c channels."""
    ver = np.ascontiguousarray(grid_meshes(1, 5501)[0].T)
    col = np.random.default_rng(5502).uniform(-0.6, 1.9, (ver.shape[0], 4)).astype(F32)
    return ver, grid_triangles(), np.ascontiguousarray(col[:, :c]), image(HW, HW, c, 5503 + c)


def flat_case(value):
    """The triangle of `coincident_pair` alone, one channel, one colour value at its three corners."""
    ver = np.array([(x, y, 0.5) for x, y in PAIR_XY], dtype=F32)
    return ver, np.array([(0, 1, 2)], dtype=np.int32), np.full((3, 1), value, dtype=F32), image(12, 12, 1, 5510)


# ---- C. every branch of the Phong vertex colours ----
LIGHT_CASES = {                                                # overrides of RENDER_CFG
    'no_directional': dict(intensity_directional=0),           # ... which takes the specular term with it
    'no_ambient': dict(intensity_ambient=0),
    'no_specular': dict(intensity_specular=0),
    'exp1': dict(specular_exp=1),
    'exp2': dict(specular_exp=2),
    'exp3': dict(specular_exp=3),
    'exp8': dict(specular_exp=8),
    'coloured': dict(color_ambient=(0.9, 0.5, 0.1), color_directional=(0.2, 0.7, 1.0), intensity_ambient=0.9, intensity_directional=0.8),
    'off_axis': dict(view_pos=(-2, 5, 2)),                     # + update_light_pos(LIGHT_MOVES['off_axis'])
    'behind': dict(light_pos=(0, 0, -5), intensity_ambient=0.1, intensity_specular=0.9),
}
LIGHT_MOVES = {'off_axis': (4, -3, 1)}
EXPONENT_CASES = ('exp1', 'exp2', 'exp3', 'exp8')
GRAZING_CFG = dict(RENDER_CFG, light_pos=(3, 0, 0), view_pos=(-3, 0, 0), intensity_ambient=0.1, intensity_specular=0.9)
LIGHT_ATOL = 1e-6                                              # float32 power (numpy) against an exactly rounded product: one ulp below 1


def light_cfg(name):
    """(constructor arguments, position for update_light_pos or None)."""
    return dict(RENDER_CFG, **LIGHT_CASES[name]), LIGHT_MOVES.get(name)


def final_cfg(name):
    """The configuration in force after update_light_pos: what a pipeline without that method is constructed with."""
    cfg, moved = light_cfg(name)
    return dict(cfg, light_pos=moved) if moved is not None else cfg


def light_mesh(flat=False):
    """One grid face plus an isolated vertex (no triangle: NaN normal) at the face's centroid; flat=True: every depth 7.0.
    The face is folded along its middle column, the right half laid back over the left one a little deeper, so the normals of the
    right half point towards the light of RENDER_CFG and those of the left half away from it; the relief of the left half is
    flattened to a quarter.  On the unfolded face the Lambert term of RENDER_CFG has one sign throughout: either ambient + Lambert
    saturate every colour at 1, or no Lambert term is there to be switched off.  The specular term of RENDER_CFG is visible where
    the Lambert term is clipped away and the normal is close to the axis -- the flattened back-facing half."""
    ver = grid_meshes(1, 5601)[0].T.copy()
    x, z = (ver[:, k].reshape(GRID_ROWS, GRID_COLS) for k in (0, 2))
    mid = GRID_COLS // 2
    z[:, :mid + 1] = z.mean() + 0.25 * (z[:, :mid + 1] - z.mean())
    x[:, mid + 1:] = 2 * x[:, mid:mid + 1] - x[:, mid + 1:]
    z[:, mid + 1:] -= 6.0
    ver = np.ascontiguousarray(np.concatenate([ver, ver.mean(0, keepdims=True)], 0), dtype=F32)
    if flat:
        ver[:, 2] = 7.0
    return ver, grid_triangles()


def lambert_term(osim, ver, tri, cfg):
    """The unclipped cosine between normal and light direction, as the oracle's vertex_colours forms it (lighting.py:46-50)."""
    box = ver.copy()
    box -= box.min(0)[None, :]
    box /= box.max()
    box *= 2
    box -= box.max(0)[None, :] / 2
    return np.sum(osim.get_normal(ver, tri) * osim._unit_rows(osim._row(cfg['light_pos']) - box), axis=1)


# ---- D. more than 254 faces ----
def many_faces():
    """300 small faces for render_batch, per-vertex colours for the first 254 of them in one syn_rasterize call."""
    meshes = synth.make_face_meshes(MANY_FACES, MANY_ROWS, MANY_COLS, height=MANY_HW, width=MANY_HW, seed=5701)
    tri = synth.make_grid_topology(MANY_ROWS, MANY_COLS)
    col = np.random.default_rng(5702).uniform(0, 1, (FACE_LIMIT + 1, meshes.shape[2], 3)).astype(F32)
    return meshes, tri, col, image(MANY_HW, MANY_HW, 3, 5703)


def oracle_lights(osim, meshes, tri, cfg):
    return np.stack([osim.RenderPipeline(**cfg).light(np.ascontiguousarray(m.T), tri) for m in meshes])


# ---- E. syn_add_weighted ----
BLEND_SIZES = (1, 255, 257, 3 * 37 * 41)
BLEND_WEIGHTS = ((0.5, 0.5), (1.0, 1.0), (1.5, -0.5))          # ties on odd sums | saturation at 255 | clipping at 0


def blend_inputs(n):
    rng = np.random.default_rng(5800 + n)
    return rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)


def blend_edge_share(alpha, beta):
    """Share of all elements (the four sizes together) on which a weight pair meets the edge it is there for."""
    a, b = (np.concatenate(x).astype(np.float64) for x in zip(*(blend_inputs(n) for n in BLEND_SIZES)))
    v = a * alpha + b * beta
    if (alpha, beta) == (0.5, 0.5):
        return float((v % 1 == 0.5).mean())
    return float((v > 255).mean()) if beta > 0 else float((v < 0).mean())


# ---- expected outputs: one recipe for the generator (impl='ref' + the reference's lighting) and the tests (impl='oracle') ----
def expected_images(osim, impl='oracle'):
    out = {}
    ver, tris, col, bg = coincident_pair()
    for order, tri in tris.items():
        for rev in (0, 1):
            out[f'a1_{order}_rev{rev}'] = osim.rasterize(ver, tri, col, bg=bg.copy(), reverse=bool(rev), impl=impl)
    ver, tri, col, bg = zero_soup()
    for rev in (0, 1):
        out[f'a2_rev{rev}'] = osim.rasterize(ver, tri, col, bg=bg.copy(), reverse=bool(rev), impl=impl)
    ver, tri, col, bg = threshold_pair()
    out['a3'] = osim.rasterize(ver, tri, col, bg=bg.copy(), impl=impl)
    meshes, tri, col, bg = stacked_faces()
    out['a4'] = sequential(osim, meshes, tri, col, bg, impl=impl)
    for c in CHANNELS:
        ver, tri, col, bg = channel_case(c)
        out[f'b_c{c}'] = osim.rasterize(ver, tri, col, bg=bg.copy(), impl=impl)
    for k, (value, _) in enumerate(FLAT_COLOURS):
        ver, tri, col, bg = flat_case(value)
        out[f'b_flat{k}'] = osim.rasterize(ver, tri, col, bg=bg.copy(), impl=impl)
    meshes, tri, col, bg = many_faces()
    out['d_f254'] = sequential(osim, meshes[:FACE_LIMIT], tri, col[:FACE_LIMIT], bg, impl=impl)
    return out


def expected_lights(osim, impl='oracle', light_fn=None):
    """light_fn(name or 'grazing', constructor cfg, moved light or None, vertices, triangles) -> [nver,3]; default: the oracle's."""
    if light_fn is None:
        light_fn = lambda name, cfg, moved, ver, tri: osim.RenderPipeline(impl=impl, **(dict(cfg, light_pos=moved) if moved is not None else cfg)).light(ver, tri)
    ver, tri = light_mesh()
    out = {'c_normal': osim.get_normal(ver, tri, impl=impl), 'c_light_base': light_fn('base', dict(RENDER_CFG), None, ver, tri)}
    for name in LIGHT_CASES:
        cfg, moved = light_cfg(name)
        out['c_light_' + name] = light_fn(name, cfg, moved, ver, tri)
    ver, tri = light_mesh(flat=True)
    out['c_flat_normal'] = osim.get_normal(ver, tri, impl=impl)
    out['c_light_grazing'] = light_fn('grazing', dict(GRAZING_CFG), None, ver, tri)
    return out


def check_nonvacuity(osim, img, lit):
    """The conditions under which the cases test what they are there for, on the ORACLE's output (img = expected_images(osim),
    lit = expected_lights(osim)).  Raises AssertionError; returns the measured figures."""
    m = {}
    # A1: the first listed triangle keeps the pixel, whatever the signs
    ver, tris, col, bg = coincident_pair()
    y, x = PAIR_PROBE
    for order, first in (('neg_first', RED), ('pos_first', GREEN)):
        for rev in (0, 1):
            got = img[f'a1_{order}_rev{rev}'][11 - y if rev else y, x]
            assert tuple(got) == tuple(int(255 * v) for v in first), (order, rev, got)
    # A2: the sign of a zero never decides; the order does
    ver, tri, col, bg = zero_soup()
    for z in (0.0, -0.0):
        same = ver.copy()
        same[:, 2] = z
        assert np.array_equal(osim.rasterize(same, tri, col, bg=bg.copy()), img['a2_rev0']), z
    assert np.signbit(ver[:, 2]).any() and not np.signbit(ver[:, 2]).all() and (ver[:, 2] == 0).all()
    back = osim.rasterize(ver, np.ascontiguousarray(tri[::-1]), col, bg=bg.copy())
    m['a2_covered'] = float((img['a2_rev0'] != bg).any(2).mean())
    m['a2_order_matters'] = float((back != img['a2_rev0']).any(2).mean())
    assert m['a2_order_matters'] > 0.5, m
    # A3: each triangle is drawn on some of its pixels and not on others
    ver, tri, col, bg = threshold_pair()
    drawn = (img['a3'] != bg).any(2)
    for k in range(2):
        ins = inside_mask(ver, tri[k], HW, HW)
        m[f'a3_tri{k}_inside'], m[f'a3_tri{k}_drawn'] = int(ins.sum()), int((ins & drawn).sum())
    for k in range(2):                                         # at least a handful of pixels on either side of the threshold
        assert m[f'a3_tri{k}_drawn'] >= 5 and m[f'a3_tri{k}_inside'] - m[f'a3_tri{k}_drawn'] >= 5, m
    assert not (drawn & ~inside_mask(ver, tri[0], HW, HW) & ~inside_mask(ver, tri[1], HW, HW)).any()
    # A4: face 2 is behind face 0 everywhere and still ends up on top of it
    meshes, tri, col, bg = stacked_faces()
    assert meshes[2, 2].max() < meshes[0, 2].min()
    c0, c2 = cover(osim, meshes[0], tri, HW, HW), cover(osim, meshes[2], tri, HW, HW)
    alone = sequential(osim, meshes[2:], tri, col[2:], bg)
    both = c0 & c2
    assert np.array_equal(img['a4'][both], alone[both])
    m['a4_face0_pixels'], m['a4_overwritten'] = int(c0.sum()), int(both.sum())
    assert both.sum() >= 0.1 * c0.sum(), m
    # B: the frame is partly covered and colours outside [0, 1] reach the pixels
    for c in CHANNELS:
        ver, tri, col, bg = channel_case(c)
        covered = cover(osim, ver.T, tri, HW, HW)
        clipped = osim.rasterize(ver, tri, np.clip(col, 0, 1), bg=bg.copy())
        m[f'b_c{c}_covered'] = float(covered.mean())
        m[f'b_c{c}_wrapped'] = float((clipped != img[f'b_c{c}']).any(2)[covered].mean())
        assert 0.1 <= covered.mean() <= 0.5 and m[f'b_c{c}_wrapped'] >= 0.25, m
        assert np.array_equal(img[f'b_c{c}'][~covered], bg[~covered])
    for k, (_, byte) in enumerate(FLAT_COLOURS):
        assert int(img[f'b_flat{k}'][PAIR_PROBE][0]) == byte, (k, img[f'b_flat{k}'][PAIR_PROBE])
    # C: every configuration moves the light by more than the bar could hide
    base = lit['c_light_base']
    assert np.isnan(lit['c_normal'][-1]).all() and np.isfinite(lit['c_normal'][:-1]).all()
    for name in LIGHT_CASES:
        got = lit['c_light_' + name]
        fin = np.isfinite(got) & np.isfinite(base)
        assert fin[:-1].all()
        assert np.isnan(got[-1]).all() == (name != 'no_directional'), name
        step = 1e-4 if name in EXPONENT_CASES else 0.05
        m[f'c_{name}_moved'] = float((np.abs(got - base)[fin] > step).mean())
        assert m[f'c_{name}_moved'] >= 0.25, (name, m)
    assert (lit['c_light_no_directional'] == F32(0.75)).all()
    m['c_no_ambient_zeros'] = float((lit['c_light_no_ambient'] == 0).mean())
    m['c_off_axis_ones'] = float((lit['c_light_off_axis'] == 1).mean())
    assert min(m['c_no_ambient_zeros'], m['c_off_axis_ones']) * base.size >= 5, m       # a handful of exact 0s and exact 1s
    ver, tri = light_mesh()
    lam = lambert_term(osim, ver, tri, final_cfg('behind'))[:-1]
    lam0 = lambert_term(osim, ver, tri, RENDER_CFG)[:-1]
    m['c_behind_sign_flipped'] = float((np.sign(lam) == -np.sign(lam0)).mean())
    assert m['c_behind_sign_flipped'] >= 0.9, m
    # the cos != 0 branch: a Lambert term of exactly 0 at every vertex that has a normal
    ver, tri = light_mesh(flat=True)
    lam = lambert_term(osim, ver, tri, GRAZING_CFG)[:-1]
    assert (lam == 0).all() and (np.abs(lit['c_flat_normal'][:-1]) == np.array([0, 0, 1], F32)).all()
    assert (lit['c_light_grazing'][:-1] == F32(0.1)).all() and np.isnan(lit['c_light_grazing'][-1]).all()
    # D: the faces beyond the 254th change the picture
    meshes, tri, col, bg = many_faces()
    lights = oracle_lights(osim, meshes, tri, RENDER_CFG)
    all_faces = sequential(osim, meshes, tri, lights, bg)
    first = sequential(osim, meshes[:FACE_LIMIT], tri, lights[:FACE_LIMIT], bg)
    m['d_changed_by_late_faces'] = float((all_faces != first).any(2).mean())
    assert m['d_changed_by_late_faces'] >= 0.05, m
    # E: every weight pair meets its edge
    for alpha, beta in BLEND_WEIGHTS:
        m[f'e_{alpha}_{beta}'] = blend_edge_share(alpha, beta)
        assert m[f'e_{alpha}_{beta}'] >= 0.1, m
    return m
