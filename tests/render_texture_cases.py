"""Inputs and CPU definitions of the per-pixel texture-mapping tests.  tests/golden/render_texture_golden.npz is written by
tests/golden/make_render_texture_golden.py from exactly these inputs (rebuilt from the seeds a fixture case stores) with the
reference's own compiled `_render_texture_core` (oracle/_ref/libsim3dr_ref.so, Sim3DR/lib/rasterize_kernel.cpp:353-458);
`texture_rule` is the order-free numpy statement of that function the GPU tests use where no fixture exists."""
import ctypes as C
import types

import numpy as np

import visibility_cases as vc

REF_SYMBOL = '_Z20_render_texture_corePfS_PiS_S_S0_S_iiiiiiiiii'   # _render_texture_core(float*, float*, int*, float*, float*, int*, float*, 10 x int)
NEAREST, BILINEAR = 0, 1
INIT_DEPTH = np.float32(-1e8)
SOUP_TEX_SEED, SOUP_TEX_SHAPE, SOUP_FILL = 5207, (16, 20, 4), -5.0
SOUP_VARIANTS = ((3, NEAREST), (3, BILINEAR), (1, NEAREST), (1, BILINEAR))          # (image channels, mapping type)
SMALL_TEX_SEED, SHIFT_XY, SHIFT_DEPTH = 5311, (3.0, 2.0), 0.5
FULL_TEX_HW, FULL_SMALL_FRAME = 256, 64


def ref_render_texture(image, vertices, triangles, texture, tex_coords, tex_triangles, depth, h, w, c, mapping_type):
    """The reference's own function, in place on the caller's image [h,w,c] and depth [h,w]."""
    fn = getattr(C.CDLL(vc.REF_LIB), REF_SYMBOL)
    fn.restype, fn.argtypes = None, [C.c_void_p] * 7 + [C.c_int] * 10
    for a, dt in ((image, np.float32), (vertices, np.float32), (triangles, np.int32), (texture, np.float32), (tex_coords, np.float32),
                  (tex_triangles, np.int32), (depth, np.float32)):
        assert a.dtype == dt and a.flags.c_contiguous
    th, tw, tc = texture.shape
    assert image.size == h * w * c and depth.size == h * w and c <= tc and tex_coords.shape[1] == 3
    assert tex_triangles.shape == triangles.shape and tex_triangles.max() < tex_coords.shape[0] and triangles.max() < tex_coords.shape[0]
    fn(image.ctypes.data, vertices.ctypes.data, triangles.ctypes.data, texture.ctypes.data, tex_coords.ctypes.data, tex_triangles.ctypes.data,
       depth.ctypes.data, vertices.shape[0], tex_coords.shape[0], triangles.shape[0], h, w, c, th, tw, tc, mapping_type)


def _clamp(x, hi):
    """x = x > hi ? hi : x; x = x >= 0 ? x : 0 -- the reference's max(min()) for every finite value; NaN becomes 0."""
    x = np.where(x > hi, hi, x)
    return np.where(x >= 0, x, np.float32(0))


def sample_texture(texture, x, y, c, mapping_type):
    """float32 [n,c]: the texture [th,tw,tc] (any dtype, read as float32) at float32 coordinates (x, y), clamped as above; nearest =
    round half away from zero, bilinear in the operation order of rasterize_kernel.cpp:445-447."""
    f = np.float32
    th, tw, _ = texture.shape
    x, y = _clamp(x.astype(f), f(tw - 1)), _clamp(y.astype(f), f(th - 1))
    fx, fy = np.floor(x), np.floor(y)
    xd, yd = x - fx, y - fy
    if mapping_type == NEAREST:
        rx, ry = (fx + (xd >= 0.5)).astype(int), (fy + (yd >= 0.5)).astype(int)          # x, y >= 0 here
        return texture[ry, rx, :c].astype(f)
    x0, x1, y0, y1 = fx.astype(int), np.ceil(x).astype(int), fy.astype(int), np.ceil(y).astype(int)
    ul, ur, dl, dr = (texture[a, b, :c].astype(f) for a, b in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    xd, yd = xd[:, None], yd[:, None]
    out = ul * (1 - xd) * (1 - yd) + ur * xd * (1 - yd) + dl * (1 - xd) * yd + dr * xd * yd
    assert out.dtype == f
    return out


def texture_rule(image, depth, vertices, triangles, texture, tex_coords, tex_triangles, mapping_type, state=None):
    """The order-free statement of _render_texture_core, in place on image [h,w,c] and depth [h,w] (float32): per pixel, among the
    candidates -- triangles whose box (ceil of the minimum .. floor of the maximum, clipped to the frame) holds the pixel and that
    contain it OR the pixel lies on the two-pixel frame border (:418) -- with a depth greater than the CALLER's buffer, the greatest
    depth wins, the earliest index among equals (+0 == -0).  Walks the triangles LAST TO FIRST replacing on >=.  The winner's texture
    coordinate reads x through tex_triangles and y through the MESH triangle's indices (:393-398), is clamped (NaN -> 0) and sampled.
    `state` = (initial depth, won mask) carries over to an EARLIER mesh drawn into the same buffers (shared z-buffer: call for the
    meshes last to first); returns it."""
    f = np.float32
    h, w, c = image.shape
    init, won = state if state is not None else (depth.copy(), np.zeros((h, w), bool))
    with np.errstate(all='ignore'):
        for i in range(triangles.shape[0] - 1, -1, -1):
            p = vertices[triangles[i]]
            (p0x, p0y, d0), (p1x, p1y, d1), (p2x, p2y, d2) = p
            if not np.isfinite(p[:, :2]).all():
                continue                                       # weights and depth are NaN: never wins; the reference's box is undefined
            x0, x1 = max(int(np.ceil(p[:, 0].min())), 0), min(int(np.floor(p[:, 0].max())), w - 1)
            y0, y1 = max(int(np.ceil(p[:, 1].min())), 0), min(int(np.floor(p[:, 1].max())), h - 1)
            if x1 < x0 or y1 < y0:
                continue
            ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
            px, py = xs.astype(f), ys.astype(f)
            v0x, v0y, v1x, v1y, v2x, v2y = p2x - p0x, p2y - p0y, p1x - p0x, p1y - p0y, px - p0x, py - p0y
            dot00, dot01, dot02 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v0x * v2x + v0y * v2y
            dot11, dot12 = v1x * v1x + v1y * v1y, v1x * v2x + v1y * v2y
            den = dot00 * dot11 - dot01 * dot01
            inv = f(0) if den == 0 else f(1) / den
            u, v = (dot11 * dot02 - dot01 * dot12) * inv, (dot00 * dot12 - dot01 * dot02) * inv
            w0, w1, w2 = f(1) - u - v, v, u
            dep = w0 * d0 + w1 * d1 + w2 * d2
            sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            border = (xs < 2) | (xs > w - 3) | (ys < 2) | (ys > h - 3)
            take = (border | ((u >= 0) & (v >= 0) & (u + v < 1))) & (dep > init[sl]) & (~won[sl] | (dep >= depth[sl]))
            if not take.any():
                continue
            tt, mt = tex_triangles[i], triangles[i]
            tx = tex_coords[tt[0], 0] * w0 + tex_coords[tt[1], 0] * w1 + tex_coords[tt[2], 0] * w2
            ty = tex_coords[mt[0], 1] * w0 + tex_coords[mt[1], 1] * w1 + tex_coords[mt[2], 1] * w2
            assert tx.dtype == f and dep.dtype == f
            depth[sl][take] = dep[take]
            image[sl][take] = sample_texture(texture, tx[take], ty[take], c, mapping_type)
            won[sl] |= take
    return init, won


def rule_shared(image, depth, meshes, triangles, texture, tex_coords, tex_triangles, mapping_type):
    """All meshes ([F,nver,3]) into ONE image and depth buffer = the reference called once per mesh in order."""
    state = None
    for f in range(meshes.shape[0] - 1, -1, -1):
        state = texture_rule(image, depth, meshes[f], triangles, texture, tex_coords, tex_triangles, mapping_type, state)
    return state[1]


# ---- soup: visibility_cases.build_soup() with a small texture, coordinates reaching outside it, separate tex_triangles ----
def build_soup_case(seed=vc.SOUP_SEED, hw=vc.SOUP_HW, ntri=400, tex_seed=SOUP_TEX_SEED):
    ver, tri, (depth, _, _) = vc.build_soup(seed, hw, ntri)               # initial depth 0.5 over the right half
    rng = np.random.default_rng(tex_seed)
    th, tw, tc = SOUP_TEX_SHAPE
    tex_nver = ver.shape[0] + 11
    texture = rng.uniform(0, 255, SOUP_TEX_SHAPE).astype(np.float32)
    coords = np.stack([rng.uniform(-5, tw + 4, tex_nver), rng.uniform(-5, th + 4, tex_nver), rng.uniform(-1, 1, tex_nver)], 1)
    coords[::3, :2] = np.rint(coords[::3, :2])                            # a third exactly on texels (and on the clamp's bounds)
    tex_tri = np.ascontiguousarray(rng.permutation(tri.reshape(-1)).reshape(-1, 3), dtype=np.int32)
    assert not np.array_equal(tex_tri, tri)
    return dict(hw=hw, vertices=ver, triangles=tri, depth=depth, texture=texture, tex_coords=np.ascontiguousarray(coords, dtype=np.float32),
                tex_triangles=tex_tri)


def soup_image(case, c):
    return np.full((case['hw'], case['hw'], c), SOUP_FILL, np.float32)


# ---- meshes: the grids of visibility_cases with the texture coordinates of the model's UV asset ----
def uv_coords(assets, th, tw, kept=False):
    from synergynet_amd import sim3dr
    stub = types.SimpleNamespace(param_pack=types.SimpleNamespace(uv_vert=assets['uv_vert'], keep_ind=assets['keep_ind']))
    return sim3dr.uv_tex_coords(stub, th, tw, kept=kept)


def byte_texture(seed, th, tw, c=3):
    """uint8 [th,tw,c]: smooth enough to show where it lands, every byte value present."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:th, 0:tw]
    base = np.stack([(xx * 255) // max(tw - 1, 1), (yy * 255) // max(th - 1, 1), ((xx + yy) * 8) % 256], -1)[:, :, :c]
    return ((base + rng.integers(0, 64, (th, tw, c))) % 256).astype(np.uint8)


def overlapping_pair(meshes):
    """[2,3,N]: the frontal face and the turned one shifted a few pixels and 0.5 deeper, so that they overlap."""
    second = meshes[1].copy()
    second[0] += np.float32(SHIFT_XY[0]); second[1] += np.float32(SHIFT_XY[1]); second[2] += np.float32(SHIFT_DEPTH)
    return np.ascontiguousarray(np.stack([meshes[0], second]))


def scaled(meshes, hw, frame):
    """[F,3,N] meshes of a hw-pixel frame brought to a `frame`-pixel one (x and y in float32; depth as it is)."""
    out = meshes.copy()
    out[:, :2] *= np.float32(frame / hw)
    return out


def interleaved(meshes):
    """[F,3,N] -> [F,N,3], the reference's layout."""
    return np.ascontiguousarray(np.transpose(meshes, (0, 2, 1)))


def fresh(h, w, c, lead=()):
    return np.zeros(tuple(lead) + (h, w, c), np.float32), np.full(tuple(lead) + (h, w), INIT_DEPTH, np.float32)


def ref_per_face(meshes, tri, texture, coords, h, w, c, mapping_type):
    """shared = 0 by the reference: every mesh into planes of its own."""
    image, depth = fresh(h, w, c, lead=(meshes.shape[0],))
    for f, v in enumerate(interleaved(meshes)):
        ref_render_texture(image[f], v, tri, texture, coords, tri, depth[f], h, w, c, mapping_type)
    return image, depth


def ref_shared(meshes, tri, texture, coords, h, w, c, mapping_type):
    """shared = 1 by the reference: one call per mesh, in order, on the same image and depth buffer."""
    image, depth = fresh(h, w, c)
    for v in interleaved(meshes):
        ref_render_texture(image, v, tri, texture, coords, tri, depth, h, w, c, mapping_type)
    return image, depth


def small_variants(case):
    """name -> (meshes [2,3,N], float32 texture, tex_coords, image channels, mapping type, shared) of the `small` fixture case."""
    pair = overlapping_pair(case['meshes'])
    t64 = byte_texture(SMALL_TEX_SEED, 64, 64).astype(np.float32)
    t256 = byte_texture(SMALL_TEX_SEED + 1, 256, 256).astype(np.float32)
    c64, c256 = uv_coords(case['assets'], 64, 64), uv_coords(case['assets'], 256, 256)
    return dict(faces64=(case['meshes'], t64, c64, 3, BILINEAR, False),
                faces256=(case['meshes'], t256, c256, 1, NEAREST, False),
                shared256=(pair, t256, c256, 3, BILINEAR, True),
                shared256_swapped=(np.ascontiguousarray(pair[::-1]), t256, c256, 3, BILINEAR, True),
                shared64=(pair, t64, c64, 3, NEAREST, True))
