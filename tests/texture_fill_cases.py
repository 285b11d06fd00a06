"""The definition of the push-pull completion of UV textures (syn_texture_fill, sim3dr.fill_texture) in numpy, and the seeded cases
the CPU and GPU tests share.  Integer arithmetic only: any tiling and any reduction order must reproduce `fill` byte for byte.

  level 0   w0 = (mask != 0), c0 = tex * w0;  merge: the T views collapse into one texture, w0 = sum_t (mask_t != 0),
            c0 = sum_t tex_t * (mask_t != 0)
  push      level l+1 is ceil(H_l/2) x ceil(W_l/2); w and c are the plain sums over the up-to-four children that exist
  own       where w > 0: floor((2c + w) / (2w)) per channel (round half up)
  pull      from the 1x1 level down: V = own where w > 0, elsewhere (9 V[py,px] + 3 V[py,nx] + 3 V[ny,px] + V[ny,nx] + 8) >> 4 on the
            level above, py = y >> 1, ny = clamp(py + (y odd ? +1 : -1), 0, H_{l+1} - 1), px / nx likewise
  output    V_0; a texture without a valid texel is all 0."""
import numpy as np


def level0(tex, mask, merge=False):
    """(c0 uint64 [T',H,W,ch], w0 uint64 [T',H,W]) of tex uint8 [T,H,W,ch], mask uint8 [T,H,W]; T' = 1 with merge."""
    v = (mask != 0)
    c = tex.astype(np.uint64) * v[..., None].astype(np.uint64)
    w = v.astype(np.uint64)
    return (c.sum(0, keepdims=True), w.sum(0, keepdims=True)) if merge else (c, w)


def push(a, order='block'):
    """One push step on [H,W,...] sums: the plain sum over the up-to-four children that exist.  `order`: 'block' adds the four
    children at once, 'rows' adds row pairs first and column pairs second, 'cols' the other way round."""
    H, W = a.shape[:2]
    p = np.zeros(((H + 1) // 2 * 2, (W + 1) // 2 * 2) + a.shape[2:], a.dtype)
    p[:H, :W] = a
    if order == 'block':
        return p.reshape((p.shape[0] // 2, 2, p.shape[1] // 2, 2) + a.shape[2:]).sum((1, 3), dtype=a.dtype)
    if order == 'rows':
        r = p[0::2] + p[1::2]
        return r[:, 0::2] + r[:, 1::2]
    assert order == 'cols'
    r = p[:, 0::2] + p[:, 1::2]
    return r[0::2] + r[1::2]


def pyramid(c0, w0, order='block'):
    """Lists of the sums of one texture from level 0 up to the 1x1 level."""
    cs, ws = [c0], [w0]
    while ws[-1].shape != (1, 1):
        cs.append(push(cs[-1], order))
        ws.append(push(ws[-1], order))
    return cs, ws


def own_value(c, w):
    """floor((2c + w) / (2w)) where w > 0 (0 elsewhere), uint64 [H,W,ch]."""
    w = w[..., None]
    return np.where(w > 0, (2 * c + w) // np.maximum(2 * w, 1), 0).astype(np.uint64)


def _parents(n, n_up):
    y = np.arange(n)
    p = y >> 1
    return p, np.clip(p + np.where(y & 1, 1, -1), 0, n_up - 1)


def pull(cs, ws):
    V = None
    for c, w in zip(reversed(cs), reversed(ws)):
        own = own_value(c, w)
        if V is not None:
            (py, ny), (px, nx) = _parents(w.shape[0], V.shape[0]), _parents(w.shape[1], V.shape[1])
            up = (9 * V[py][:, px] + 3 * V[py][:, nx] + 3 * V[ny][:, px] + V[ny][:, nx] + 8) >> 4
            own = np.where(w[..., None] > 0, own, up)
        V = own
    assert V.max(initial=0) <= 255
    return V.astype(np.uint8)


def fill(tex, mask, merge=False, order='block'):
    """The definition.  tex uint8 [H,W,ch] or [T,H,W,ch], mask uint8 of the matching shape; returns uint8 of tex's shape, or [H,W,ch]
    with merge (which takes [T,H,W,ch])."""
    tex, mask = np.asarray(tex), np.asarray(mask)
    assert tex.dtype == np.uint8 and mask.dtype == np.uint8 and tex.ndim in (3, 4) and mask.shape == tex.shape[:-1]
    t4, m4 = (tex, mask) if tex.ndim == 4 else (tex[None], mask[None])
    c0, w0 = level0(t4, m4, merge)
    out = np.stack([pull(*pyramid(c0[t], w0[t], order)) for t in range(c0.shape[0])])
    return out[0] if merge or tex.ndim == 3 else out


# ---- seeded cases ----
def random_case(seed, T, H, W, ch, valid):
    """tex uint8 [T,H,W,ch] (every texel random, also the invalid ones: they must not leak), mask uint8 [T,H,W] with a share `valid`
    of nonzero texels whose values mix 1, 255 and others."""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (T, H, W, ch), dtype=np.uint8)
    mask = np.where(rng.uniform(0, 1, (T, H, W)) < valid, rng.choice(np.array([1, 255, 7, 128], np.uint8), (T, H, W)), 0).astype(np.uint8)
    return tex, mask


# (name, T, H, W, ch, share of valid texels): the smallest sizes at which a tiling by 64 x 64 can go wrong -- below one tile, exactly
# one, a one-texel ring across ragged tiles, several tiles, non-square, and every channel count
SIZE_CASES = [('1x1', 1, 1, 1, 3, 1.0), ('5x1', 1, 5, 1, 3, 0.5), ('1x7', 2, 1, 7, 4, 0.5), ('37x53', 1, 37, 53, 3, 0.3),
              ('64x64', 1, 64, 64, 1, 0.2), ('65x130', 1, 65, 130, 3, 0.1), ('128x192', 1, 128, 192, 4, 0.05),
              ('256x256_T3', 3, 256, 256, 3, 0.6), ('300x200', 1, 300, 200, 3, 0.3), ('1024x512_2pct', 1, 1024, 512, 3, 0.02),
              ('256x256_ch1', 1, 256, 256, 1, 0.01), ('256x256_ch4', 1, 256, 256, 4, 0.01),
              # beyond the issue's list.  The top of the pyramid has a small form (at most 512 sums from the per-tile level up to 1x1)
              # and a large one: 1100 x 1100 is 18 x 18 tiles, 324 + 81 + 25 + 9 + 4 + 1 = 444 sums, still small;
              # 4096 x 70 the greatest extent in one direction (64 x 2 tiles, 191 sums, small); 1300 x 1300 is 21 x 21 tiles,
              # 441 + 121 + 36 + 9 + 4 + 1 = 612 sums, the large form; 4096 x 4096 is 64 x 64 tiles, 5461 sums, all the large form holds
              ('1100x1100_ch1', 1, 1100, 1100, 1, 0.001), ('4096x70', 1, 4096, 70, 3, 0.01),
              ('1300x1300_ch1', 1, 1300, 1300, 1, 0.001), ('4096x4096_ch1', 1, 4096, 4096, 1, 0.0005)]


def top_sums(H, W, tile=64):
    """The sums from the per-tile level up to 1x1: what decides between the two forms of the top of the pyramid."""
    h, w, n = -(-H // tile), -(-W // tile), 0
    while True:
        n += h * w
        if h == 1 and w == 1:
            return n
        h, w = (h + 1) // 2, (w + 1) // 2


def size_case(name):
    i = [c[0] for c in SIZE_CASES].index(name)
    _, T, H, W, ch, valid = SIZE_CASES[i]
    return random_case(1000 + i, T, H, W, ch, valid)


def mask_cases():
    """name -> (tex [1,H,W,3], mask [1,H,W]); 256 x 256 unless the name says otherwise."""
    rng = np.random.default_rng(77)
    tex = rng.integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)
    z = lambda: np.zeros((1, 256, 256), np.uint8)
    out = {}
    out['random60'] = (tex, random_case(1, 1, 256, 256, 3, 0.6)[1])
    out['random1'] = (tex, random_case(2, 1, 256, 256, 3, 0.01)[1])
    out['all_valid'] = (tex, np.full((1, 256, 256), 255, np.uint8))
    out['empty'] = (tex, z())
    t130 = rng.integers(0, 256, (1, 130, 130, 3), dtype=np.uint8)
    m130 = np.zeros((1, 130, 130), np.uint8)
    m130[0, 129, 129] = 1
    out['single_corner_130'] = (t130, m130)
    m = z(); m[0, :, :100] = 255
    out['left100'] = (tex, m)
    m = z()
    for k in (63, 64, 127, 128):
        m[0, k, :] = 255
        m[0, :, k] = 255
    out['tile_borders'] = (tex, m)
    m = random_case(3, 1, 256, 256, 3, 0.3)[1]
    m[m != 0] = np.where(rng.uniform(0, 1, int((m != 0).sum())) < 0.5, 1, 255).astype(np.uint8)
    out['mask_1_and_255'] = (tex, m)
    return out


def merge_case(T):
    """T views of 256 x 256 with different masks: a band no view saw, a band all saw, the rest seen by a random subset."""
    tex, mask = random_case(500 + T, T, 256, 256, 3, 0.5)
    mask[:, 40:60, :] = 0
    mask[:, 100:130, :] = 255
    return tex, mask


def invariants(tex, mask, out):
    """The five properties the definition was prototyped against, for one unmerged call (tex [T,H,W,ch])."""
    v = mask != 0
    for t in range(tex.shape[0]):
        assert np.array_equal(out[t][v[t]], tex[t][v[t]])                      # valid texels are unchanged
        if v[t].any():
            lo, hi = tex[t][v[t]].min(0), tex[t][v[t]].max(0)
            assert (out[t] >= lo).all() and (out[t] <= hi).all()               # within [min, max] of the valid texels
            if v[t].sum() == 1:
                assert (out[t] == tex[t][v[t]][0]).all()                       # a single valid texel floods the texture
        else:
            assert not out[t].any()                                            # an empty mask gives zeros
