// gfx950 kernels of syn_texture_fill: push-pull (pyramid) completion of uint8 UV textures, the step behind texture_from_image
// (render_kernels.hip: every vertex writes one texel, so a texture has holes by construction).  DESIGN 5.5c has the definition;
// tests/texture_fill_cases.py states it in numpy.  Integer arithmetic only: the result does not depend on the tiling or on the order
// of the sums, and the tests ask for it byte for byte.
//
// Three launches for every size and every batch (the batch is part of grid.x), no launch per level:
//   push   one workgroup per (texture, 64x64 tile): tex and mask are read once (all T views of a texel with merge), reduced 2x2 to the
//          tile's 32x32 level-1 sums and on through LDS to its single level-6 sum; levels 1..6 go to the global pyramid.
//   top    one workgroup per texture: the level-6 grid (one sum per tile, at most 64x64) is pushed to 1x1 and pulled back down in LDS;
//          written out: V_6, one packed colour per tile.
//   pull   one workgroup per (texture, tile): at every level the tile's region plus a ONE-texel ring.  The ring's parents and their
//          nx / ny neighbours lie in the parent region plus its own ring, so the workgroup reads V_6 of the 3x3 tiles around it and the
//          ring's sums from the global pyramid, recomputes the ring redundantly and needs nothing from another workgroup.
// Pyramid layout (per output texture): levels 1..6 one after the other, level l as NC = ch + 1 planes (colour sums, then the weight) of
// (nty * n_l) x (ntx * n_l) uint32, n_l = 64 >> l -- padded to whole tiles, the padding holds zero sums ("children that exist").
// With H*W <= 2^24 (and T*H*W <= 2^24 with merge, the host refuses more) every sum fits 32 bits: 255 * 2^24 < 2^32.
#include "syn_internal.h"

namespace syn {

namespace {
constexpr int kTile = 64, kTileLog = 6;
constexpr int kTileSums = 1024 + 256 + 64 + 16 + 4 + 1;        // levels 1..6 of one tile
constexpr int kMaxC = 4;
// The top kernel holds levels 6 .. 1x1.  The host refuses sizes above kTextureFillMaxDim = 2^12, so there are at most 7 of them
// (64x64 down to 1x1) with 4096 + 1024 + ... + 1 = 5461 sums: what off[] and the larger CAP below are sized for.
constexpr int kTopLevels = 7, kTopSumsMax = 5461, kTopCapSmall = 512, kTopCapLarge = 5464;
static_assert(kTextureFillMaxDim == kTile << (kTopLevels - 1), "the top kernel's off[] holds the levels of a 4096 x 4096 texture");
static_assert(((1 << (2 * kTopLevels)) - 1) / 3 == kTopSumsMax && kTopSumsMax <= kTopCapLarge, "CAP holds every sum above the tiles");

// offset of level l (1..6) inside one tile's / one plane set's run of levels, in units of n_l^2 sums per tile
__device__ __forceinline__ int tile_level_off(int l) {          // 0, 1024, 1280, 1344, 1360, 1364
    int o = 0;
    for (int j = 1; j < l; ++j) o += (kTile >> j) * (kTile >> j);
    return o;
}
__device__ __forceinline__ int level_dim(int n, int l) { return (n + (1 << l) - 1) >> l; }

// floor((2c + w) / (2w)) for w > 0 and c <= 255 w: the float quotient is within one of it, two 64-bit products settle it
__device__ __forceinline__ unsigned round_mean(unsigned c, unsigned w) {
    const unsigned long long n = 2ull * c + w, d = 2ull * w;
    unsigned q = (unsigned)((2.0f * (float)c + (float)w) / (2.0f * (float)w));
    if (d * q > n) --q;
    else if (d * (q + 1) <= n) ++q;
    return q;
}

// (9 a + 3 b + 3 c + d + 8) >> 4 on four packed colours, channel by channel
__device__ __forceinline__ unsigned blend(unsigned a, unsigned b, unsigned c, unsigned d) {
    unsigned r = 0;
#pragma unroll
    for (int q = 0; q < kMaxC; ++q) {
        const int s = 8 * q;
        r |= ((9u * ((a >> s) & 255u) + 3u * ((b >> s) & 255u) + 3u * ((c >> s) & 255u) + ((d >> s) & 255u) + 8u) >> 4) << s;
    }
    return r;
}

// V of the level above at the parents of (y, x): up[] holds a region of it, origin (oy, ox), row pitch `pitch`; hu x wu = its real size
__device__ __forceinline__ unsigned pull_from(const unsigned *up, int pitch, int oy, int ox, int hu, int wu, int y, int x) {
    const int py = y >> 1, px = x >> 1;
    const int ny = min(max(py + ((y & 1) ? 1 : -1), 0), hu - 1), nx = min(max(px + ((x & 1) ? 1 : -1), 0), wu - 1);
    const unsigned *r0 = up + (py - oy) * pitch - ox, *r1 = up + (ny - oy) * pitch - ox;
    return blend(r0[px], r0[nx], r1[px], r1[nx]);
}
}  // namespace

// ---- push: grid.x = Tout * nty * ntx, 256 threads ----
// views: the textures summed into one level 0 (T with merge, else 1; then texture t of the batch is the only view)
__global__ __launch_bounds__(256) void texfill_push_kernel(const unsigned char *__restrict__ tex, const unsigned char *__restrict__ mask,
                                                           unsigned *__restrict__ pyr, int views, int H, int W, int ch, int nty,
                                                           int ntx) {
    __shared__ unsigned s[kMaxC + 1][kTileSums];
    const int ntiles = nty * ntx, t = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, ty = tile / ntx, tx = tile % ntx;
    const int nc = ch + 1;
    unsigned *p = pyr + (size_t)t * nc * ntiles * kTileSums;
    const size_t texels = (size_t)H * W, first = views > 1 ? 0 : (size_t)t * texels;
    for (int l = 1; l <= kTileLog; ++l) {
        const int n = kTile >> l, off = tile_level_off(l);
        const size_t plane = (size_t)ntiles * n * n;
        unsigned *pl = p + (size_t)nc * ntiles * off;
        for (int i = threadIdx.x; i < n * n; i += 256) {
            const int y = i / n, x = i % n;
            unsigned acc[kMaxC + 1] = {0u, 0u, 0u, 0u, 0u};
            if (l == 1) {
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx) {
                        const int gy = ty * kTile + 2 * y + dy, gx = tx * kTile + 2 * x + dx;
                        if (gy >= H || gx >= W) continue;
                        size_t o = first + (size_t)gy * W + gx;
                        for (int v = 0; v < views; ++v, o += texels)
                            if (mask[o]) {
                                ++acc[kMaxC];
                                for (int q = 0; q < ch; ++q) acc[q] += tex[o * ch + q];
                            }
                    }
            } else {
                const int n2 = 2 * n, poff = tile_level_off(l - 1);
#pragma unroll
                for (int q = 0; q <= kMaxC; ++q) {
                    const unsigned *c = &s[q][poff + 2 * y * n2 + 2 * x];
                    acc[q] = c[0] + c[1] + c[n2] + c[n2 + 1];
                }
            }
            const size_t g = (size_t)(ty * n + y) * (ntx * n) + tx * n + x;
#pragma unroll
            for (int q = 0; q <= kMaxC; ++q) s[q][off + i] = acc[q];
            for (int q = 0; q < ch; ++q) pl[q * plane + g] = acc[q];
            pl[ch * plane + g] = acc[kMaxC];
        }
        __syncthreads();
    }
}

// ---- top: one workgroup per output texture; CAP = the sums of levels 6 .. 1x1 it can hold ----
template <int CAP>
__global__ __launch_bounds__(256) void texfill_top_kernel(const unsigned *__restrict__ pyr, unsigned *__restrict__ v6, int H, int W,
                                                          int ch, int nty, int ntx) {
    __shared__ unsigned s[kMaxC + 1][CAP];
    __shared__ unsigned V[CAP];
    const int t = blockIdx.x, ntiles = nty * ntx, nc = ch + 1;
    const unsigned *p6 = pyr + ((size_t)t * kTileSums + tile_level_off(kTileLog)) * nc * ntiles;        // n_6 = 1: one sum per tile
    for (int i = threadIdx.x; i < ntiles; i += 256) {
#pragma unroll
        for (int q = 0; q < kMaxC; ++q) s[q][i] = q < ch ? p6[(size_t)q * ntiles + i] : 0u;
        s[kMaxC][i] = p6[(size_t)ch * ntiles + i];
    }
    __syncthreads();
    // push to 1x1; level 6 + k starts at off[k].  The host counted the same sums to pick CAP: it halves the tile counts, which is
    // level_dim(H, 6 + k) because ceil(ceil(H / 64) / 2^k) = ceil(H / 2^(6 + k))
    int off[kTopLevels + 1], top = 0;
    off[0] = 0;
    for (int k = 0; level_dim(H, kTileLog + k) > 1 || level_dim(W, kTileLog + k) > 1; ++k) {
        const int hc = level_dim(H, kTileLog + k), wc = level_dim(W, kTileLog + k), hn = (hc + 1) >> 1, wn = (wc + 1) >> 1;
        off[k + 1] = off[k] + hc * wc;
        for (int i = threadIdx.x; i < hn * wn; i += 256) {
            const int y = i / wn, x = i % wn;
            const bool right = 2 * x + 1 < wc, below = 2 * y + 1 < hc;
#pragma unroll
            for (int q = 0; q <= kMaxC; ++q) {
                const unsigned *c = &s[q][off[k] + 2 * y * wc + 2 * x];
                s[q][off[k + 1] + i] = c[0] + (right ? c[1] : 0u) + (below ? c[wc] : 0u) + (right && below ? c[wc + 1] : 0u);
            }
        }
        top = k + 1;
        __syncthreads();
    }
    // pull back down to level 6
    for (int k = top; k >= 0; --k) {
        const int hc = level_dim(H, kTileLog + k), wc = level_dim(W, kTileLog + k);
        for (int i = threadIdx.x; i < hc * wc; i += 256) {
            const unsigned w = s[kMaxC][off[k] + i];
            unsigned v = 0u;
            if (w) {
#pragma unroll
                for (int q = 0; q < kMaxC; ++q) v |= round_mean(s[q][off[k] + i], w) << (8 * q);
            } else if (k < top) {
                v = pull_from(&V[off[k + 1]], (wc + 1) >> 1, 0, 0, (hc + 1) >> 1, (wc + 1) >> 1, i / wc, i % wc);
            }
            V[off[k] + i] = v;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < ntiles; i += 256) v6[(size_t)t * ntiles + i] = V[i];
}

// ---- pull: grid.x = Tout * nty * ntx, 256 threads ----
__global__ __launch_bounds__(256) void texfill_pull_kernel(const unsigned char *__restrict__ tex, const unsigned char *__restrict__ mask,
                                                           const unsigned *__restrict__ pyr, const unsigned *__restrict__ v6,
                                                           unsigned char *__restrict__ out, int views, int H, int W, int ch, int nty,
                                                           int ntx) {
    constexpr int kReg = kTile / 2 + 2;                         // the level-1 region: 32 + ring
    __shared__ unsigned Va[kReg * kReg], Vb[kReg * kReg];
    const int ntiles = nty * ntx, t = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, ty = tile / ntx, tx = tile % ntx;
    const int nc = ch + 1;
    const unsigned *p = pyr + (size_t)t * nc * ntiles * kTileSums;
    unsigned *up = Va, *cur = Vb;
    // level 6: the 3x3 tiles around this one (what lies outside the grid is never referenced: ny / nx are clamped into it)
    if (threadIdx.x < 9) {
        const int gy = ty - 1 + (int)threadIdx.x / 3, gx = tx - 1 + (int)threadIdx.x % 3;
        up[threadIdx.x] = (gy >= 0 && gy < nty && gx >= 0 && gx < ntx) ? v6[(size_t)t * ntiles + gy * ntx + gx] : 0u;
    }
    __syncthreads();
    for (int l = kTileLog - 1; l >= 1; --l) {
        const int n = kTile >> l, r = n + 2, ru = n / 2 + 2;    // this level's region and the one above it, ring included
        const int oy = ty * n - 1, ox = tx * n - 1, uy = ty * (n / 2) - 1, ux = tx * (n / 2) - 1;
        const int hl = level_dim(H, l), wl = level_dim(W, l), hu = level_dim(H, l + 1), wu = level_dim(W, l + 1);
        const int pw = ntx * n;
        const size_t plane = (size_t)ntiles * n * n;
        const unsigned *pl = p + (size_t)nc * ntiles * tile_level_off(l);
        for (int i = threadIdx.x; i < r * r; i += 256) {
            const int y = oy + i / r, x = ox + i % r;
            unsigned v = 0u;
            if (y >= 0 && y < hl && x >= 0 && x < wl) {
                const size_t g = (size_t)y * pw + x;
                const unsigned w = pl[ch * plane + g];
                if (w) {
                    for (int q = 0; q < ch; ++q) v |= round_mean(pl[q * plane + g], w) << (8 * q);
                } else {
                    v = pull_from(up, ru, uy, ux, hu, wu, y, x);
                }
            }
            cur[i] = v;
        }
        __syncthreads();
        unsigned *sw = up; up = cur; cur = sw;
    }
    // level 0: the tile itself, from V_1 (origin ty*32 - 1, pitch 34)
    const int h1 = level_dim(H, 1), w1 = level_dim(W, 1);
    const size_t texels = (size_t)H * W, first = views > 1 ? 0 : (size_t)t * texels;
    for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
        const int y = ty * kTile + i / kTile, x = tx * kTile + i % kTile;
        if (y >= H || x >= W) continue;
        size_t o = first + (size_t)y * W + x;
        unsigned char *dst = out + ((size_t)t * texels + (size_t)y * W + x) * ch;
        if (views == 1) {
            if (mask[o]) {
                for (int q = 0; q < ch; ++q) dst[q] = tex[o * ch + q];
                continue;
            }
        } else {
            unsigned acc[kMaxC] = {0u, 0u, 0u, 0u}, w = 0u;
            for (int v = 0; v < views; ++v, o += texels)
                if (mask[o]) {
                    ++w;
                    for (int q = 0; q < ch; ++q) acc[q] += tex[o * ch + q];
                }
            if (w) {
                for (int q = 0; q < ch; ++q) dst[q] = (unsigned char)round_mean(acc[q], w);
                continue;
            }
        }
        const unsigned v = pull_from(up, kReg, ty * (kTile / 2) - 1, tx * (kTile / 2) - 1, h1, w1, y, x);
        for (int q = 0; q < ch; ++q) dst[q] = (unsigned char)(v >> (8 * q));
    }
}

size_t texture_fill_scratch_bytes(int Tout, int th, int tw, int ch) {
    const size_t ntiles = (size_t)((th + kTile - 1) / kTile) * ((tw + kTile - 1) / kTile);
    return sizeof(unsigned) * (size_t)Tout * ntiles * ((size_t)(ch + 1) * kTileSums + 1);
}

void launch_texture_fill(const unsigned char *tex, const unsigned char *mask, unsigned *scratch, unsigned char *out, int T, int th,
                         int tw, int ch, int merge, hipStream_t s) {
    const int nty = (th + kTile - 1) / kTile, ntx = (tw + kTile - 1) / kTile, ntiles = nty * ntx;
    const int Tout = merge ? 1 : T, views = merge ? T : 1;
    unsigned *pyr = scratch, *v6 = scratch + (size_t)Tout * ntiles * (ch + 1) * kTileSums;
    int above = 0;                                              // the sums of levels 6 .. 1x1
    for (int h = nty, w = ntx;; h = (h + 1) / 2, w = (w + 1) / 2) {
        above += h * w;
        if (h == 1 && w == 1) break;
    }
    texfill_push_kernel<<<(unsigned)(Tout * ntiles), 256, 0, s>>>(tex, mask, pyr, views, th, tw, ch, nty, ntx);
    if (above <= kTopCapSmall) texfill_top_kernel<kTopCapSmall><<<Tout, 256, 0, s>>>(pyr, v6, th, tw, ch, nty, ntx);
    else texfill_top_kernel<kTopCapLarge><<<Tout, 256, 0, s>>>(pyr, v6, th, tw, ch, nty, ntx);     // 64x64 tiles: 5461 sums, 128 KB of LDS
    texfill_pull_kernel<<<(unsigned)(Tout * ntiles), 256, 0, s>>>(tex, mask, pyr, v6, out, views, th, tw, ch, nty, ntx);
}

}  // namespace syn
