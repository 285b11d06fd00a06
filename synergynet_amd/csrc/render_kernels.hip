// gfx950 kernels for the mesh consumers that follow the reconstruction in the reference's demo path:
//   Sim3DR.get_normal   (Sim3DR/lib/rasterize_kernel.cpp:158-215)  per-vertex normals
//   RenderPipeline      (Sim3DR/lighting.py:37-71)                   ambient + diffuse + specular vertex colours
//   Sim3DR.rasterize    (Sim3DR/lib/rasterize_kernel.cpp:219-287)  z-buffer rasteriser, barycentric colours
//   cv2.addWeighted     (utils/render.py:45)                         alpha overlay
//   textured meshes     (uv_texture_realFaces.py:45-51,96-116, lighting.py:68-70): UV colour lookup, kept-vertex gather,
//                       texture * light in the lighting epilogue
//   Sim3DR.rasterize_triangles (Sim3DR/lib/rasterize_kernel.cpp:290-348)  per-pixel winning triangle, weights, depth; on top of it
//                       vertex visibility, per-vertex colours sampled from a frame and the scatter into a UV texture image
//   _render_texture_core (Sim3DR/lib/rasterize_kernel.cpp:353-458)  per-pixel texture mapping on the z-buffer, nearest or bilinear
// The reference walks the 105 840 triangles one at a time on the host.  Here every stage is data parallel and still
// reproduces the sequential result BIT FOR BIT (tests/test_gpu_render.py):
//   * arithmetic is plain IEEE single precision in the reference's operation order -- FMA contraction is switched off for
//     this file, divisions and square roots are correctly rounded;
//   * vertex normals are summed per vertex over a CSR list of its incident triangles in ascending triangle order (built
//     once per topology by the host), which is the order the sequential loop adds them in;
//   * the z-buffer is a 64-bit atomicMax on  [face index | order-preserving depth bits | ~triangle index] : the sequential
//     rule "overwrite when strictly deeper" ends at the deepest triangle, earliest index among equals -- +0 and -0 are equal
//     to the reference's `>`, so the key of a zero depth is taken from +0 whatever its sign -- and a later face
//     overwrites an earlier one wherever it covers (each face starts from a fresh depth buffer); a second pass re-derives
//     the barycentric weights of the winning triangle and writes the colour (alpha = 1, the binding's default).
// Exception: numpy evaluates (v2v*reflection)**5 with glibc powf; the kernel uses an exactly rounded double product, which
// differs from powf in the last bit for a small fraction of inputs (light agrees to 1e-6, pixels to one grey level).
#pragma clang fp contract(off)

#include "syn_internal.h"

namespace syn {

namespace {
// `planar`: 0 -> [nver,3] interleaved (the reference's layout); >= nver -> planar rows `planar` floats apart ([3,pitch][:, :nver],
// what syn_reconstruct_pitched writes; pitch == nver is the packed [3,nver]).  The launchers map the ABI's planar = 1 to nver.
__device__ __forceinline__ float vtx(const float *v, int planar, int nver, int i, int c) {
    return planar ? v[(size_t)c * planar + i] : v[(size_t)i * 3 + c];
}
__device__ __forceinline__ size_t face_stride(int planar, int nver) { return planar ? (size_t)3 * planar : (size_t)3 * nver;
}
}  // namespace

// ---- triangle cross products (rasterize_kernel.cpp:166-185), one thread per (face, triangle) ----
__global__ __launch_bounds__(256) void tri_normal_kernel(const float *__restrict__ vertices, const int *__restrict__ tri,
                                                         float *__restrict__ tri_normal, int nver, int ntri, int planar) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= ntri) return;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    const int p0 = tri[3 * i], p1 = tri[3 * i + 1], p2 = tri[3 * i + 2];
    const float v1x = vtx(v, planar, nver, p1, 0) - vtx(v, planar, nver, p0, 0);
    const float v1y = vtx(v, planar, nver, p1, 1) - vtx(v, planar, nver, p0, 1);
    const float v1z = vtx(v, planar, nver, p1, 2) - vtx(v, planar, nver, p0, 2);
    const float v2x = vtx(v, planar, nver, p2, 0) - vtx(v, planar, nver, p0, 0);
    const float v2y = vtx(v, planar, nver, p2, 1) - vtx(v, planar, nver, p0, 1);
    const float v2z = vtx(v, planar, nver, p2, 2) - vtx(v, planar, nver, p0, 2);
    float *o = tri_normal + ((size_t)f * ntri + i) * 3;
    o[0] = v1y * v2z - v1z * v2y;
    o[1] = v1z * v2x - v1x * v2z;
    o[2] = v1x * v2y - v1y * v2x;
}

// ---- vertex normals (rasterize_kernel.cpp:187-212): ordered sum over incident triangles, then normalise ----
// normal out is [F, nver, 3] (the reference's layout).
__global__ __launch_bounds__(256) void ver_normal_kernel(const float *__restrict__ tri_normal, const int *__restrict__ adj_off,
                                                         const int *__restrict__ adj_tri, float *__restrict__ normal, int nver,
                                                         int ntri) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= nver) return;
    float x = 0.f, y = 0.f, z = 0.f;
    const float *tn = tri_normal + (size_t)f * ntri * 3;
    for (int a = adj_off[i]; a < adj_off[i + 1]; ++a) {
        const int t = adj_tri[a];
        x += tn[3 * t]; y += tn[3 * t + 1]; z += tn[3 * t + 2];
    }
    const float det = sqrtf(x * x + y * y + z * z);
    float *o = normal + ((size_t)f * nver + i) * 3;
    o[0] = x / det; o[1] = y / det; o[2] = z / det;
}

// ---- per-face, per-axis min / max of the vertices (norm_vertices, lighting.py:9-14) as order-preserving integer keys ----
// grid (kMinMaxBlocks, F): block-level reduction, then six atomics per block (a few dozen per face)
constexpr int kMinMaxBlocks = 8;
__global__ __launch_bounds__(1024) void minmax_kernel(const float *__restrict__ vertices, unsigned *__restrict__ mm, int nver, int planar) {
    __shared__ unsigned red[16][6];
    const int f = blockIdx.y;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    auto key = [](float a) { const unsigned u = __builtin_bit_cast(unsigned, a); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    unsigned k[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    for (int i = blockIdx.x * 1024 + threadIdx.x; i < nver; i += kMinMaxBlocks * 1024)
        for (int c = 0; c < 3; ++c) {
            const unsigned kk = key(vtx(v, planar, nver, i, c));
            k[c] = min(k[c], kk); k[3 + c] = max(k[3 + c], kk);
        }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            k[c] = min(k[c], (unsigned)__shfl_xor((int)k[c], s));
            k[3 + c] = max(k[3 + c], (unsigned)__shfl_xor((int)k[3 + c], s));
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 6; ++c) red[wave][c] = k[c];
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned r = red[0][threadIdx.x];
        for (int w2 = 1; w2 < 16; ++w2) r = threadIdx.x < 3 ? min(r, red[w2][threadIdx.x]) : max(r, red[w2][threadIdx.x]);
        if (threadIdx.x < 3) atomicMin(&mm[f * 6 + threadIdx.x], r); else atomicMax(&mm[f * 6 + threadIdx.x], r);
    }
}

// ---- Phong vertex colours (lighting.py:37-71 with norm_vertices :9-14), one thread per (face, vertex) ----
// cfg: [0] intensity_ambient [1..3] color_ambient [4] intensity_directional [5..7] color_directional
//      [8] intensity_specular [9] specular_exp(int) [10..12] light_pos [13..15] view_pos
namespace {
__device__ __forceinline__ void phong_vertex(const float *__restrict__ vertices, const float *__restrict__ normal,
                                             const unsigned *__restrict__ mm, const float *__restrict__ cfg, int nver, int planar,
                                             int f, int i, float out[3]) {
    auto unkey = [](unsigned k) { const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; return __builtin_bit_cast(float, u); };
    const unsigned *m = mm + f * 6;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    // norm_vertices: v -= min(0); v /= v.max(); v *= 2; v -= v.max(0) / 2   (all monotone: the extrema map to the extrema)
    float mn[3], mx[3], vn[3];
    for (int c = 0; c < 3; ++c) { mn[c] = unkey(m[c]); mx[c] = unkey(m[3 + c]) - mn[c]; }
    const float s = fmaxf(mx[0], fmaxf(mx[1], mx[2]));
    for (int c = 0; c < 3; ++c) {
        const float hi = (mx[c] / s) * 2.0f;
        vn[c] = ((vtx(v, planar, nver, i, c) - mn[c]) / s) * 2.0f - hi / 2.0f;
    }
    const float *n = normal + ((size_t)f * nver + i) * 3;
    float l[3] = {0.f, 0.f, 0.f};
    if (cfg[0] > 0)
        for (int c = 0; c < 3; ++c) l[c] += cfg[0] * cfg[1 + c];
    if (cfg[4] > 0) {
        float d[3], dn = 0.f;
        for (int c = 0; c < 3; ++c) { d[c] = cfg[10 + c] - vn[c]; dn += d[c] * d[c]; }
        dn = sqrtf(dn);
        float cs = 0.f;
        for (int c = 0; c < 3; ++c) { d[c] = d[c] / dn; cs += n[c] * d[c]; }
        const float cc = fminf(fmaxf(cs, 0.0f), 1.0f);          // np.clip propagates NaN exactly like fmin(fmax()) does not:
        const float ccl = (cs != cs) ? cs : cc;                  // keep NaN (vertices without triangles), as numpy does
        for (int c = 0; c < 3; ++c) l[c] += cfg[4] * (cfg[5 + c] * ccl);
        if (cfg[8] > 0) {
            float w[3], wn = 0.f;
            for (int c = 0; c < 3; ++c) { w[c] = cfg[13 + c] - vn[c]; wn += w[c] * w[c]; }
            wn = sqrtf(wn);
            const int e = (int)cfg[9];
            float spe = 0.f;
            for (int c = 0; c < 3; ++c) {
                const float r = (2.0f * cs) * n[c] - d[c];
                const double b = (double)((w[c] / wn) * r);
                double p = 1.0;
                for (int q = 0; q < e; ++q) p *= b;
                spe += (float)p;
            }
            float sc = (spe != spe) ? spe : fminf(fmaxf(spe, 0.0f), 1.0f);
            if (!(cs != 0.0f)) sc = 0.0f;                         // np.where(cos != 0, clip(spe), 0): NaN != 0 is True
            const float sc2 = (sc != sc) ? sc : fminf(fmaxf(sc, 0.0f), 1.0f);
            for (int c = 0; c < 3; ++c) l[c] += (cfg[8] * cfg[5 + c]) * sc2;
        }
    }
    for (int c = 0; c < 3; ++c) out[c] = (l[c] != l[c]) ? l[c] : fminf(fmaxf(l[c], 0.0f), 1.0f);
}
}  // namespace

__global__ __launch_bounds__(256) void lighting_kernel(const float *__restrict__ vertices, const float *__restrict__ normal,
                                                       const unsigned *__restrict__ mm, const float *__restrict__ cfg,
                                                       float *__restrict__ light, int nver, int planar) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= nver) return;
    float l[3];
    phong_vertex(vertices, normal, mm, cfg, nver, planar, f, i, l);
    float *o = light + ((size_t)f * nver + i) * 3;
    for (int c = 0; c < 3; ++c) o[c] = l[c];
}

// ---- textured vertex colours (lighting.py:68-70: `texture *= light`), the product in the lighting epilogue ----
// Per-face textures [F,nver,3]: colours[f] = tex[f] * light[f], one thread per (face, vertex).  colours may alias tex.
__global__ __launch_bounds__(256) void lighting_tex_kernel(const float *__restrict__ vertices, const float *__restrict__ normal,
                                                           const unsigned *__restrict__ mm, const float *__restrict__ cfg,
                                                           float *light, const float *tex, float *colors, int nver, int planar) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= nver) return;
    float l[3];
    phong_vertex(vertices, normal, mm, cfg, nver, planar, f, i, l);
    const size_t o = ((size_t)f * nver + i) * 3;
    for (int c = 0; c < 3; ++c) {
        const float t = tex[o + c];
        if (light) light[o + c] = l[c];
        colors[o + c] = t * l[c];
    }
}

// One shared texture [nver,3]: the reference multiplies the caller's array in place once per face (utils/render.py:39-42 hands
// the same array to every call), so face f is drawn with ((tex * l0) * l1) ... * lf.  One thread per vertex walks the faces in
// order; the last product goes back into tex.
__global__ __launch_bounds__(256) void lighting_tex_shared_kernel(const float *__restrict__ vertices, const float *__restrict__ normal,
                                                                  const unsigned *__restrict__ mm, const float *__restrict__ cfg,
                                                                  float *light, float *tex, float *colors, int F, int nver,
                                                                  int planar) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nver) return;
    float t[3];
    for (int c = 0; c < 3; ++c) t[c] = tex[(size_t)i * 3 + c];
    for (int f = 0; f < F; ++f) {
        float l[3];
        phong_vertex(vertices, normal, mm, cfg, nver, planar, f, i, l);
        const size_t o = ((size_t)f * nver + i) * 3;
        for (int c = 0; c < 3; ++c) {
            t[c] = t[c] * l[c];
            if (light) light[o + c] = l[c];
            colors[o + c] = t[c];
        }
    }
    for (int c = 0; c < 3; ++c) tex[(size_t)i * 3 + c] = t[c];
}

// ---- UV colour lookup (uv_texture_realFaces.py:48-49,109-115): np.flip(img, 0)[coord_u, coord_v, :] per (texture, vertex) ----
// uv_tex uint8 [T,th,tw,ch]; keep == nullptr: every vertex, else vertex keep[k]; out float32 [T,n,ch], raw 0..255 or / 255.0f.
__global__ __launch_bounds__(256) void uv_colors_kernel(const unsigned char *__restrict__ uv_tex, const int *__restrict__ coord_u,
                                                        const int *__restrict__ coord_v, const int *__restrict__ keep,
                                                        float *__restrict__ out, int n, int th, int tw, int ch, int normalize) {
    const int k = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (k >= n) return;
    const int v = keep ? keep[k] : k;
    const unsigned char *src = uv_tex + (((size_t)t * th + (th - 1 - coord_u[v])) * tw + coord_v[v]) * ch;
    float *o = out + ((size_t)t * n + k) * ch;
    for (int q = 0; q < ch; ++q) {
        const float x = (float)src[q];
        o[q] = normalize ? x / 255.0f : x;
    }
}

// ---- kept-vertex gather (vertices[:, keep_ind], uv_texture_realFaces.py:98): [F,3,pitch][:, :, :nver] -> [F,3,n_keep] ----
__global__ __launch_bounds__(256) void gather_vertices_kernel(const float *__restrict__ vertices, const int *__restrict__ keep,
                                                              float *__restrict__ out, int n_keep, int pitch) {
    const int k = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;           // row = face * 3 + coordinate
    if (k >= n_keep) return;
    out[(size_t)row * n_keep + k] = vertices[(size_t)row * pitch + keep[k]];
}

namespace {
struct Bary { float w0, w1, w2; bool in; };
// is_point_in_tri + get_point_weight (rasterize_kernel.cpp:26-82)
__device__ __forceinline__ Bary bary(float px, float py, float p0x, float p0y, float p1x, float p1y, float p2x, float p2y) {
    const float v0x = p2x - p0x, v0y = p2y - p0y, v1x = p1x - p0x, v1y = p1y - p0y, v2x = px - p0x, v2y = py - p0y;
    const float dot00 = v0x * v0x + v0y * v0y, dot01 = v0x * v1x + v0y * v1y, dot02 = v0x * v2x + v0y * v2y;
    const float dot11 = v1x * v1x + v1y * v1y, dot12 = v1x * v2x + v1y * v2y;
    const float den = dot00 * dot11 - dot01 * dot01;
    const float inv = den == 0 ? 0.0f : 1 / den;
    const float u = (dot11 * dot02 - dot01 * dot12) * inv, v = (dot00 * dot12 - dot01 * dot02) * inv;
    Bary b;
    b.w0 = 1 - u - v; b.w1 = v; b.w2 = u;
    b.in = (u >= 0) && (v >= 0) && (u + v < 1);
    return b;
}
// the bilinear expression of rasterize_kernel.cpp:445-447, left to right (tex_resolve_kernel; sample_vertex_colors_kernel keeps its
// own copy of the line: routed through this function hipcc swaps the operands of four of its additions)
__device__ __forceinline__ float bilerp(float ul, float ur, float dl, float dr, float xd, float yd) {
    return ul * (1 - xd) * (1 - yd) + ur * xd * (1 - yd) + dl * (1 - xd) * yd + dr * xd * yd;
}
__device__ __forceinline__ unsigned depth_key(float d) {
    const unsigned u = __builtin_bit_cast(unsigned, d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
}  // namespace

// ---- z-buffer pass 1 (rasterize_kernel.cpp:229-262): one thread per (face, triangle) walks its bounding box ----
// A zero depth is keyed as +0 (as in tri_depth_kernel): the raw bits would order -0 below +0, which the reference's `>` does not.
__global__ __launch_bounds__(256) void raster_depth_kernel(const float *__restrict__ vertices, const int *__restrict__ tri,
                                                           unsigned long long *__restrict__ zkey, int nver, int ntri, int h,
                                                           int w, int planar) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= ntri) return;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    const int t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    const float p0x = vtx(v, planar, nver, t0, 0), p0y = vtx(v, planar, nver, t0, 1), d0 = vtx(v, planar, nver, t0, 2);
    const float p1x = vtx(v, planar, nver, t1, 0), p1y = vtx(v, planar, nver, t1, 1), d1 = vtx(v, planar, nver, t1, 2);
    const float p2x = vtx(v, planar, nver, t2, 0), p2y = vtx(v, planar, nver, t2, 1), d2 = vtx(v, planar, nver, t2, 2);
    const int x_min = max((int)floorf(fminf(p0x, fminf(p1x, p2x))), 0), x_max = min((int)ceilf(fmaxf(p0x, fmaxf(p1x, p2x))), w - 1);
    const int y_min = max((int)floorf(fminf(p0y, fminf(p1y, p2y))), 0), y_max = min((int)ceilf(fmaxf(p0y, fmaxf(p1y, p2y))), h - 1);
    if (x_max < x_min || y_max < y_min) return;
    const unsigned long long hi = ((unsigned long long)(f + 1) << 56), lo = (unsigned long long)(0xffffffu - (unsigned)i);
    for (int y = y_min; y <= y_max; ++y)
        for (int x = x_min; x <= x_max; ++x) {
            const Bary b = bary((float)x, (float)y, p0x, p0y, p1x, p1y, p2x, p2y);
            if (!b.in) continue;
            const float depth = b.w0 * d0 + b.w1 * d1 + b.w2 * d2;
            if (!(depth > -1e8f)) continue;                       // the fresh depth buffer holds -1e8 (Sim3DR.py:23)
            atomicMax(&zkey[(size_t)y * w + x], hi | ((unsigned long long)depth_key(depth == 0.0f ? 0.0f : depth) << 24) | lo);
        }
}

// ---- pass 2 (rasterize_kernel.cpp:264-280, alpha = 1): one thread per pixel shades the winning triangle ----
__global__ __launch_bounds__(256) void raster_shade_kernel(const float *__restrict__ vertices, const int *__restrict__ tri,
                                                           const float *__restrict__ colors, const unsigned long long *__restrict__ zkey,
                                                           unsigned char *__restrict__ image, int nver, int h, int w, int c,
                                                           int planar, int reverse) {
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= h * w) return;
    const unsigned long long k = zkey[px];
    if (k == 0ull) return;
    const int f = (int)(k >> 56) - 1;
    int i = (int)(0xffffffu - (unsigned)(k & 0xffffffull));
    // hipcc 7.2 folds ((k & 0xffffff) ^ 0xffffff) * 12 into a 24-bit multiply pattern and then widens it again WITHOUT the mask
    // (memory fault on tri[3*i]); an opaque copy keeps the masked value
    asm volatile("" : "+v"(i));
    const int y = px / w, x = px % w;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    const float *col = colors + (size_t)f * nver * c;
    const int t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    const Bary b = bary((float)x, (float)y, vtx(v, planar, nver, t0, 0), vtx(v, planar, nver, t0, 1), vtx(v, planar, nver, t1, 0),
                        vtx(v, planar, nver, t1, 1), vtx(v, planar, nver, t2, 0), vtx(v, planar, nver, t2, 1));
    unsigned char *o = image + ((size_t)(reverse ? (h - 1 - y) : y) * w + x) * c;
    for (int q = 0; q < c; ++q) {
        const float pc = b.w0 * col[c * t0 + q] + b.w1 * col[c * t1 + q] + b.w2 * col[c * t2 + q];
        o[q] = (unsigned char)(int)(255 * pc);      // (1-alpha)*image + alpha*255*p_color with alpha = 1: 0*image + 255*p_color exactly
    }
}

// ---- cv2.addWeighted for uint8 images (utils/render.py:45): saturate(round-half-even(a*alpha + b*beta)) ----
__global__ __launch_bounds__(256) void add_weighted_kernel(const unsigned char *__restrict__ a, float alpha,
                                                           const unsigned char *__restrict__ b, float beta,
                                                           unsigned char *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = (float)a[i] * alpha + (float)b[i] * beta;
    out[i] = (unsigned char)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
}

// ---- Sim3DR.rasterize_triangles (rasterize_kernel.cpp:290-348): per pixel the winning triangle, its weights and its depth ----
// Every face has its own key plane [F,h,w] of [order-preserving depth bits | ~triangle index] (no face field: any F).
// Pass 1, one thread per (face, triangle).  The box is THIS function's (ceil of the minimum, floor of the maximum, :316-320), not
// _rasterize's.  A candidate competes only above the caller's depth buffer (:337; NaN never does).  +0 and -0 are equal to the
// reference's `>`, so the key is taken from +0 for both and the earlier triangle wins; pass 2 recomputes the stored depth.
__global__ __launch_bounds__(256) void tri_depth_kernel(const float *__restrict__ vertices, const int *__restrict__ tri,
                                                        const float *__restrict__ depth0, unsigned long long *__restrict__ zkey,
                                                        int nver, int ntri, int h, int w, int planar) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= ntri) return;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    const int t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    const float p0x = vtx(v, planar, nver, t0, 0), p0y = vtx(v, planar, nver, t0, 1), d0 = vtx(v, planar, nver, t0, 2);
    const float p1x = vtx(v, planar, nver, t1, 0), p1y = vtx(v, planar, nver, t1, 1), d1 = vtx(v, planar, nver, t1, 2);
    const float p2x = vtx(v, planar, nver, t2, 0), p2y = vtx(v, planar, nver, t2, 1), d2 = vtx(v, planar, nver, t2, 2);
    const int x_min = max((int)ceilf(fminf(p0x, fminf(p1x, p2x))), 0), x_max = min((int)floorf(fmaxf(p0x, fmaxf(p1x, p2x))), w - 1);
    const int y_min = max((int)ceilf(fminf(p0y, fminf(p1y, p2y))), 0), y_max = min((int)floorf(fmaxf(p0y, fmaxf(p1y, p2y))), h - 1);
    if (x_max < x_min || y_max < y_min) return;
    const size_t plane = (size_t)f * h * w;
    const unsigned long long lo = (unsigned long long)(0xffffffu - (unsigned)i);
    for (int y = y_min; y <= y_max; ++y)
        for (int x = x_min; x <= x_max; ++x) {
            const Bary b = bary((float)x, (float)y, p0x, p0y, p1x, p1y, p2x, p2y);
            if (!b.in) continue;
            const float depth = b.w0 * d0 + b.w1 * d1 + b.w2 * d2;
            const size_t px = plane + (size_t)y * w + x;
            if (!(depth > depth0[px])) continue;
            atomicMax(&zkey[px], ((unsigned long long)depth_key(depth == 0.0f ? 0.0f : depth) << 24) | lo);
        }
}

// Pass 2, one thread per (face, pixel): where a triangle won, its depth, index and weights (1-u-v, v, u) re-derived with the same
// expressions; elsewhere the caller's three buffers stay as they are (:337-343).
__global__ __launch_bounds__(256) void tri_resolve_kernel(const float *__restrict__ vertices, const int *__restrict__ tri,
                                                          const unsigned long long *__restrict__ zkey, float *__restrict__ depth,
                                                          int *__restrict__ tri_buf, float *__restrict__ weight, int nver, int h,
                                                          int w, int planar) {
    const int px = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (px >= h * w) return;
    const size_t o = (size_t)f * h * w + px;
    const unsigned long long k = zkey[o];
    if (k == 0ull) return;
    int i = (int)(0xffffffu - (unsigned)(k & 0xffffffull));
    asm volatile("" : "+v"(i));                              // the opaque copy of raster_shade_kernel (hipcc 7.2 mask loss)
    const int y = px / w, x = px % w;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    const int t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    const Bary b = bary((float)x, (float)y, vtx(v, planar, nver, t0, 0), vtx(v, planar, nver, t0, 1), vtx(v, planar, nver, t1, 0),
                        vtx(v, planar, nver, t1, 1), vtx(v, planar, nver, t2, 0), vtx(v, planar, nver, t2, 1));
    depth[o] = b.w0 * vtx(v, planar, nver, t0, 2) + b.w1 * vtx(v, planar, nver, t1, 2) + b.w2 * vtx(v, planar, nver, t2, 2);
    tri_buf[o] = i;
    float *wo = weight + o * 3;
    wo[0] = b.w0; wo[1] = b.w1; wo[2] = b.w2;
}

// ---- per-vertex visibility (the 3DDFA lineage's rule): a vertex is visible when it is a corner of a triangle that won a pixel ----
// one thread per (face, pixel); every writer stores the same byte, so the race between them is benign.  visible [F,nver] zeroed.
__global__ __launch_bounds__(256) void vertex_visible_kernel(const int *__restrict__ tri_buf, const int *__restrict__ tri,
                                                             unsigned char *__restrict__ visible, int nver, int ntri, int hw) {
    const int px = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (px >= hw) return;
    const int i = tri_buf[(size_t)f * hw + px];
    if (i < 0 || i >= ntri) return;                          // -1 (nothing drawn) or a caller's value that is no triangle
    unsigned char *vis = visible + (size_t)f * nver;
    for (int c = 0; c < 3; ++c) vis[tri[3 * i + c]] = 1;
}

// ---- per-vertex colours from a frame: bilinear sample at the vertex' (x, y) in the operation order of the reference's only
// bilinear code (rasterize_kernel.cpp:428-447), one thread per (face, vertex); a vertex with a non-finite x or y gets 0 ----
__global__ __launch_bounds__(256) void sample_vertex_colors_kernel(const float *__restrict__ vertices,
                                                                   const unsigned char *__restrict__ image, float *__restrict__ out,
                                                                   int nver, int h, int w, int ch, int planar, int normalize) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= nver) return;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    float x = vtx(v, planar, nver, i, 0), y = vtx(v, planar, nver, i, 1);
    float *o = out + ((size_t)f * nver + i) * ch;
    if (!(fabsf(x) <= 3.402823466e38f) || !(fabsf(y) <= 3.402823466e38f)) {
        for (int q = 0; q < ch; ++q) o[q] = 0.0f;
        return;
    }
    x = fmaxf(fminf(x, (float)(w - 1)), 0.0f);
    y = fmaxf(fminf(y, (float)(h - 1)), 0.0f);
    const float fx = floorf(x), fy = floorf(y);
    const float xd = x - fx, yd = y - fy;
    const int x0 = (int)fx, x1 = (int)ceilf(x), y0 = (int)fy, y1 = (int)ceilf(y);
    for (int q = 0; q < ch; ++q) {
        const float ul = (float)image[((size_t)y0 * w + x0) * ch + q], ur = (float)image[((size_t)y0 * w + x1) * ch + q];
        const float dl = (float)image[((size_t)y1 * w + x0) * ch + q], dr = (float)image[((size_t)y1 * w + x1) * ch + q];
        const float c = ul * (1 - xd) * (1 - yd) + ur * xd * (1 - yd) + dl * (1 - xd) * yd + dr * xd * yd;
        o[q] = normalize ? c / 255.0f : c;
    }
}

// ---- UV scatter, the inverse of uv_colors_kernel: tex[th-1-coord_u[v], coord_v[v], :] = uint8(clip(rint(colour[v]), 0, 255)) ----
// Several vertices share a texel; numpy's in-order assignment leaves the HIGHEST vertex index there.  Pass 1 (one thread per
// (face, vertex)) takes the maximum of v + 1 per texel into owner [F,th,tw] (zeroed); pass 2 (one thread per (face, texel))
// writes the owner's colour and mask 255, or zeros where no vertex landed.
__global__ __launch_bounds__(256) void uv_owner_kernel(const int *__restrict__ coord_u, const int *__restrict__ coord_v,
                                                       const unsigned char *__restrict__ visible, unsigned *__restrict__ owner,
                                                       int nver, int th, int tw) {
    const int v = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (v >= nver) return;
    if (visible && !visible[(size_t)f * nver + v]) return;
    atomicMax(&owner[((size_t)f * th + (th - 1 - coord_u[v])) * tw + coord_v[v]], (unsigned)v + 1u);
}

__global__ __launch_bounds__(256) void uv_scatter_kernel(const float *__restrict__ colors, const unsigned *__restrict__ owner,
                                                         unsigned char *__restrict__ tex, unsigned char *__restrict__ mask,
                                                         int nver, int texels, int ch) {
    const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (t >= texels) return;
    const size_t o = (size_t)f * texels + t;
    const unsigned own = owner[o];
    const float *col = colors + ((size_t)f * nver + (own ? own - 1 : 0)) * ch;
    for (int q = 0; q < ch; ++q) {
        const float c = own ? col[q] : 0.0f;
        tex[o * ch + q] = (unsigned char)fminf(fmaxf(rintf(c), 0.0f), 255.0f);
    }
    mask[o] = own ? 255 : 0;
}

// ---- Sim3DR's _render_texture_core (rasterize_kernel.cpp:353-458): the z-buffer walk that samples a texture IMAGE per pixel ----
// Keys are [order-preserving depth bits (32) | ~index (32)], index = triangle (a key plane per face) or face * ntri + triangle (shared:
// ONE plane for all faces = the reference called once per mesh, in order, on the same image and depth buffer).
// Pass 1, one thread per (face, triangle): the box walk of tri_depth_kernel with the line that is commented out there and live here
// (:418): on the two-pixel frame border the inside test is bypassed and the weights are extrapolated ((1,0,0) for zero area).
__global__ __launch_bounds__(256) void tex_depth_kernel(const float *__restrict__ vertices, const int *__restrict__ tri,
                                                        const float *__restrict__ depth0, unsigned long long *__restrict__ zkey,
                                                        int nver, int ntri, int h, int w, int planar, int shared) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= ntri) return;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    const int t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    const float p0x = vtx(v, planar, nver, t0, 0), p0y = vtx(v, planar, nver, t0, 1), d0 = vtx(v, planar, nver, t0, 2);
    const float p1x = vtx(v, planar, nver, t1, 0), p1y = vtx(v, planar, nver, t1, 1), d1 = vtx(v, planar, nver, t1, 2);
    const float p2x = vtx(v, planar, nver, t2, 0), p2y = vtx(v, planar, nver, t2, 1), d2 = vtx(v, planar, nver, t2, 2);
    const int x_min = max((int)ceilf(fminf(p0x, fminf(p1x, p2x))), 0), x_max = min((int)floorf(fmaxf(p0x, fmaxf(p1x, p2x))), w - 1);
    const int y_min = max((int)ceilf(fminf(p0y, fminf(p1y, p2y))), 0), y_max = min((int)floorf(fmaxf(p0y, fmaxf(p1y, p2y))), h - 1);
    if (x_max < x_min || y_max < y_min) return;
    const size_t plane = shared ? 0 : (size_t)f * h * w;
    const unsigned long long lo = (unsigned long long)~(shared ? (unsigned)f * (unsigned)ntri + (unsigned)i : (unsigned)i);
    for (int y = y_min; y <= y_max; ++y)
        for (int x = x_min; x <= x_max; ++x) {
            const Bary b = bary((float)x, (float)y, p0x, p0y, p1x, p1y, p2x, p2y);
            if (!(x < 2 || x > w - 3 || y < 2 || y > h - 3 || b.in)) continue;
            const float depth = b.w0 * d0 + b.w1 * d1 + b.w2 * d2;
            const size_t px = plane + (size_t)y * w + x;
            if (!(depth > depth0[px])) continue;
            atomicMax(&zkey[px], ((unsigned long long)depth_key(depth == 0.0f ? 0.0f : depth) << 32) | lo);
        }
}

namespace {
__device__ __forceinline__ void store_pixel(float *o, float v) { *o = v; }
__device__ __forceinline__ void store_pixel(unsigned char *o, float v) { *o = (unsigned char)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }
}  // namespace

// Pass 2, one thread per (key plane, pixel): where a key won, the weights and the depth of the winner re-derived with the same
// expressions, its texture coordinate (:427; x through tex_tri, y through the MESH triangle's indices, :393-398, row stride 3),
// the clamp (:428-429, written so that NaN becomes 0 -- the reference converts NaN to int there), the sample (:433-449) and the
// stores.  TexT float or uint8 (read as (float)byte), ImgT float or uint8 (uint8(clip(rint(v), 0, 255)), as uv_scatter_kernel).
template <typename TexT, typename ImgT>
__global__ __launch_bounds__(256) void tex_resolve_kernel(const float *__restrict__ vertices, const int *__restrict__ tri,
                                                          const int *__restrict__ tex_tri, const float *__restrict__ tex_coords,
                                                          const TexT *__restrict__ texture, const unsigned long long *__restrict__ zkey,
                                                          ImgT *__restrict__ image, float *__restrict__ depth, int nver, int ntri, int h,
                                                          int w, int c, int planar, int shared, int tex_per_face, int th, int tw, int tc,
                                                          int mapping) {
    const int px = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (px >= h * w) return;
    const size_t o = (size_t)g * h * w + px;
    const unsigned long long k = zkey[o];
    if (k == 0ull) return;
    unsigned idx = ~(unsigned)k;
    asm volatile("" : "+v"(idx));                            // the opaque copy of raster_shade_kernel (hipcc 7.2 mask loss)
    int f = g, i = (int)idx;
    if (shared) { f = (int)(idx / (unsigned)ntri); i = (int)(idx - (unsigned)f * (unsigned)ntri); }
    const int y = px / w, x = px % w;
    const float *v = vertices + (size_t)f * face_stride(planar, nver);
    const int t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    const Bary b = bary((float)x, (float)y, vtx(v, planar, nver, t0, 0), vtx(v, planar, nver, t0, 1), vtx(v, planar, nver, t1, 0),
                        vtx(v, planar, nver, t1, 1), vtx(v, planar, nver, t2, 0), vtx(v, planar, nver, t2, 1));
    depth[o] = b.w0 * vtx(v, planar, nver, t0, 2) + b.w1 * vtx(v, planar, nver, t1, 2) + b.w2 * vtx(v, planar, nver, t2, 2);
    float tx = b.w0 * tex_coords[3 * tex_tri[3 * i]] + b.w1 * tex_coords[3 * tex_tri[3 * i + 1]] + b.w2 * tex_coords[3 * tex_tri[3 * i + 2]];
    float ty = b.w0 * tex_coords[3 * t0 + 1] + b.w1 * tex_coords[3 * t1 + 1] + b.w2 * tex_coords[3 * t2 + 1];
    const float xhi = (float)(tw - 1), yhi = (float)(th - 1);
    tx = tx > xhi ? xhi : tx; tx = tx >= 0 ? tx : 0.0f;
    ty = ty > yhi ? yhi : ty; ty = ty >= 0 ? ty : 0.0f;
    const TexT *t = texture + (tex_per_face ? (size_t)f * th * tw * tc : 0);
    ImgT *out = image + o * c;
    if (mapping == 0) {
        const TexT *s = t + ((size_t)(int)roundf(ty) * tw + (int)roundf(tx)) * tc;
        for (int q = 0; q < c; ++q) store_pixel(out + q, (float)s[q]);
    } else {
        const float fx = floorf(tx), fy = floorf(ty);
        const float xd = tx - fx, yd = ty - fy;
        const size_t x0 = (size_t)(int)fx * tc, x1 = (size_t)(int)ceilf(tx) * tc;
        const TexT *r0 = t + (size_t)(int)fy * tw * tc, *r1 = t + (size_t)(int)ceilf(ty) * tw * tc;
        for (int q = 0; q < c; ++q)
            store_pixel(out + q, bilerp((float)r0[x0 + q], (float)r0[x1 + q], (float)r1[x0 + q], (float)r1[x1 + q], xd, yd));
    }
}

void launch_mesh_normals(const float *vertices, const int *tri, const int *adj_off, const int *adj_tri, float *tri_normal,
                         float *normal, unsigned *mm, int F, int nver, int ntri, int planar, hipStream_t s) {
    // per-face extrema start at +inf / -inf in key space
    (void)hipMemsetAsync(mm, 0, sizeof(unsigned) * 6 * F, s);
    (void)hipMemset2DAsync(mm, 6 * sizeof(unsigned), 0xff, 3 * sizeof(unsigned), F, s);
    tri_normal_kernel<<<dim3((ntri + 255) / 256, F), 256, 0, s>>>(vertices, tri, tri_normal, nver, ntri, planar);
    ver_normal_kernel<<<dim3((nver + 255) / 256, F), 256, 0, s>>>(tri_normal, adj_off, adj_tri, normal, nver, ntri);
    minmax_kernel<<<dim3(kMinMaxBlocks, F), 1024, 0, s>>>(vertices, mm, nver, planar);
}

void launch_mesh_lighting(const float *vertices, const float *normal, const unsigned *mm, const float *cfg, float *light, int F,
                          int nver, int planar, hipStream_t s) {
    lighting_kernel<<<dim3((nver + 255) / 256, F), 256, 0, s>>>(vertices, normal, mm, cfg, light, nver, planar);
}

void launch_mesh_lighting_tex(const float *vertices, const float *normal, const unsigned *mm, const float *cfg, float *light,
                              float *tex, int shared, float *colors, int F, int nver, int planar, hipStream_t s) {
    if (shared)
        lighting_tex_shared_kernel<<<(nver + 255) / 256, 256, 0, s>>>(vertices, normal, mm, cfg, light, tex, colors, F, nver, planar);
    else
        lighting_tex_kernel<<<dim3((nver + 255) / 256, F), 256, 0, s>>>(vertices, normal, mm, cfg, light, tex, colors, nver, planar);
}

void launch_uv_colors(const unsigned char *uv_tex, const int *coord_u, const int *coord_v, const int *keep, float *out, int T, int n,
                      int th, int tw, int ch, int normalize, hipStream_t s) {
    uv_colors_kernel<<<dim3((n + 255) / 256, T), 256, 0, s>>>(uv_tex, coord_u, coord_v, keep, out, n, th, tw, ch, normalize);
}

void launch_gather_vertices(const float *vertices, const int *keep, float *out, int F, int n_keep, int pitch, hipStream_t s) {
    gather_vertices_kernel<<<dim3((n_keep + 255) / 256, 3 * F), 256, 0, s>>>(vertices, keep, out, n_keep, pitch);
}

void launch_rasterize(const float *vertices, const int *tri, const float *colors, unsigned long long *zkey, unsigned char *image,
                      int F, int nver, int ntri, int h, int w, int c, int planar, int reverse, hipStream_t s) {
    (void)hipMemsetAsync(zkey, 0, sizeof(unsigned long long) * (size_t)h * w, s);
    raster_depth_kernel<<<dim3((ntri + 255) / 256, F), 256, 0, s>>>(vertices, tri, zkey, nver, ntri, h, w, planar);
    raster_shade_kernel<<<(h * w + 255) / 256, 256, 0, s>>>(vertices, tri, colors, zkey, image, nver, h, w, c, planar, reverse);
}

void launch_rasterize_triangles(const float *vertices, const int *tri, unsigned long long *zkey, float *depth, int *tri_buf,
                                float *weight, int F, int nver, int ntri, int h, int w, int planar, hipStream_t s) {
    (void)hipMemsetAsync(zkey, 0, sizeof(unsigned long long) * (size_t)F * h * w, s);
    tri_depth_kernel<<<dim3((ntri + 255) / 256, F), 256, 0, s>>>(vertices, tri, depth, zkey, nver, ntri, h, w, planar);
    tri_resolve_kernel<<<dim3((h * w + 255) / 256, F), 256, 0, s>>>(vertices, tri, zkey, depth, tri_buf, weight, nver, h, w, planar);
}

void launch_render_texture(const float *vertices, const int *tri, const int *tex_tri, const float *tex_coords, const void *texture,
                           int tex_u8, int tex_per_face, int th, int tw, int tc, int mapping, unsigned long long *zkey, void *image,
                           int image_u8, float *depth, int F, int nver, int ntri, int h, int w, int c, int planar, int shared,
                           hipStream_t s) {
    const int planes = shared ? 1 : F;
    (void)hipMemsetAsync(zkey, 0, sizeof(unsigned long long) * (size_t)planes * h * w, s);
    tex_depth_kernel<<<dim3((ntri + 255) / 256, F), 256, 0, s>>>(vertices, tri, depth, zkey, nver, ntri, h, w, planar, shared);
    const dim3 grid((h * w + 255) / 256, planes);
#define SYN_TEX_RESOLVE(TexT, ImgT)                                                                                                 \
    tex_resolve_kernel<TexT, ImgT><<<grid, 256, 0, s>>>(vertices, tri, tex_tri, tex_coords, (const TexT *)texture, zkey, (ImgT *)image, \
                                                        depth, nver, ntri, h, w, c, planar, shared, tex_per_face, th, tw, tc, mapping)
    if (tex_u8) { if (image_u8) SYN_TEX_RESOLVE(unsigned char, unsigned char); else SYN_TEX_RESOLVE(unsigned char, float); }
    else { if (image_u8) SYN_TEX_RESOLVE(float, unsigned char); else SYN_TEX_RESOLVE(float, float); }
#undef SYN_TEX_RESOLVE
}

void launch_vertex_visibility(const int *tri_buf, const int *tri, unsigned char *visible, int F, int nver, int ntri, int h, int w,
                              hipStream_t s) {
    (void)hipMemsetAsync(visible, 0, (size_t)F * nver, s);
    vertex_visible_kernel<<<dim3((h * w + 255) / 256, F), 256, 0, s>>>(tri_buf, tri, visible, nver, ntri, h * w);
}

void launch_sample_vertex_colors(const float *vertices, const unsigned char *image, float *out, int F, int nver, int h, int w, int ch,
                                 int planar, int normalize, hipStream_t s) {
    sample_vertex_colors_kernel<<<dim3((nver + 255) / 256, F), 256, 0, s>>>(vertices, image, out, nver, h, w, ch, planar, normalize);
}

void launch_uv_scatter(const float *colors, const unsigned char *visible, const int *coord_u, const int *coord_v, unsigned *owner,
                       unsigned char *tex, unsigned char *mask, int F, int nver, int th, int tw, int ch, hipStream_t s) {
    (void)hipMemsetAsync(owner, 0, sizeof(unsigned) * (size_t)F * th * tw, s);
    uv_owner_kernel<<<dim3((nver + 255) / 256, F), 256, 0, s>>>(coord_u, coord_v, visible, owner, nver, th, tw);
    uv_scatter_kernel<<<dim3((th * tw + 255) / 256, F), 256, 0, s>>>(colors, owner, tex, mask, nver, th * tw, ch);
}

void launch_add_weighted(const unsigned char *a, float alpha, const unsigned char *b, float beta, unsigned char *out, size_t n,
                         hipStream_t s) {
    add_weighted_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a, alpha, b, beta, out, n);
}

}  // namespace syn
