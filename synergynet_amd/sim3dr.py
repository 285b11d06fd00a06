"""Mesh consumers on the GPU: the reference's Sim3DR package and utils/render.py.

Same names, argument meaning and return types as the reference:
  get_normal(vertices, triangles)                          Sim3DR/Sim3DR.py:8-11
  rasterize(vertices, triangles, colors, bg=..., ...)      Sim3DR/Sim3DR.py:14-29
  RenderPipeline(**cfg)(vertices, triangles, bg, texture)  Sim3DR/lighting.py:23-71
  render(img, ver_lst, alpha=0.6, tex=None, connectivity=None)   utils/render.py:31-50 (returns the blended image; no files)
numpy in, numpy out, like the reference -- but every stage runs in HIP kernels through the C ABI
(syn_load_triangles / syn_mesh_shade / syn_rasterize / syn_add_weighted, csrc/render_kernels.hip) on the most recently
constructed SynergyNet's handle; there is no CPU fallback.  `render_batch` is the device-resident entry: meshes as the
[F,3,N] tensor `reconstruct(..., dense=True)` returns, no transposes, no host copies.

Textured meshes (the reference's uv_texture_realFaces.py / artistic.py): `uv_vertex_colors` looks one colour per vertex up in
a UV texture image, `render_batch(..., uv_tex= | tex=)` gathers the kept vertex subset, multiplies texture and light in the
lighting kernel and draws the kept topology -- syn_load_uv_map / syn_uv_colors / syn_gather_vertices / syn_mesh_shade_textured,
all on the device.  The handle keeps two topology slots (full mesh, kept mesh); `model._topology_uploads` counts the uploads.

Visibility buffers: `rasterize_triangles` is the third entry point of the reference's binding (Sim3DR/lib/rasterize.pyx:74-86: per
pixel the winning triangle, its barycentric weights and its depth, written into the caller's arrays).  `visibility_batch` is its
device-resident form plus the per-vertex visibility that follows from it, `vertex_colors_from_image` samples one colour per vertex
from a frame, and `texture_from_image` chains them into a UV texture image (and its mask of written texels) -- what
`render_batch(uv_tex=)` and `uv_vertex_colors` consume.  syn_rasterize_triangles / syn_vertex_visibility /
syn_sample_vertex_colors / syn_uv_scatter.  `fill_texture` (and `texture_from_image(fill=True)`) completes the texels no vertex
wrote by a push-pull over the texture's pyramid, optionally merging several views of one face first: syn_texture_fill.

Per-pixel texture mapping: `render_texture_core` is the last compute entry of the reference's binding (its `_render_texture_core`,
commented out in rasterize.pyx:104-123): a z-buffer walk that samples the texture IMAGE per pixel, nearest or bilinear, so nothing
between the vertices is thrown away.  `render_texture_batch` is its device-resident form for F meshes and the model's UV map
(`uv_tex_coords`), all faces in one z-buffer or each in its own planes: syn_load_tex_coords / syn_render_texture.
"""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import torch

from . import abi
from . import inference as _inf

RENDER_CFG = dict(intensity_ambient=0.75, color_ambient=(1, 1, 1), intensity_directional=0.7, color_directional=(1, 1, 1),
                  intensity_specular=0.2, specular_exp=5, light_pos=(0, 0, 5), view_pos=(0, 0, 5))      # utils/render.py:18-27


def _model():
    return _inf._model()


def _triangles(m, triangles):
    """Upload the topology when it differs from the one the handle holds (the reference passes it on every call)."""
    t = np.ascontiguousarray(np.asarray(triangles), dtype=np.int32)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError('triangles must be [ntri,3] (0-based), as Sim3DR takes them')
    key = (t.shape[0], zlib.crc32(t.tobytes()))          # content hash: the reference passes the array on every call
    return t, key


def _count_upload(m, slot):
    """`model._topology_uploads` = [uploads of the syn_load_triangles slot, uploads of the kept slot of syn_load_uv_map]."""
    if not hasattr(m, '_topology_uploads'):
        m._topology_uploads = [0, 0]
    m._topology_uploads[slot] += 1


def _texc_keys(m):
    """What the two topology slots hold as texture coordinates (syn_load_tex_coords); `model._tex_coord_uploads` counts the uploads."""
    if not hasattr(m, '_texc_key'):
        m._texc_key, m._tex_coord_uploads = [None, None], [0, 0]
    return m._texc_key


def _ensure_tex_coords(m, slot, key, make):
    """The texture coordinates `make()` returns ([tex_nver,3] float32, [ntri,3] int32 or None) in topology slot `slot`, selected;
    uploaded when `key` differs from what the slot holds."""
    _select(m, slot)
    if _texc_keys(m)[slot] != key:
        tc, tt = make()
        abi.check(m._lib.syn_load_tex_coords(m._h, tc.ctypes.data_as(C.c_void_p), tc.shape[0],
                                             tt.ctypes.data_as(C.c_void_p) if tt is not None else None))
        m._texc_key[slot] = key
        m._tex_coord_uploads[slot] += 1


def _select(m, slot):
    """Point syn_mesh_shade* / syn_rasterize at a topology slot (0: syn_load_triangles, 1: the kept mesh); a host-side switch."""
    abi.check(m._lib.syn_select_topology(m._h, slot))


def _ensure_topology(m, triangles, nver):
    t, key = _triangles(m, triangles)
    if getattr(m, '_tri_key', None) != (key, nver):
        abi.check(m._lib.syn_load_triangles(m._h, t.ctypes.data_as(C.c_void_p), t.shape[0], nver))
        m._tri_key = (key, nver)
        _count_upload(m, 0)
        _texc_keys(m)[0] = None                          # the handle drops a slot's texture coordinates with its topology
    _select(m, 0)
    return t


def _ensure_uv_map(m):
    """Upload the model's UV assets (param_pack.uv_vert / keep_ind / tri_deletion) once: pixel tables, kept vertices and the
    kept topology in the handle's second slot.  Returns (n_vert, n_keep)."""
    pp = getattr(m, 'param_pack', None)
    if pp is None or getattr(pp, 'uv_vert', None) is None or pp.keep_ind is None or pp.tri_deletion is None:
        raise RuntimeError('Missing data: the model has no UV assets (BFM_UV.npy, keptInd.npy, deletedTri.npy)')
    objs = (pp.uv_vert, pp.keep_ind, pp.tri_deletion)
    held = getattr(m, '_uv_key', None)
    if held is None or any(a is not b for a, b in zip(held[0], objs)):
        from .params import uv_pixel_coords
        cu, cv = (np.ascontiguousarray(a, dtype=np.int32) for a in uv_pixel_coords(pp.uv_vert))
        keep = np.asarray(pp.keep_ind).reshape(-1)
        td = np.asarray(pp.tri_deletion)
        if td.ndim != 2 or td.shape[0] != 3:
            raise ValueError('tri_deletion must be [3,ntri] (1-based), as deletedTri.npy holds it')
        keep = np.ascontiguousarray(keep, dtype=np.int32)
        tri = np.ascontiguousarray(td.T.astype(np.int64) - 1, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        abi.check(m._lib.syn_load_uv_map(m._h, ptr(cu), ptr(cv), cu.size, ptr(keep), keep.size, ptr(tri), tri.shape[0]))
        m._uv_key = (objs, cu.size, keep.size)
        _count_upload(m, 1)
        _texc_keys(m)[1] = None
    return m._uv_key[1], m._uv_key[2]


def _cfg16(pipe):
    f = lambda v: [float(x) for x in np.asarray(v, dtype=np.float32).reshape(-1)]
    vals = ([float(np.float32(pipe.intensity_ambient))] + f(pipe.color_ambient) + [float(np.float32(pipe.intensity_directional))] +
            f(pipe.color_directional) + [float(np.float32(pipe.intensity_specular)), float(pipe.specular_exp)] +
            f(pipe.light_pos) + f(pipe.view_pos))
    return (C.c_float * 16)(*vals)


def _planar_arg(meshes):
    """The ABI's `planar` argument for a [F,3,N] float32 device tensor: 1 for packed rows, the row pitch for the pitched view
    reconstruct() returns ([F,3,pitch][:, :, :N]); anything else (non-unit column stride, unevenly spaced faces) is refused."""
    F, three, n = meshes.shape
    pitch = meshes.stride(1) if n > 1 else n
    if three != 3 or meshes.dtype != torch.float32 or (n > 1 and meshes.stride(2) != 1) or pitch < n or (F > 1 and meshes.stride(0) != 3 * pitch):
        raise RuntimeError('meshes must be a float32 [F,3,N] tensor with unit column stride and equally pitched rows')
    return 1 if pitch == n else int(pitch)


def _shade(m, verts_t, planar, cfg=None):
    """verts_t: device tensor [F,3,N] (planar: 1 packed, > 1 row pitch) or [F,N,3]; returns (normal, light or None) device
    tensors [F,N,3]."""
    F = verts_t.shape[0]
    n = verts_t.shape[2] if planar else verts_t.shape[1]
    normal = torch.empty((F, n, 3), dtype=torch.float32, device=m.device)
    light = torch.empty_like(normal) if cfg is not None else None
    with torch.cuda.device(m.device):
        abi.check(m._lib.syn_mesh_shade(m._h, verts_t.data_ptr(), F, int(planar), cfg, normal.data_ptr(),
                                        light.data_ptr() if light is not None else None, m._stream()))
    return normal, light


def _shade_textured(m, verts_t, planar, cfg, tex_t, shared, want_light=False):
    """Normals + Phong light with `texture *= light` (lighting.py:68-70) in the kernel's epilogue, on the selected topology.
    tex_t: float32 device tensor, [n,3] when shared (multiplied in place face after face, like the reference's caller array) or
    [F,n,3].  Returns (normal, light or None, colours [F,n,3])."""
    F = verts_t.shape[0]
    n = verts_t.shape[2] if planar else verts_t.shape[1]
    if tex_t.dtype != torch.float32 or not tex_t.is_contiguous() or tuple(tex_t.shape) != ((n, 3) if shared else (F, n, 3)):
        raise ValueError(f'tex must be a contiguous float32 [{n},3] or [{F},{n},3] array (one colour per vertex of the mesh), got '
                         f'{tuple(tex_t.shape)} {tex_t.dtype}')
    normal = torch.empty((F, n, 3), dtype=torch.float32, device=m.device)
    light = torch.empty_like(normal) if want_light else None
    colors = torch.empty_like(normal)
    with torch.cuda.device(m.device):
        abi.check(m._lib.syn_mesh_shade_textured(m._h, verts_t.data_ptr(), F, int(planar), cfg, normal.data_ptr(),
                                                 light.data_ptr() if light is not None else None, tex_t.data_ptr(), int(shared),
                                                 colors.data_ptr(), m._stream()))
    return normal, light, colors


def _tex_arg(m, tex, F, n):
    """A caller's texture as (device tensor, shared?, host array to update afterwards or None).  numpy arrays are the
    reference's calling convention ([n,3] float32, multiplied in place); device tensors stay on the device."""
    if isinstance(tex, torch.Tensor):
        t, back = tex, None
        if t.device != m.device:
            raise ValueError(f'tex tensor must live on {m.device}')
    else:
        if not isinstance(tex, np.ndarray) or tex.dtype != np.float32:
            raise TypeError('tex must be a float32 numpy array or device tensor (the reference multiplies it in place)')
        t, back = torch.from_numpy(np.ascontiguousarray(tex)).to(m.device), tex
    if t.dim() not in (2, 3) or tuple(t.shape[-2:]) != (n, 3) or (t.dim() == 3 and t.shape[0] != F):
        raise ValueError(f'tex must be [{n},3] or [{F},{n},3] (one colour per vertex of the mesh), got {tuple(t.shape)}')
    return t, t.dim() == 2, back


def uv_vertex_colors(model, uv_tex, kept=True, normalize=False):
    """One colour per vertex from a UV texture image (uv_texture_realFaces.py:48-49,109-115): uv_tex uint8 [H,W,ch] or
    [T,H,W,ch] (array or device tensor, rows as cv2.imread delivers them -- the flip of :109 is part of the lookup).  Returns a
    float32 device tensor [n,ch] / [T,n,ch], n = the kept vertices (kept=True: `colors_uv[keep_ind]`) or all of them; values
    0..255 (what write_obj_with_colors takes) or / 255 with normalize=True (what render takes as `tex`)."""
    _ensure_uv_map(model)
    t = uv_tex if isinstance(uv_tex, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(uv_tex))
    if t.dtype != torch.uint8 or t.dim() not in (3, 4):
        raise TypeError('uv_tex must be uint8 [H,W,ch] or [T,H,W,ch]')
    t = t.to(model.device).contiguous()
    t4 = t if t.dim() == 4 else t[None]
    T, th, tw, ch = t4.shape
    n = model._uv_key[2] if kept else model._uv_key[1]
    out = torch.empty((T, n, ch), dtype=torch.float32, device=model.device)
    with torch.cuda.device(model.device):
        abi.check(model._lib.syn_uv_colors(model._h, t4.data_ptr(), T, th, tw, ch, int(bool(kept)), int(bool(normalize)),
                                           out.data_ptr(), model._stream()))
    return out if t.dim() == 4 else out[0]


def gather_kept(model, meshes):
    """meshes[:, :, keep_ind] on the device (uv_texture_realFaces.py:98): [F,3,N] float32, packed or the pitched view
    reconstruct() returns (read in place) -> packed [F,3,n_keep]."""
    n_vert, n_keep = _ensure_uv_map(model)
    if meshes.shape[2] != n_vert:
        raise ValueError(f'meshes have {meshes.shape[2]} vertices, the UV map {n_vert}')
    planar = _planar_arg(meshes)
    out = torch.empty((meshes.shape[0], 3, n_keep), dtype=torch.float32, device=model.device)
    with torch.cuda.device(model.device):
        abi.check(model._lib.syn_gather_vertices(model._h, meshes.data_ptr(), meshes.shape[0], planar, out.data_ptr(), model._stream()))
    return out


def _ensure_model_topology(model, n):
    """The model's `triangles` in topology slot 0 (uploaded when the attribute or the vertex count changed), selected."""
    if getattr(model, '_tri_obj', None) is not model.triangles or getattr(model, '_tri_key', (None, None))[1] != n:
        t = np.asarray(model.triangles)                  # the class attribute is [3,ntri] (synergy3DMM.py:105), Sim3DR wants [ntri,3]
        _ensure_topology(model, np.ascontiguousarray(t.T if t.shape[0] == 3 else t), n)
        model._tri_obj = model.triangles                 # same object next time: skip the host-side comparison
    _select(model, 0)


def _raster_triangles(m, verts_t, F, planar, depth, tri, bary, height, width):
    with torch.cuda.device(m.device):
        abi.check(m._lib.syn_rasterize_triangles(m._h, verts_t.data_ptr(), F, int(planar), depth.data_ptr(), tri.data_ptr(),
                                                 bary.data_ptr(), height, width, m._stream()))


def rasterize_triangles(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight, ntri, h, w):
    """Sim3DR/lib/rasterize.pyx:74-86, the binding's own signature: vertices [nver,3] float32, triangles [>= ntri,3] int32 and three
    C-contiguous arrays the CALLER initialises (usually -1e8, -1 and 0) and that are updated in place: depth_buffer float32 and
    triangle_buffer int32 of h*w elements, barycentric_weight float32 of h*w*3.  Where a triangle is deeper than depth_buffer the
    pixel gets its depth, index and weights; every other element keeps the caller's value."""
    m = _model()
    for a, dt, n, name in ((depth_buffer, np.float32, h * w, 'depth_buffer'), (triangle_buffer, np.int32, h * w, 'triangle_buffer'),
                           (barycentric_weight, np.float32, h * w * 3, 'barycentric_weight')):
        if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or a.size != n:
            raise TypeError(f'{name} must be a C-contiguous {np.dtype(dt).name} array of {n} elements (rasterize.pyx:74-86)')
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    t = np.asarray(triangles)
    if not 0 < ntri <= t.shape[0]:
        raise ValueError(f'ntri={ntri} with {t.shape[0]} triangles')
    _ensure_topology(m, t[:ntri], v.shape[0])
    m._tri_obj = None                                    # slot 0 may no longer hold the model's own topology: render_batch re-checks
    dev =[torch.from_numpy(a.reshape(-1)).to(m.device) for a in (depth_buffer, triangle_buffer, barycentric_weight)]
    _raster_triangles(m, torch.from_numpy(v).to(m.device), 1, 0, dev[0], dev[1], dev[2], h, w)
    for a, d in zip((depth_buffer, triangle_buffer, barycentric_weight), dev):
        a.reshape(-1)[...] = d.cpu().numpy()


def _visibility(model, meshes, height, width):
    F, _, n = meshes.shape
    _ensure_model_topology(model, n)
    planar = _planar_arg(meshes)
    dev = model.device
    depth = torch.full((F, height, width), -1e8, dtype=torch.float32, device=dev)       # the binding's usual initial values
    tri = torch.full((F, height, width), -1, dtype=torch.int32, device=dev)
    bary = torch.zeros((F, height, width, 3), dtype=torch.float32, device=dev)
    visible = torch.empty((F, n), dtype=torch.uint8, device=dev)
    _raster_triangles(model, meshes, F, planar, depth, tri, bary, height, width)
    with torch.cuda.device(dev):
        abi.check(model._lib.syn_vertex_visibility(model._h, tri.data_ptr(), F, height, width, visible.data_ptr(), model._stream()))
    return depth, tri, bary, visible


def visibility_batch(model, meshes, height, width):
    """Visibility buffers of F meshes on the device: meshes [F,3,N] float32 device tensor in image coordinates (what
    reconstruct(..., dense=True) returns; pitched rows are read in place), topology = the model's `triangles`, uploaded once.
    Returns (depth [F,H,W] float32, -1e8 where nothing was drawn; tri [F,H,W] int32, -1 there; bary [F,H,W,3] float32, 0 there;
    visible [F,N] bool: the vertex is a corner of a triangle that won a pixel)."""
    depth, tri, bary, visible = _visibility(model, meshes, int(height), int(width))
    return depth, tri, bary, visible.view(torch.bool)


def _frame(model, img):
    t = (img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img)))
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] > 4:
        raise TypeError('img must be uint8 [H,W,ch] with ch <= 4')
    return t.to(model.device).contiguous()


def vertex_colors_from_image(model, img, meshes, normalize=False):
    """One colour per vertex from a frame: img uint8 [H,W,ch] (array or device tensor), meshes [F,3,N] float32 device tensor in the
    frame's pixel coordinates.  Bilinear sample at the vertex' (x, y), clamped to the frame, in the float32 operation order of the
    reference's bilinear code (rasterize_kernel.cpp:428-447).  Returns a float32 device tensor [F,N,ch], 0..255 or / 255 with
    normalize=True; a vertex with a non-finite coordinate gets 0."""
    F, _, n = meshes.shape
    _ensure_model_topology(model, n)
    planar = _planar_arg(meshes)
    img_t = _frame(model, img)
    H, W, ch = img_t.shape
    out = torch.empty((F, n, ch), dtype=torch.float32, device=model.device)
    with torch.cuda.device(model.device):
        abi.check(model._lib.syn_sample_vertex_colors(model._h, meshes.data_ptr(), F, planar, img_t.data_ptr(), H, W, ch,
                                                      int(bool(normalize)), out.data_ptr(), model._stream()))
    return out


def _u8(model, a, what, allow_bool=False):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if allow_bool and t.dtype == torch.bool:
        t = t.view(torch.uint8)                                 # same bytes: False 0, True 1
    if t.dtype != torch.uint8:
        raise TypeError(f'{what} must be uint8')
    return t.to(model.device).contiguous()


def fill_texture(model, uv_tex, mask, merge=False):
    """Fills the texels of UV textures that `mask` marks as not written (0), by a deterministic push-pull over the texture's pyramid
    (syn_texture_fill; DESIGN 5.5c has the definition, integer arithmetic only): written texels keep their value, every other texel
    gets a smooth blend of the written ones around it, the nearest ones weighing most; a texture without a written texel comes out 0.
    uv_tex uint8 [H,W,ch] or [T,H,W,ch] with ch <= 4 and H, W <= 4096, mask uint8 (or bool) [H,W] / [T,H,W]; arrays or device tensors.
    merge=True takes T views of ONE face ([T,H,W,ch], e.g. the frames of a video): a texel seen by several views gets their rounded
    mean before the holes no view saw are filled.  Returns a uint8 device tensor of the input's shape, or [H,W,ch] with merge; the
    inputs are not modified.  Three kernel launches whatever T."""
    t = _u8(model, uv_tex, 'uv_tex')
    mk = _u8(model, mask, 'mask', allow_bool=True)
    if t.dim() not in (3, 4) or tuple(mk.shape) != tuple(t.shape[:-1]):
        raise ValueError(f'uv_tex must be [H,W,ch] or [T,H,W,ch] and mask its shape without the channels, got {tuple(t.shape)} and '
                         f'{tuple(mk.shape)}')
    if merge and t.dim() != 4:
        raise ValueError('merge takes the views as one [T,H,W,ch] array')
    t4 = t if t.dim() == 4 else t[None]
    T, th, tw, ch = t4.shape
    out = torch.empty((1 if merge else T, th, tw, ch), dtype=torch.uint8, device=model.device)
    with torch.cuda.device(model.device):
        abi.check(model._lib.syn_texture_fill(model._h, t4.data_ptr(), mk.data_ptr(), T, th, tw, ch, int(bool(merge)), out.data_ptr(),
                                              model._stream()))
    return out[0] if merge or t.dim() == 3 else out


def texture_from_image(model, img, meshes, tex_hw=256, occlusion=True, fill=False):
    """From a photograph and the meshes reconstructed from it to UV texture images: every vertex takes its colour from the frame
    (vertex_colors_from_image) and writes it to its texel of the model's UV map (param_pack.uv_vert), the inverse of
    uv_vertex_colors.  occlusion=True writes only the vertices visibility_batch finds visible at the frame's size; texels no
    vertex writes stay 0 unless fill=True, which completes them from the written ones (fill_texture).  Where vertices share a
    texel the highest vertex index wins.
    tex_hw: texture size, an int or (height, width).  Returns (uv_tex uint8 [F,th,tw,ch], mask uint8 [F,th,tw], 255 where a vertex
    wrote -- also with fill=True), device tensors; uv_tex is what render_batch(uv_tex=) and uv_vertex_colors take.  Nothing is
    downloaded in between."""
    F, _, n = meshes.shape
    n_vert, _ = _ensure_uv_map(model)
    if n != n_vert:
        raise ValueError(f'meshes have {n} vertices, the UV map {n_vert}')
    th, tw = (int(tex_hw), int(tex_hw)) if np.isscalar(tex_hw) else (int(tex_hw[0]), int(tex_hw[1]))
    img_t = _frame(model, img)
    H, W, ch = img_t.shape
    colors = vertex_colors_from_image(model, img_t, meshes)
    visible = _visibility(model, meshes, H, W)[3] if occlusion else None
    tex = torch.empty((F, th, tw, ch), dtype=torch.uint8, device=model.device)
    mask = torch.empty((F, th, tw), dtype=torch.uint8, device=model.device)
    with torch.cuda.device(model.device):
        abi.check(model._lib.syn_uv_scatter(model._h, colors.data_ptr(), visible.data_ptr() if visible is not None else None, F, ch,
                                            tex.data_ptr(), mask.data_ptr(), th, tw, model._stream()))
    return (fill_texture(model, tex, mask) if fill else tex), mask


def _render_texture(m, verts_t, F, planar, tex_t, mapping, image, depth, shared):
    T, th, tw, tc = tex_t.shape
    H, W, c = image.shape[-3:]
    with torch.cuda.device(m.device):
        abi.check(m._lib.syn_render_texture(m._h, verts_t.data_ptr(), F, int(planar), tex_t.data_ptr(), int(tex_t.dtype == torch.uint8), T, th,
                                            tw, tc, int(mapping), image.data_ptr(), int(image.dtype == torch.uint8), depth.data_ptr(), H, W,
                                            c, int(bool(shared)), m._stream()))


def render_texture_core(image, vertices, triangles, texture, tex_coords, tex_triangles, depth_buffer, nver, tex_nver, ntri, h, w, c,
                        tex_h, tex_w, tex_c, mapping_type):
    """The argument list of the reference's (commented-out) binding, Sim3DR/lib/rasterize.pyx:104-123 -> rasterize_kernel.cpp:353-458:
    image float32 [h,w,c] and depth_buffer float32 [h,w] are C-contiguous arrays the CALLER initialises and that are updated in place;
    vertices [nver,3] float32, triangles [>= ntri,3] int32, texture float32 [tex_h,tex_w,tex_c], tex_coords [tex_nver,3] float32 (x =
    texture column, y = row), tex_triangles [>= ntri,3] int32, mapping_type 0 nearest / 1 bilinear.  Where a triangle is deeper than
    depth_buffer the pixel gets the texture's colour at its interpolated coordinate and the depth; every other element keeps the
    caller's value.  include/synergy_hip.h states the semantics, the reference's three quirks included."""
    m = _model()
    for a, n, name in ((image, h * w * c, 'image'), (depth_buffer, h * w, 'depth_buffer')):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or a.size != n:
            raise TypeError(f'{name} must be a C-contiguous float32 array of {n} elements (rasterize.pyx:104-123)')
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    t, tt = np.asarray(triangles), np.asarray(tex_triangles)
    tex = np.ascontiguousarray(texture, dtype=np.float32)
    tc = np.ascontiguousarray(tex_coords, dtype=np.float32)
    if not 0 < ntri <= min(t.shape[0], tt.shape[0]):
        raise ValueError(f'ntri={ntri} with {t.shape[0]} triangles and {tt.shape[0]} tex_triangles')
    if v.shape != (nver, 3) or tc.shape != (tex_nver, 3) or tex.size != tex_h * tex_w * tex_c:
        raise ValueError('vertices must be [nver,3], tex_coords [tex_nver,3] and texture [tex_h,tex_w,tex_c]')
    _ensure_topology(m, t[:ntri], nver)
    m._tri_obj = None                                    # slot 0 may no longer hold the model's own topology: render_batch re-checks
    tt = np.ascontiguousarray(tt[:ntri], dtype=np.int32)
    _ensure_tex_coords(m, 0, ('arrays', tex_nver, zlib.crc32(tc.tobytes()), zlib.crc32(tt.tobytes())), lambda: (tc, tt))
    img_d = torch.from_numpy(image.reshape(h, w, c)).to(m.device)
    dep_d = torch.from_numpy(depth_buffer.reshape(h, w)).to(m.device)
    _render_texture(m, torch.from_numpy(v).to(m.device), 1, 0, torch.from_numpy(tex.reshape(1, tex_h, tex_w, tex_c)).to(m.device),
                    mapping_type, img_d, dep_d, True)
    image.reshape(-1)[...] = img_d.cpu().numpy().reshape(-1)
    depth_buffer.reshape(-1)[...] = dep_d.cpu().numpy().reshape(-1)


def uv_tex_coords(model, tex_h, tex_w, kept=False):
    """The texture coordinates of the model's UV asset for a tex_h x tex_w texture, [n,3] float32 (n = all vertices, or the kept subset):
    x = uv[:,0] * (tex_w-1), y = (tex_h-1) - uv[:,1] * (tex_h-1), z = 0, evaluated in the asset's own dtype and cast once.  The
    continuous counterpart of params.uv_pixel_coords plus the row flip of the UV lookup: a texture from texture_from_image lands where
    it was taken from."""
    pp = getattr(model, 'param_pack', None)
    if pp is None or getattr(pp, 'uv_vert', None) is None:
        raise RuntimeError('Missing data: the model has no UV asset (BFM_UV.npy)')
    uv = np.asarray(pp.uv_vert)
    x, y = uv[:, 0] * (int(tex_w) - 1), (int(tex_h) - 1) - uv[:, 1] * (int(tex_h) - 1)
    out = np.stack([x, y, np.zeros_like(x)], 1).astype(np.float32)
    if kept:
        if pp.keep_ind is None:
            raise RuntimeError('Missing data: the model has no kept-vertex list (keptInd.npy)')
        out = out[np.asarray(pp.keep_ind).reshape(-1)]
    return np.ascontiguousarray(out)


def render_texture_batch(model, meshes, uv_tex, height=None, width=None, background=None, mapping='bilinear', shared=True, kept=False):
    """Per-pixel textured render of F meshes on the device.  meshes [F,3,N] float32 device tensor in image coordinates (what
    reconstruct(..., dense=True) returns; pitched rows are read in place); uv_tex the UV texture image, uint8 or float32, [th,tw,c] (one
    for all faces) or [F,th,tw,c] -- what texture_from_image / fill_texture produce; its texture coordinates are uv_tex_coords(model,
    th, tw), uploaded once per (topology slot, texture size).  mapping 'nearest' or 'bilinear'.
    shared=True: ONE image [H,W,c] and depth [H,W]; all faces compete in one z-buffer (proper occlusion between faces; the earliest
    face wins among equal depths).  shared=False: [F,H,W,c] and [F,H,W], every face its own planes.
    background: uint8 or float32 [H,W,c] (or [F,H,W,c] with shared=False), copied, decides the image dtype and c <= the texture's
    channels; default zeros float32 of height x width with the texture's channels.  A uint8 image stores uint8(clip(rint(v), 0, 255)).
    kept=True draws the model's kept vertex subset with the kept topology.  Returns (image, depth) device tensors; depth is -1e8 where
    nothing was drawn."""
    F, _, n = meshes.shape
    tex_t = uv_tex if isinstance(uv_tex, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(uv_tex))
    if tex_t.dtype not in (torch.uint8, torch.float32) or tex_t.dim() not in (3, 4) or tex_t.shape[-1] > 4:
        raise TypeError('uv_tex must be uint8 or float32, [th,tw,c] or [F,th,tw,c] with c <= 4')
    tex_t = tex_t.to(model.device).contiguous()
    tex_t = tex_t if tex_t.dim() == 4 else tex_t[None]
    if tex_t.shape[0] not in (1, F):
        raise ValueError(f'{tex_t.shape[0]} textures for {F} faces (one, or one per face)')
    mapping_type = {'nearest': 0, 'bilinear': 1}.get(mapping)
    if mapping_type is None:
        raise ValueError("mapping must be 'nearest' or 'bilinear'")
    th, tw = int(tex_t.shape[1]), int(tex_t.shape[2])
    if kept:
        meshes = gather_kept(model, meshes)
    else:
        _ensure_model_topology(model, n)
    slot = 1 if kept else 0
    uv = model.param_pack.uv_vert
    _ensure_tex_coords(model, slot, ('uv', th, tw, id(uv)), lambda: (uv_tex_coords(model, th, tw, kept=kept), None))
    model._texc_uv = uv                                  # held, so that its id stays its own
    planar = _planar_arg(meshes)
    lead = () if shared else (F,)
    if background is None:
        if height is None or width is None:
            raise ValueError('give height and width, or a background')
        image = torch.zeros(lead + (int(height), int(width), int(tex_t.shape[3])), dtype=torch.float32, device=model.device)
    else:
        bg = background if isinstance(background, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(background))
        if bg.dtype not in (torch.uint8, torch.float32) or bg.dim() not in (3, 4) or (bg.dim() == 4 and (shared or bg.shape[0] != F)):
            raise TypeError('background must be uint8 or float32 [H,W,c] (or [F,H,W,c] with shared=False)')
        bg = bg.to(model.device)
        image = (bg.expand(lead + tuple(bg.shape)) if bg.dim() == 3 else bg).contiguous().clone()
    depth = torch.full(tuple(image.shape[:-1]), -1e8, dtype=torch.float32, device=model.device)
    _render_texture(model, meshes, F, planar, tex_t, mapping_type, image, depth, shared)
    return image, depth


def get_normal(vertices, triangles):
    """Sim3DR/Sim3DR.py:8-11: vertices [nver,3] float32, triangles [ntri,3] int32 -> normals [nver,3] float32."""
    m = _model()
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    _ensure_topology(m, triangles, v.shape[0])
    vt = torch.from_numpy(v).to(m.device)[None]
    normal, _ = _shade(m, vt, planar=False)
    return normal[0].cpu().numpy()


def rasterize(vertices, triangles, colors, bg=None, height=None, width=None, channel=None, reverse=False):
    """Sim3DR/Sim3DR.py:14-29 (bg is drawn into and returned, like the reference's in-place Cython call)."""
    m = _model()
    if bg is not None:
        height, width, channel = bg.shape
    else:
        assert height is not None and width is not None and channel is not None
        bg = np.zeros((height, width, channel), dtype=np.uint8)
    if bg.dtype != np.uint8:
        raise TypeError('bg must be uint8 (the reference binding takes unsigned char, rasterize.pyx:97)')
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    col = np.ascontiguousarray(colors, dtype=np.float32)
    _ensure_topology(m, triangles, v.shape[0])
    vt = torch.from_numpy(v).to(m.device)[None]
    ct = torch.from_numpy(col).to(m.device)[None]
    img = torch.from_numpy(np.ascontiguousarray(bg)).to(m.device)
    with torch.cuda.device(m.device):
        abi.check(m._lib.syn_rasterize(m._h, vt.data_ptr(), ct.data_ptr(), 1, 0, channel, img.data_ptr(), height, width,
                                       int(reverse), m._stream()))
    bg[...] = img.cpu().numpy()
    return bg


class RenderPipeline:
    """Sim3DR/lighting.py:23-71; a texture is multiplied with the light in the lighting kernel and, like :69, in place."""

    def __init__(self, **kwargs):
        conv = lambda o: np.array(o, dtype=np.float32)[None, :] if isinstance(o, (tuple, list)) else o
        self.intensity_ambient = conv(kwargs.get('intensity_ambient', 0.3))
        self.intensity_directional = conv(kwargs.get('intensity_directional', 0.6))
        self.intensity_specular = conv(kwargs.get('intensity_specular', 0.1))
        self.specular_exp = kwargs.get('specular_exp', 5)
        self.color_ambient = conv(kwargs.get('color_ambient', (1, 1, 1)))
        self.color_directional = conv(kwargs.get('color_directional', (1, 1, 1)))
        self.light_pos = conv(kwargs.get('light_pos', (0, 0, 5)))
        self.view_pos = conv(kwargs.get('view_pos', (0, 0, 5)))

    def update_light_pos(self, light_pos):
        self.light_pos = np.array(light_pos, dtype=np.float32)[None, :]

    def light(self, vertices, triangles):
        """The vertex colours of lighting.py:40-64, [nver,3] float32."""
        m = _model()
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        _ensure_topology(m, triangles, v.shape[0])
        _, light = _shade(m, torch.from_numpy(v).to(m.device)[None], planar=False, cfg=_cfg16(self))
        return light[0].cpu().numpy()

    def __call__(self, vertices, triangles, bg, texture=None):
        if texture is None:
            return rasterize(vertices, triangles, self.light(vertices, triangles), bg=bg)
        m = _model()
        if bg.dtype != np.uint8:
            raise TypeError('bg must be uint8 (the reference binding takes unsigned char, rasterize.pyx:97)')
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        _ensure_topology(m, triangles, v.shape[0])
        vt = torch.from_numpy(v).to(m.device)[None]
        tex_t, shared, back = _tex_arg(m, texture, 1, v.shape[0])
        if not shared:
            raise ValueError('texture must be [nver,3]')
        height, width, channel = bg.shape
        img = torch.from_numpy(np.ascontiguousarray(bg)).to(m.device)
        _, _, colors = _shade_textured(m, vt, False, _cfg16(self), tex_t, True)
        with torch.cuda.device(m.device):
            abi.check(m._lib.syn_rasterize(m._h, vt.data_ptr(), colors.data_ptr(), 1, 0, channel, img.data_ptr(), height, width, 0,
                                           m._stream()))
        if back is not None:
            back[...] = tex_t.cpu().numpy()              # `texture *= light` (lighting.py:69): the caller's array holds the product
        bg[...] = img.cpu().numpy()
        return bg


def _draw_and_blend(model, img, meshes, colors, planar, alpha):
    img_t = (img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))).to(model.device)
    H, W, ch = img_t.shape
    F = meshes.shape[0]
    overlap = img_t.clone()
    res = torch.empty_like(img_t)
    with torch.cuda.device(model.device):
        for f0 in range(0, F, 254):                      # the z-key has an 8-bit face field; later faces overwrite earlier ones
            f1 = min(F, f0 + 254)
            abi.check(model._lib.syn_rasterize(model._h, meshes[f0:f1].data_ptr(), colors[f0:f1].data_ptr(), f1 - f0, planar, ch,
                                               overlap.data_ptr(), H, W, 0, model._stream()))
        abi.check(model._lib.syn_add_weighted(model._h, img_t.data_ptr(), C.c_float(1 - alpha), overlap.data_ptr(), C.c_float(alpha),
                                              res.data_ptr(), img_t.numel(), model._stream()))
    return overlap, res


def _render_textured(model, img, meshes, tex, alpha, pipe):
    """The meshes (vertex count = that of the selected topology) drawn with tex * light; tex as _tex_arg takes it."""
    F, _, n = meshes.shape
    tex_t, shared, back = _tex_arg(model, tex, F, n)
    planar = _planar_arg(meshes)
    _, _, colors = _shade_textured(model, meshes, planar, _cfg16(pipe), tex_t, shared)
    out = _draw_and_blend(model, img, meshes, colors, planar, alpha)
    if back is not None and shared:
        back[...] = tex_t.cpu().numpy()                  # the reference leaves the caller's array multiplied (lighting.py:69)
    return out


def render_batch(model, img, meshes, alpha=0.6, cfg=None, uv_tex=None, tex=None):
    """Device-resident utils/render.py:31-50: img uint8 [H,W,3] (tensor or array), meshes [F,3,N] float32 device tensor in
    image coordinates (reconstruct(..., roi=..., dense=True)); the topology is the model's `triangles`.
    Returns (solid overlay, blended result) as uint8 device tensors.

    Textured (the texture demos, uv_texture_realFaces.py:96-116): with `uv_tex` (uint8 UV texture image [H,W,3], or [F,H,W,3]
    for one per face) or `tex` (float32 colours in [0,1] per KEPT vertex, [n_keep,3] shared or [F,n_keep,3]) the full meshes
    are gathered to the model's kept vertex subset, lit, multiplied with the texture and drawn with the kept topology
    (param_pack.keep_ind / tri_deletion) -- gather, lookup, shade, raster and blend on the device.  A shared `tex` is
    multiplied in place face after face like the reference's (lighting.py:69)."""
    pipe = RenderPipeline(**(cfg or RENDER_CFG))
    if uv_tex is not None or tex is not None:
        if uv_tex is not None and tex is not None:
            raise ValueError('give uv_tex or tex, not both')
        kept = gather_kept(model, meshes)
        if uv_tex is not None:
            tex = uv_vertex_colors(model, uv_tex, kept=True, normalize=True)
            if tex.shape[-1] != 3:
                raise ValueError('uv_tex must have 3 channels to be rendered')
        _select(model, 1)
        return _render_textured(model, img, kept, tex, alpha, pipe)
    F, _, n = meshes.shape
    _ensure_model_topology(model, n)
    planar = _planar_arg(meshes)       # the pitched rows reconstruct() writes are read in place: no packed copy on the device path
    with torch.cuda.device(model.device):
        _, light = _shade(model, meshes, planar=planar, cfg=_cfg16(pipe))
    return _draw_and_blend(model, img, meshes, light, planar, alpha)


def render(img, ver_lst, alpha=0.6, wfp=None, tex=None, connectivity=None):
    """utils/render.py:31-50: img uint8 [H,W,3], ver_lst = the mesh list of get_all_outputs ((3,N) arrays).  Returns the
    blended image; `wfp` (file output through cv2.imwrite in the reference) is not supported here.
    tex [N,3] float32 in [0,1]: one colour per vertex of the meshes AS PASSED (the texture demos pass the kept subset and
    connectivity=tri_deletion-1, uv_texture_realFaces.py:115-116); it is multiplied with the light of every face in turn, in
    place, so the caller's array is left mutated like the reference's (lighting.py:69)."""
    if wfp is not None:
        raise NotImplementedError('file output is outside this library (the reference uses cv2.imwrite)')
    m = _model()
    meshes = torch.from_numpy(np.stack([np.asarray(v, dtype=np.float32) for v in ver_lst])).to(m.device)
    saved = m.triangles
    if connectivity is not None:
        tri = np.ascontiguousarray(np.asarray(connectivity).T, dtype=np.int32)
        _ensure_topology(m, tri, meshes.shape[2])
        m.triangles = torch.from_numpy(tri.T.astype(np.int64))
    try:
        if tex is None:
            return render_batch(m, img, meshes, alpha)[1].cpu().numpy()
        t = np.asarray(m.triangles)
        _ensure_topology(m, np.ascontiguousarray(t.T if t.shape[0] == 3 else t), meshes.shape[2])
        return _render_textured(m, img, meshes, tex, alpha, RenderPipeline(**RENDER_CFG))[1].cpu().numpy()
    finally:
        m.triangles = saved
