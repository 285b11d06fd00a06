"""Generate tests/golden/render_texture_golden.npz (authoring container only: needs oracle/_ref, built from the reference checkout).

    python tests/golden/make_render_texture_golden.py

Every image and depth buffer comes from the reference's own compiled `_render_texture_core` (Sim3DR/lib/rasterize_kernel.cpp:353-458,
tests/render_texture_cases.ref_render_texture) on seeded inputs (tests/render_texture_cases.py).  Cases:
  soup   visibility_cases.build_soup() on 64 x 64: initial depth 0.5 over the right half, image pre-filled with -5, a 16 x 20 x 4 float
         texture, texture coordinates reaching outside it on every side (a third of them integers), tex_triangles a seeded permutation;
         c = 3 and 1, nearest and bilinear; full arrays
  small  40 x 44 grid at 160 px, frontal and turned 60 degrees, texture coordinates of the UV asset at 64^2 and 256^2: every face in
         its own planes, and both in ONE z-buffer (the second shifted a few pixels and 0.5 deeper), in both orders; full arrays
  full   53215 vertices at 450 px (and on a 64 x 64 frame): sha256 of image and depth
Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import render_texture_cases as rc         # noqa: E402
import visibility_cases as vc             # noqa: E402
from make_visibility_golden import CASES  # noqa: E402


def main():
    assert vc.ref_available(), 'oracle/_ref not built'
    out = {}
    soup = rc.build_soup_case()
    hw = soup['hw']
    out['soup_cfg'] = np.array([vc.SOUP_SEED, hw, soup['triangles'].shape[0], rc.SOUP_TEX_SEED], dtype=np.int64)
    for c, mt in rc.SOUP_VARIANTS:
        image, depth = rc.soup_image(soup, c), soup['depth'].copy()
        rc.ref_render_texture(image, soup['vertices'], soup['triangles'], soup['texture'], soup['tex_coords'], soup['tex_triangles'], depth,
                              hw, hw, c, mt)
        out[f'soup_image_c{c}_m{mt}'] = image
        assert 'soup_depth' not in out or out['soup_depth'].tobytes() == depth.tobytes()
        out['soup_depth'] = depth
    won = out['soup_depth'].view(np.uint32) != soup['depth'].view(np.uint32)
    d, t, b = vc.build_soup()[2]
    vc.ref_rasterize_triangles(soup['vertices'], soup['triangles'], d, t, b, hw, hw)       # the same walk WITHOUT the border rule
    inside = d.view(np.uint32) == depth.view(np.uint32)                                     # the overall winner contains the pixel
    x, y = soup['tex_coords'][:, 0], soup['tex_coords'][:, 1]
    print('soup: won pixels', int(won.sum()), 'of them only through the border rule', int((won & ~inside).sum()),
          'signed zeros -0 / +0', int(((depth == 0) & np.signbit(depth) & won).sum()), int(((depth == 0) & ~np.signbit(depth) & won).sum()),
          'coordinates outside (left, right, top, bottom)', int((x < 0).sum()), int((x > 19).sum()), int((y < 0).sum()), int((y > 15).sum()))
    case = vc.build_mesh_case(CASES['small'])
    out['small_cfg'] = np.array(CASES['small'], dtype=np.int64)
    hw = case['hw']
    for name, (meshes, tex, coords, c, mt, shared) in rc.small_variants(case).items():
        image, depth = (rc.ref_shared if shared else rc.ref_per_face)(meshes, case['tri_full'], tex, coords, hw, hw, c, mt)
        out[f'small_{name}_image'], out[f'small_{name}_depth'] = image, depth
        print('small', name, 'pixels drawn', int((depth != rc.INIT_DEPTH).sum()))
    a, b = out['small_shared256_image'], out['small_shared256_swapped_image']
    print('small shared: elements that depend on the order of the faces', int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    case = vc.build_mesh_case(CASES['full'])
    out['full_cfg'] = np.array(CASES['full'], dtype=np.int64)
    tex = rc.byte_texture(rc.SMALL_TEX_SEED + 2, rc.FULL_TEX_HW, rc.FULL_TEX_HW).astype(np.float32)
    coords = rc.uv_coords(case['assets'], rc.FULL_TEX_HW, rc.FULL_TEX_HW)
    for tag, frame in (('', case['hw']), ('64', rc.FULL_SMALL_FRAME)):
        image, depth = rc.ref_per_face(rc.scaled(case['meshes'], case['hw'], frame), case['tri_full'], tex, coords, frame, frame, 3, rc.BILINEAR)
        out[f'full_image{tag}_sha256'], out[f'full_depth{tag}_sha256'] = vc.sha(image), vc.sha(depth)
        out[f'full_pixel_count{tag}'] = (depth != rc.INIT_DEPTH).reshape(2, -1).sum(1).astype(np.int64)
        print('full', frame, 'pixels drawn', out[f'full_pixel_count{tag}'])
    path = os.path.join(HERE, 'render_texture_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
