"""Generate tests/golden/visibility_golden.npz (authoring container only: needs oracle/_ref, built from the reference checkout).

    python tests/golden/make_visibility_golden.py

The three buffers of Sim3DR.rasterize_triangles (Sim3DR/lib/rasterize_kernel.cpp:290-348) come from the reference's own compiled
function (tests/visibility_cases.ref_rasterize_triangles) on seeded inputs (tests/visibility_cases.py); what is defined on top of
them (vertex visibility, colours sampled from the frame, UV texture and mask) from the numpy lines of the same module.  Cases:
  soup   64 x 64, 400 triangles: zero-area, duplicate, equal-depth, +0 / -0 depth, NaN corner, off-frame and box-edge triangles,
         NON-DEFAULT initial buffers (depth 0.5, triangle -7, weight 0.25 over the right half); full buffers
  small  40 x 44 grid at 160 px, two faces (frontal, turned 60 degrees about the vertical axis): full buffers, visibility, sampled
         colours, UV texture and mask
  full   53215 vertices at 450 px, the same two poses: visibility as packed bits, counts and the sha256 of every buffer
Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import visibility_cases as vc             # noqa: E402

#            rows cols n_vert hw  mesh img uv
CASES = dict(small=(40, 44, 40 * 44, 160, 940, 41, 31),
             full=(231, 231, 53215, 450, 940, 232, 35))


def reference_buffers(case):
    hw = case['hw']
    depth, tri, bary = vc.fresh_buffers(hw, hw, lead=(case['n_faces'],))
    for f in range(case['n_faces']):
        vc.ref_rasterize_triangles(np.ascontiguousarray(case['meshes'][f].T), case['tri_full'], depth[f], tri[f], bary[f], hw, hw)
    return depth, tri, bary


def main():
    assert vc.ref_available(), 'oracle/_ref not built'
    out = {}
    ver, tri, (depth, tb, bw) = vc.build_soup()
    init_tb = tb.copy()
    vc.ref_rasterize_triangles(ver, tri, depth, tb, bw, vc.SOUP_HW, vc.SOUP_HW)
    out['soup_cfg'] = np.array([vc.SOUP_SEED, vc.SOUP_HW, tri.shape[0]], dtype=np.int64)
    out['soup_depth'], out['soup_tri'], out['soup_bary'] = depth, tb, bw
    print('soup: winning pixels', int((tb != init_tb).sum()), 'distinct winners', np.unique(tb[tb >= 0]).size,
          'signed zeros', int(((depth == 0) & np.signbit(depth)).sum()), int(((depth == 0) & ~np.signbit(depth) & (tb >= 0)).sum()))
    for name, cfg in CASES.items():
        case = vc.build_mesh_case(cfg)
        buf = reference_buffers(case)
        r = vc.mesh_pipeline(case, buf)
        out[name + '_cfg'] = np.array(cfg, dtype=np.int64)
        out[name + '_visible_count'] = r['visible'].sum(1).astype(np.int64)
        out[name + '_pixel_count'] = (buf[1] >= 0).reshape(2, -1).sum(1).astype(np.int64)
        out[name + '_texel_count'] = (r['mask'] != 0).reshape(2, -1).sum(1).astype(np.int64)
        full = dict(depth=buf[0], tri=buf[1], bary=buf[2], **r)
        if name == 'small':
            for k, v in full.items():
                out[f'{name}_{k}'] = v.astype(np.uint8) if v.dtype == bool else v
        else:
            out[name + '_visible_bits'] = np.packbits(r['visible'], axis=1)
            for k, v in full.items():
                out[f'{name}_{k}_sha256'] = vc.sha(v.astype(np.uint8) if v.dtype == bool else v)
        print(name, 'visible share', r['visible'].mean(1), 'pixels', out[name + '_pixel_count'], 'texels', out[name + '_texel_count'])
    path = os.path.join(HERE, 'visibility_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
