"""Generate tests/golden/mesh_edges_golden.npz (authoring container only: needs oracle/_ref, built from the reference checkout).

    python tests/golden/make_mesh_edges_golden.py

What the reference's own code gives on the inputs of tests/mesh_edge_cases.py:
  images   its compiled C++ rasteriser (oracle.sim3dr with impl='ref'), several faces drawn one call after the other;
  normals  its compiled get_normal;
  lights   its Sim3DR/lighting.py, imported by tests/golden/make_golden.load_reference_sim3dr, the vertex colours caught by a probe
           in place of its rasterize call (update_light_pos where the case moves the light).
Expected outputs only: the inputs are rebuilt from the seeds of the case module.  Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))
sys.path.insert(0, HERE)

import mesh_edge_cases as mc              # noqa: E402
from make_golden import load_reference_sim3dr   # noqa: E402
from oracle import sim3dr as osim         # noqa: E402


def main():
    ref = load_reference_sim3dr()
    assert osim.ref_available(), 'oracle/_ref not built'
    lighting = sys.modules['Sim3DR.lighting']

    def reference_light(name, cfg, moved, ver, tri):
        app = ref.RenderPipeline(**cfg)
        if moved is not None:
            app.update_light_pos(moved)
        caught = []
        real = lighting.rasterize
        lighting.rasterize = lambda v, t, c, bg=None, **kw: (caught.append(c.copy()), bg)[1]
        try:
            app(ver.copy(), tri, np.zeros((mc.HW, mc.HW, 3), np.uint8))
        finally:
            lighting.rasterize = real
        return caught[0]

    out = dict(mc.expected_images(osim, impl='ref'))
    out.update(mc.expected_lights(osim, impl='ref', light_fn=reference_light))
    oracle_img, oracle_lit = mc.expected_images(osim), mc.expected_lights(osim)
    for k, v in out.items():
        if v.dtype == np.uint8 or 'normal' in k:
            assert np.array_equal(v, oracle_img[k] if k in oracle_img else oracle_lit[k], equal_nan=True), k
        else:
            d = np.abs(v - oracle_lit[k])
            print(k, 'reference vs oracle: max', np.nanmax(d), 'NaN', int(np.isnan(v).sum()))
    for k, v in mc.check_nonvacuity(osim, oracle_img, oracle_lit).items():
        print(f'{k}: {v}')
    path = os.path.join(HERE, 'mesh_edges_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
