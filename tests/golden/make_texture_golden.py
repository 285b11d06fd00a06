"""Generate tests/golden/texture_golden.npz (authoring container only: needs the reference checkout and oracle/_ref).

    python tests/golden/make_texture_golden.py

Textured rendering of the reference's texture demos (uv_texture_realFaces.py:96-116 -> utils/render.py:31-50 ->
Sim3DR/lighting.py:37-71) on seeded inputs (tests/texture_cases.py), with oracle.sim3dr.RenderPipeline(impl='ref'): the
reference's own C++ normals and rasteriser under the checker's numpy restatement of its lighting.  Three cases:
  small   3 faces sharing one texture (multiplied in place face after face), kept subset of a 40 x 44 grid, 160 px frame
  perface 3 faces with a texture each, 32 x 30 grid, 96 px frame
  full    53215 vertices before keeping, 450 x 450 frame, 2 faces: configuration and overlay only
and the bytes the reference's own write_obj_with_colors writes (the one function definition is picked out of
uv_texture_realFaces.py where it lies and executed; the script's imports cannot be satisfied here).  Data only.
"""
import ast
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import texture_cases as tc                # noqa: E402
from oracle import ref_loader             # noqa: E402
from oracle import sim3dr as osim         # noqa: E402

#         rows cols n_vert hw  F  mesh img uv tex n_tex smooth
CASES = dict(small=(40, 44, 40 * 44, 160, 3, 940, 40, 31, 51, 1, 1),
             perface=(32, 30, 32 * 30, 96, 3, 932, 32, 33, 53, 3, 1),
             full=(231, 231, 53215, 450, 2, 1131, 231, 35, 55, 1, 2))


def reference_write_obj_with_colors():
    src = open(os.path.join(ref_loader.REF_ROOT, 'uv_texture_realFaces.py')).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == 'write_obj_with_colors']
    ns = {}
    exec(compile(ast.Module(body=fn, type_ignores=[]), 'uv_texture_realFaces.py', 'exec'), ns)
    return ns['write_obj_with_colors']


def obj_inputs(which):
    rng = np.random.default_rng(70 + which)
    nv, nt = (40, 60) if which == 0 else (25, 30)
    vert = (rng.standard_normal((3, nv)) * 60.0 + 60.0).astype(np.float32)
    vert[:, :4] = np.array([[0.00005, -0.00005, 0.12345, -0.0], [0.5, -2.5, 1234.56785, 1e-7], [1e5, 0.99995, -0.99995, 7.0]], dtype=np.float32)
    tri = rng.integers(1, nv + 1, size=(3, nt)).astype(np.int32)
    col = rng.integers(0, 256, (nv, 3)).astype(np.float32)           # what the demo passes: uint8 colours as float32
    if which == 1:
        col = col / np.float32(255.0)                                  # non-integral float32: `{}` prints the shortest repr
    return vert, tri, col


def main():
    osim.build()
    assert osim.ref_available(), 'oracle/_ref not built'
    out = {}
    for name, cfg in CASES.items():
        case = tc.build(cfg)
        tex = tc.demo_tex(case)
        r = tc.oracle_render(case, tex, impl='ref')
        out[name + '_cfg'] = np.array(cfg, dtype=np.int64)
        out[name + '_kept'] = np.array([case['keep'].size, case['tri_kept'].shape[0]], dtype=np.int64)
        out[name + '_overlay'] = r['overlay']
        if name != 'full':
            out[name + '_normal'], out[name + '_light'], out[name + '_colours'] = r['normal'], r['light'], r['colours']
            out[name + '_blend'] = r['blend']
        if tex.ndim == 2 and name != 'full':
            out[name + '_tex_final'] = tex                              # the shared array after the last face
        print(name, 'kept', case['keep'].size, 'of', case['n_vert'], 'triangles', case['tri_kept'].shape[0], 'drawn pixels',
              int((r['overlay'] != case['img']).any(2).sum()))
    write = reference_write_obj_with_colors()
    with tempfile.TemporaryDirectory() as td:
        for which, arg in enumerate(('mesh_col', 'mesh_col2.obj')):
            vert, tri, col = obj_inputs(which)
            write(os.path.join(td, arg), vert, tri, col)
            fn = arg if arg.endswith('.obj') else arg + '.obj'
            out[f'obj{which}_bytes'] = np.frombuffer(open(os.path.join(td, fn), 'rb').read(), dtype=np.uint8)
            out[f'obj{which}_name'], out[f'obj{which}_arg'] = np.array(fn), np.array(arg)
            out[f'obj{which}_vertices'], out[f'obj{which}_triangles'], out[f'obj{which}_colors'] = vert, tri, col
    path = os.path.join(HERE, 'texture_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
