"""Generate tests/golden/augment_golden.npz (authoring container only: needs the reference checkout and PIL).

    python tests/golden/make_augment_golden.py

Everything recorded here is computed by the REAL reference, imported from where it lies (oracle/ref_loader.py): utils.ddfa's
adjust_brightness / adjust_contrast / adjust_saturation (PIL's ImageEnhance) composed with its own Lambda / Compose as ColorJitter composes
them, ToTensor, CenterCrop in its train form and Normalize, on the cases of tests/augment_cases.py:
  * per group `name` (one shape, margin and normalisation):  name.src [N,H,W,3], name.src_index / op / factor / mask per case, name.margin,
    name.mean, name.std, and the reference's results name.u8 [B,H,W,3] (after CenterCrop) and name.f32 [B,3,H,W] (after Normalize).
    A forced order is a Compose of the reference's steps in that order; a forced mask kind is CenterCrop with its module's `random`
    answering that kind.
  * draws.*: the reference's whole Compose_GT on DRAW_COUNT consecutive samples, numpy's and python's generators seeded alike, with its
    adjust_* functions and CenterCrop's mask methods wrapped so that what it DREW is logged: draws.op / factor / mask, the sources and
    the results.
Data only.  The generator asserts what the tests rely on: the restatement equals every recording, and a single-rounding blend does not.
"""
import os
import random
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import augment_cases as ac                      # noqa: E402
from make_loss_golden import ref_module         # noqa: E402

OP_NAMES = {ac.BRIGHTNESS: 'adjust_brightness', ac.CONTRAST: 'adjust_contrast', ac.SATURATION: 'adjust_saturation'}


class _Forced:
    """stands in for the `random` module inside utils.ddfa while one CenterCrop runs: the draw is below any prob > 0.5, the kind is given"""
    def __init__(self, kind):
        self.kind = kind

    def random(self):
        return 0.5

    def randint(self, a, b):
        assert (a, b) == (1, 7)
        return self.kind


def run_case(ddfa, img, ops, factors, mask, margin, mean, std):
    steps = [ddfa.Lambda(lambda im, fn=getattr(ddfa, OP_NAMES[int(op)]), f=float(f): fn(im, f)) for op, f in zip(ops, factors) if op != ac.SKIP]
    arr = np.array(ddfa.Compose(steps)(Image.fromarray(img)))
    keep, ddfa.random = ddfa.random, _Forced(int(mask))
    try:
        out = ddfa.CenterCrop(margin, prob=1.0 if mask else 0.0)(ddfa.ToTensor()(arr))
    finally:
        ddfa.random = keep
    u8 = np.ascontiguousarray(out.numpy().transpose(1, 2, 0)).astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), out.numpy().transpose(1, 2, 0))
    f32 = ddfa.Normalize(mean=mean, std=std)(out).numpy().copy()
    return u8, f32


def record_draws(ddfa, out):
    srcs = [ac.image(7, 5, 501), ac.image(7, 5, 502, coarse=True), ac.image(7, 5, 503)]
    log = []
    keep = {n: getattr(ddfa, n) for n in OP_NAMES.values()}

    def wrap(op, fn):
        def f(img, factor):
            log[-1]['op'].append(op)
            log[-1]['factor'].append(factor)
            return fn(img, factor)
        return f
    for op, n in OP_NAMES.items():
        setattr(ddfa, n, wrap(op, keep[n]))
    crop = ddfa.CenterCrop(1, prob=ac.DRAW_PROB)
    for kind, fn in list(crop.switcher.items()):
        crop.switcher[kind] = (lambda img, h, w, kind=kind, fn=fn: (log[-1].__setitem__('mask', kind), fn(img, h, w))[1])
    chain = ddfa.Compose_GT([ddfa.ColorJitter(0.4, 0.4, 0.4), ddfa.ToTensor(), crop, ddfa.Normalize(mean=127.5, std=128)])
    np.random.seed(ac.DRAW_SEED)
    random.seed(ac.DRAW_SEED)
    res = []
    try:
        for i in range(ac.DRAW_COUNT):
            log.append(dict(op=[], factor=[], mask=0))
            got, _ = chain(srcs[i % 3].copy(), None)
            res.append(got.numpy().copy())
    finally:
        for n, fn in keep.items():
            setattr(ddfa, n, fn)
    assert all(len(e['op']) == 3 for e in log)
    out.update({'draws.src': np.stack(srcs), 'draws.op': np.array([e['op'] for e in log], dtype=np.uint8),
                'draws.factor': np.array([e['factor'] for e in log], dtype=np.float64), 'draws.mask': np.array([e['mask'] for e in log], dtype=np.uint8),
                'draws.f32': np.stack(res), 'draws.seed': np.array(ac.DRAW_SEED), 'draws.prob': np.array(ac.DRAW_PROB), 'draws.margin': np.array(1)})
    print('draws: orders', len({tuple(e['op']) for e in log}), 'mask kinds', sorted({e['mask'] for e in log}))
    assert len({tuple(e['op']) for e in log}) == 6 and len({e['mask'] for e in log}) >= 5
    # the restatement on the logged draws
    for i, e in enumerate(log):
        _, f32 = ac.train_transform(srcs[i % 3], e['op'], e['factor'], e['mask'], 1, 127.5, 128)
        assert np.array_equal(ac.bits(f32), ac.bits(res[i])), i


def main():
    torch.set_num_threads(4)
    import PIL
    ddfa = ref_module('utils.ddfa')
    out = {'pil_version': np.array(PIL.__version__), 'torch_version': np.array(torch.__version__)}
    names, fused_differs = [], {}
    for g in ac.build_groups():
        name, B = g['name'], len(g['mask'])
        names.append(name)
        u8, f32 = [], []
        for i in range(B):
            a, b = run_case(ddfa, g['src'][g['src_index'][i]], g['op'][i], g['factor'][i], g['mask'][i], int(g['margin']), g['mean'], g['std'])
            u8.append(a)
            f32.append(b)
        u8, f32 = np.stack(u8), np.stack(f32)
        want_u8, want_f32 = ac.group_expected(g)
        assert np.array_equal(want_u8, u8), name
        assert np.array_equal(ac.bits(want_f32), ac.bits(f32)), name
        fused_u8, _ = ac.group_expected(g, fused=True)
        fused_differs[name] = int((fused_u8 != u8).sum())
        print(f'{name}: {B} cases, non-zero bytes {int((u8 != 0).sum())} of {u8.size}, a single-rounding blend differs in {fused_differs[name]} bytes')
        for k in ('src', 'src_index', 'op', 'factor', 'mask'):
            out[f'{name}.{k}'] = g[k]
        out[f'{name}.margin'], out[f'{name}.mean'], out[f'{name}.std'] = np.array(g['margin']), np.float32(g['mean']), np.float32(g['std'])
        out[f'{name}.u8'], out[f'{name}.f32'] = u8, f32
    out['groups'] = np.array(names)
    # what the tests rely on: a case at a factor of 0.6 / 0.8 / 1.2 where one rounding instead of two changes recorded bytes
    assert fused_differs['p120'] > 0 and fused_differs['p7x5_m0'] > 0, fused_differs
    record_draws(ddfa, out)
    path = os.path.join(HERE, 'augment_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 900 << 10


if __name__ == '__main__':
    main()
