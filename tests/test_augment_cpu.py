"""Train-time augmentation without a GPU: the numpy restatement of tests/augment_cases.py against what the reference's own classes
produced (tests/golden/augment_golden.npz) bit for bit, the bite of the fixture -- each wrong port misses a recorded case, and by how
many bytes is printed --, draw_records against the reference's logged draws, the new symbol in header / ctypes table / library, the
refusals that touch no device, and the Python surface."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest

import augment_cases as ac
from conftest import ROOT


@pytest.fixture(scope='module')
def gold():
    return ac.load_golden()


def test_fixture_is_data_and_holds_the_case_table(gold):
    groups, draws, z = gold
    assert all(v.dtype.kind in 'iufU' for v in z.values())
    assert os.path.getsize(ac.GOLDEN) < 1 << 20
    built = ac.build_groups()
    assert [g['name'] for g in built] == list(groups)
    for g in built:
        r = groups[g['name']]
        for k in ('src', 'src_index', 'op', 'factor', 'mask'):
            assert np.array_equal(g[k], r[k]), (g['name'], k)
        assert (int(r['margin']), float(r['mean']), float(r['std'])) == (g['margin'], g['mean'], g['std'])
    ops = np.concatenate([g['op'] for g in built])
    assert {tuple(o) for o in ops} >= set(ac.ORDERS)                                   # all six orders
    assert set(np.concatenate([g['mask'] for g in built]).tolist()) == set(range(8))    # all eight mask kinds
    fac = np.concatenate([g['factor'].ravel() for g in built])
    assert set(ac.SPECIAL_FACTORS) <= set(fac.tolist())
    shapes = {g['src'].shape[1:3] for g in built}
    assert shapes >= {(1, 1), (3, 2), (7, 5), (16, 33), (4, 4), (120, 120)}


@pytest.mark.parametrize('name', [g['name'] for g in ac.build_groups()])
def test_restatement_matches_the_recording_bit_for_bit(gold, name):
    g = gold[0][name]
    u8, f32 = ac.group_expected(g)
    assert u8.dtype == g['u8'].dtype == np.uint8 and np.array_equal(u8, g['u8'])
    assert g['f32'].dtype == np.float32 and np.array_equal(ac.bits(f32), ac.bits(g['f32']))
    if 2 * int(g['margin']) >= min(g['src'].shape[1:3]):
        assert not g['u8'].any()                                                        # what the reference's slices give: all zeros
        assert np.array_equal(ac.bits(g['f32']), ac.bits(np.full_like(g['f32'], (np.float32(0) - g['mean']) / g['std'])))


def test_special_images(gold):
    g = gold[0]['p4x4_special']
    assert (g['u8'][0] == 255).all()                                                    # all 255 under brightness 1.4 stays 255
    # grey mean exactly 90.5 -> 91, one grey level less -> 90: contrast 0.0 leaves the mean itself
    assert (g['u8'][6] == 91).all() and (g['u8'][7] == 90).all()
    h = gold[0]['p1x2_half']
    assert (h['u8'][0] == 11).all() and (h['u8'][2] == 10).all() and (h['u8'][4] == 255).all()


# ---- the fixture bites: each wrong port misses the recording ----
def _misses(gold, what, names, **wrong):
    total = 0
    for name in names:
        g = gold[0][name]
        u8, _ = ac.group_expected(g, **wrong)
        total += int((u8 != g['u8']).sum())
    print(f'{what}: {total} recorded bytes differ')
    assert total > 0, what


def test_bite_single_rounding_blend(gold):
    _misses(gold, 'fused multiply-add', ['p120'], fused=True)
    g = gold[0]['p120']
    assert set(np.float32([0.6, 0.8, 1.2]).tolist()) <= set(g['factor'][0].astype(np.float32).tolist())
    one = {k: (v[:1] if k in ('src_index', 'op', 'factor', 'mask', 'u8', 'f32') else v) for k, v in g.items()}
    assert (ac.group_expected(one, fused=True)[0] != one['u8']).any()                   # the case at exactly 0.6 / 0.8 / 1.2


def test_bite_grey_from_swapped_channels(gold):
    _misses(gold, 'grey with channels 0 and 2 swapped', ['p7x5_m0', 'p120'], swapped=True)


def test_bite_kind_4_as_a_true_lower_right_quadrant(gold):
    _misses(gold, 'rdown as the lower right quadrant', ['p7x5_m0'], box_wrong=dict(true_rdown=True))


def test_bite_kind_7_ending_at_h_minus_h_floor_4(gold):
    assert gold[0]['p7x5_m0']['src'].shape[1] == 7
    _misses(gold, 'center box ending at H - H//4', ['p7x5_m0'], box_wrong=dict(center_floor=True))


def test_bite_contrast_mean_before_an_earlier_step(gold):
    _misses(gold, 'contrast mean of the image as it arrived', ['p7x5_m0', 'p120'], stale_mean=True)


def test_bite_mean_rounded_down(gold):
    _misses(gold, 'contrast mean rounded down', ['p4x4_special', 'p1x2_half'], round_down=True)


# ---- the draws ----
def test_draw_records_reproduces_the_reference_draws(gold):
    from synergynet_amd import augment
    d = gold[1]
    rs, pr = np.random.RandomState(int(d['seed'])), random.Random(int(d['seed']))
    rec = augment.draw_records(ac.DRAW_COUNT, 0.4, 0.4, 0.4, prob=float(d['prob']), np_random=rs, py_random=pr)
    assert rec.dtype == augment.RECORD_DTYPE and rec.dtype.itemsize == 20
    assert np.array_equal(rec['op'], d['op']) and np.array_equal(rec['mask'], d['mask'])
    assert np.array_equal(rec['factor'], d['factor'].astype(np.float32))
    assert np.array_equal(rec['src_index'], np.arange(ac.DRAW_COUNT))
    assert (d['mask'] != 0).sum() > 16 and len({tuple(o) for o in d['op']}) == 6
    # the global generators, seeded as the reference's loop was
    np.random.seed(int(d['seed']))
    random.seed(int(d['seed']))
    rec2 = augment.draw_records(ac.DRAW_COUNT, prob=float(d['prob']))
    assert rec2.tobytes() == rec.tobytes()
    # and the restatement on those records gives what the reference's whole Compose_GT gave
    for i in range(ac.DRAW_COUNT):
        _, f32 = ac.train_transform(d['src'][i % 3], rec['op'][i], rec['factor'][i], int(rec['mask'][i]), int(d['margin']), 127.5, 128)
        assert np.array_equal(ac.bits(f32), ac.bits(d['f32'][i])), i


def test_draw_records_with_a_step_switched_off():
    from synergynet_amd import augment
    rs = np.random.RandomState(3)
    rec = augment.draw_records(5, brightness=0.4, contrast=0, saturation=2.0, prob=0.0, np_random=rs, py_random=random.Random(3))
    assert (np.sort(rec['op'], axis=1) == [0, 1, 3]).all() and (rec['op'][:, 2] == 0).all() and (rec['mask'] == 0).all()
    sat = rec['factor'][rec['op'] == 3]
    assert (sat >= 0).all() and (sat <= 3).all()                                         # max(0, 1 - 2.0) .. 1 + 2.0


def test_check_records_names_the_bad_field():
    from synergynet_amd import augment
    good = augment.draw_records(4, np_random=np.random.RandomState(0), py_random=random.Random(0))
    augment.check_records(good, 4)
    for field, value, word in (('op', 4, 'op'), ('mask', 8, 'mask'), ('factor', np.nan, 'finite'), ('factor', np.inf, 'finite'),
                               ('src_index', -1, 'src_index'), ('src_index', 4, 'src_index')):
        bad = good.copy()
        if bad[field].ndim == 2:
            bad[field][1, 1] = value
        else:
            bad[field][1] = value
        with pytest.raises(ValueError, match=word):
            augment.check_records(bad, 4)


# ---- ABI ----
def test_new_symbol_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import SOURCES, build_library
    assert 'augment_kernels.hip' in SOURCES
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    s = 'syn_train_transform_u8'
    assert s in abi.EXPORTED_SYMBOLS and hasattr(l, s)
    decl = re.search(r'\bint ' + s + r'\(([^;]*)\);', hdr)
    assert decl
    args = re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S)
    assert len(args.split(',')) == len(abi._SIGS[s][1]) == 13
    limit = re.search(r'#define SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES (\d+)', hdr)
    assert limit and int(limit.group(1)) == abi.SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES == 160 * 1024 - 64


def test_refusals_that_touch_no_device():
    from synergynet_amd import abi
    lib = abi.lib()
    buf = np.full(64, 7.0, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.syn_train_transform_u8(None, p, 1, 1, 1, p, 1, 0, 127.5, 128.0, p, None, None) == abi.SYN_ERR_INVALID
    assert b'syn_train_transform_u8' in lib.syn_last_error() and b'NULL' in lib.syn_last_error()
    assert (buf == 7.0).all()


def test_python_surface():
    from synergynet_amd import augment
    from synergynet_amd.synergy3DMM import SynergyNet
    for f in ('draw_records', 'TrainTransform', 'train_batches', 'check_records'):
        assert callable(getattr(augment, f)), f
    with pytest.raises(NotImplementedError, match='hue'):
        augment.TrainTransform(None, 0.4, 0.4, 0.4, hue=0.1)
    t = augment.TrainTransform(None, 0.4, 0.4, 0.4)
    assert (t.margin, t.prob, t.mean, t.std) == (5, 0.01, 127.5, 128.0)
    for bad in (dict(std=0), dict(std=float('inf')), dict(mean=float('nan')), dict(margin=-1), dict(brightness=-0.1)):
        with pytest.raises(ValueError):
            augment.TrainTransform(None, **bad)
    sig = inspect.signature(SynergyNet.losses_crops_u8)
    assert sig.parameters['bn'].default == 'running' and sig.parameters['momentum'].default == 0.1       # today's path by default
    assert list(sig.parameters)[:4] == ['self', 'crops', 'target', 'meter']
