"""GPU parity of the train-time augmentation (syn_train_transform_u8, augment.TrainTransform / train_batches) against what
the reference's own classes produced (tests/golden/augment_golden.npz) and the numpy restatement of tests/augment_cases.py.  The
arithmetic is exact, so every comparison is equality of bits: bytes as bytes, fp32 as uint32.  Every launch runs between 64 guard words
on either side of both outputs."""
import random

import numpy as np
import pytest

import augment_cases as ac
from synergynet_amd import abi

pytestmark = pytest.mark.gpu

SIG = getattr(abi, '_SIGS')['syn_train_transform_u8']                           # KeyError without the feature
GUARD = 256                                                                      # bytes = 64 words


@pytest.fixture(scope='module')
def gold():
    return ac.load_golden()


@pytest.fixture(scope='module')
def model(pack, backbone_sd):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)
    m.load_synergy_state(synth.make_synergy_state(11))
    return m


def _records(g, idx=None):
    from synergynet_amd import augment
    idx = np.arange(len(g['mask'])) if idx is None else np.asarray(idx)
    r = np.zeros(len(idx), dtype=augment.RECORD_DTYPE)
    r['src_index'], r['op'], r['factor'], r['mask'] = g['src_index'][idx], g['op'][idx], g['factor'][idx].astype(np.float32), g['mask'][idx]
    return r


def _launch(m, src, rec, margin, mean, std, f32=True, u8=True, src_off=0, f32_off=0, u8_off=0, N=None, H=None, W=None, B=None, expect=0):
    """syn_train_transform_u8 on host arrays; both outputs between guards, at the byte offsets given -> (f32 [B,3,H,W] | None,
    u8 [B,H,W,3] | None).  expect: the status the call must return; a refused call must leave the 0xA5 fill everywhere."""
    import torch
    n, h, w = src.shape[:3]
    b = len(rec)
    dsrc = torch.zeros(src.size + src_off + 16, dtype=torch.uint8, device='cuda')
    dsrc[src_off:src_off + src.size] = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).cuda()
    drec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy()).cuda()
    nf, nu = b * 3 * h * w * 4, b * h * w * 3
    bf = torch.full((GUARD + f32_off + nf + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    bu = torch.full((GUARD + u8_off + nu + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    rc = m._lib.syn_train_transform_u8(m._h, dsrc.data_ptr() + src_off, n if N is None else N, h if H is None else H, w if W is None else W,
                                       drec.data_ptr(), b if B is None else B, margin, mean, std,
                                       bf.data_ptr() + GUARD + f32_off if f32 else None, bu.data_ptr() + GUARD + u8_off if u8 else None, m._stream())
    assert rc == expect, (rc, m._lib.syn_last_error())
    torch.cuda.synchronize()
    hf, hu = bf.cpu().numpy(), bu.cpu().numpy()
    lo_f, lo_u = GUARD + f32_off, GUARD + u8_off
    assert (hf[:lo_f] == 0xA5).all() and (hf[lo_f + nf:] == 0xA5).all() and (hu[:lo_u] == 0xA5).all() and (hu[lo_u + nu:] == 0xA5).all(), 'guards'
    if rc != 0 or not f32:
        assert (hf == 0xA5).all()
    if rc != 0 or not u8:
        assert (hu == 0xA5).all()
    if rc != 0:
        return None, None
    return (hf[lo_f:lo_f + nf].copy().view(np.float32).reshape(b, 3, h, w) if f32 else None,
            hu[lo_u:lo_u + nu].reshape(b, h, w, 3) if u8 else None)


def _same(got_f32, got_u8, want_f32, want_u8):
    if got_u8 is not None:
        assert np.array_equal(got_u8, want_u8)
    if got_f32 is not None:
        assert np.array_equal(ac.bits(got_f32), ac.bits(want_f32))


@pytest.mark.parametrize('name', [g['name'] for g in ac.build_groups()])
def test_every_recorded_case_bit_for_bit(model, gold, name):
    g = gold[0][name]
    args = (int(g['margin']), float(g['mean']), float(g['std']))
    n = len(g['mask'])
    _same(*_launch(model, g['src'], _records(g), *args), g['f32'], g['u8'])            # the whole group: orders, masks and sources mixed
    for B, kw in ((1, dict(u8=False)), (3, dict(f32=False)), (17, dict())):
        idx = (np.arange(B) * 5 + B) % n
        _same(*_launch(model, g['src'], _records(g, idx), *args, **kw), g['f32'][idx], g['u8'][idx])


@pytest.mark.parametrize('name', ['p120', 'p16x33_m0', 'p7x5_m0'])
def test_f32_is_the_normalised_u8_as_torch_computes_it_on_the_device(model, gold, name):
    import torch
    g = gold[0][name]
    f32, u8 = _launch(model, g['src'], _records(g), int(g['margin']), float(g['mean']), float(g['std']))
    mean, std = torch.tensor(float(g['mean']), device='cuda'), torch.tensor(float(g['std']), device='cuda')     # device tensors: a true division
    want = (torch.from_numpy(u8).cuda().permute(0, 3, 1, 2).float() - mean) / std
    assert np.array_equal(ac.bits(want.cpu().numpy()), ac.bits(f32))


@pytest.mark.parametrize('name', ['p7x5_m0', 'p16x33_m5', 'p120'])
def test_a_face_has_the_same_bits_alone_anywhere_and_repeated(model, gold, name):
    g = gold[0][name]
    args = (int(g['margin']), float(g['mean']), float(g['std']))
    n = len(g['mask'])
    k = 1 % n
    alone = _launch(model, g['src'], _records(g, [k]), *args)
    idx = (np.arange(17) * 3) % n
    idx[[0, 5, 16]] = k                                                                 # first, inside, last -- and three times the same source
    f32, u8 = _launch(model, g['src'], _records(g, idx), *args)
    for pos in (0, 5, 16):
        _same(f32[pos:pos + 1], u8[pos:pos + 1], *alone)
    _same(f32, u8, g['f32'][idx], g['u8'][idx])


@pytest.mark.parametrize('name', ['p1x1', 'p7x5_m0', 'p16x33_m0', 'p120'])
def test_unaligned_buffers(model, gold, name):
    g = gold[0][name]
    args = (int(g['margin']), float(g['mean']), float(g['std']))
    _same(*_launch(model, g['src'], _records(g), *args, src_off=1, u8_off=3, f32_off=4), g['f32'], g['u8'])
    _same(*_launch(model, g['src'], _records(g), *args, src_off=4, u8_off=2, f32_off=12, f32=True, u8=True), g['f32'], g['u8'])
    _same(*_launch(model, g['src'], _records(g), *args, src_off=8, u8_off=1, f32=False), g['f32'], g['u8'])


@pytest.mark.parametrize('name', ['p7x5_m0', 'p120'])
def test_bad_records_give_zero_faces_and_touch_nothing_else(model, gold, name):
    g = gold[0][name]
    args = (int(g['margin']), float(g['mean']), float(g['std']))
    n, N = len(g['mask']), g['src'].shape[0]
    idx = np.arange(9) % n
    rec = _records(g, idx)
    rec['src_index'][1], rec['src_index'][3], rec['op'][5, 1], rec['mask'][7] = -1, N, 9, 8
    bad = [1, 3, 5, 7]
    f32, u8 = _launch(model, g['src'], rec, *args)
    want_u8, want_f32 = g['u8'][idx].copy(), g['f32'][idx].copy()
    want_u8[bad] = 0
    want_f32[bad] = (np.float32(0) - np.float32(g['mean'])) / np.float32(g['std'])
    _same(f32, u8, want_f32, want_u8)
    rec['src_index'][1], rec['src_index'][3] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    rec['op'][5], rec['mask'][7] = 255, 255
    _same(*_launch(model, g['src'], rec, *args), want_f32, want_u8)


def test_every_refusal_leaves_the_outputs_untouched(model, gold):
    import torch
    g = gold[0]['p7x5_m0']
    rec, src = _records(g, [0, 1, 2]), g['src']
    E = abi.SYN_ERR_INVALID
    lib = model._lib
    for kw in (dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(W=-5), dict(B=0), dict(B=-2), dict(f32=False, u8=False)):
        _launch(model, src, rec, 0, 127.5, 128.0, expect=E, **kw)
    for margin, mean, std in ((-1, 127.5, 128.0), (0, 127.5, 0.0), (0, 127.5, -0.0), (0, 127.5, float('inf')), (0, 127.5, float('nan')),
                              (0, float('nan'), 128.0), (0, float('-inf'), 128.0)):
        _launch(model, src, rec, margin, mean, std, expect=E)
    # NULL pointers and overlaps
    d = torch.full((4096,), 7, dtype=torch.uint8, device='cuda')
    r = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    s, p = model._stream(), d.data_ptr()
    call = lambda h, sp, rp, of, ou: lib.syn_train_transform_u8(h, sp, 3, 7, 5, rp, 3, 0, 127.5, 128.0, of, ou, s)
    assert call(None, p, r.data_ptr(), p + 2048, None) == E and b'NULL' in lib.syn_last_error()
    assert call(model._h, None, r.data_ptr(), p + 2048, None) == E
    assert call(model._h, p, None, p + 2048, None) == E
    assert call(model._h, p, r.data_ptr(), None, None) == E and b'both outputs' in lib.syn_last_error()
    face = 3 * 7 * 5 * 3
    assert call(model._h, p, r.data_ptr(), None, p + face - 1) == E and b'overlap' in lib.syn_last_error()      # out_u8 into the set's last byte
    assert call(model._h, p + 2048, r.data_ptr(), p + 2048 - 4 * face + 4, None) == E                           # out_f32 ends inside the set
    assert call(model._h, p, r.data_ptr(), p + 1024, p + 1024 + 4 * face - 1) == E                              # the outputs into each other
    assert call(model._h, p, r.data_ptr(), None, p) == E                                                        # in place is not allowed
    torch.cuda.synchronize()
    assert (d == 7).all()
    assert call(model._h, p, r.data_ptr(), p + 1024, p + 1024 + 4 * face) == 0                                  # back to back is fine
    torch.cuda.synchronize()


def test_largest_accepted_face_and_the_first_refused(model):
    from synergynet_amd import augment
    limit = abi.SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES
    W = limit // 3
    assert 3 * W == limit                                                               # 1 x 54592: every byte of the limit
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (2, 1, W, 3), dtype=np.uint8)
    rec = np.zeros(3, dtype=augment.RECORD_DTYPE)
    rec['src_index'] = [1, 0, 1]
    rec['op'] = [ac.ORDERS[1], ac.ORDERS[4], (ac.CONTRAST, ac.SKIP, ac.SATURATION)]
    rec['factor'] = [(0.6, 1.2, 0.8), (1.4, 0.8, 3.0), (0.0, 1.0, 1.7)]
    rec['mask'] = [0, 6, 5]
    want = [ac.train_transform(src[rec['src_index'][i]], rec['op'][i], rec['factor'][i], int(rec['mask'][i]), 0, 127.5, 128.0) for i in range(3)]
    _same(*_launch(model, src, rec, 0, 127.5, 128.0), np.stack([w[1] for w in want]), np.stack([w[0] for w in want]))
    # a tall one just below the limit: 233 x 234 x 3 = 163566
    src = rng.integers(0, 256, (1, 233, 234, 3), dtype=np.uint8)
    want = ac.train_transform(src[0], rec['op'][0], rec['factor'][0], 7, 5, 127.5, 128.0)
    r1 = rec[:1].copy()
    r1['src_index'], r1['mask'] = 0, 7
    _same(*_launch(model, src, r1, 5, 127.5, 128.0), want[1][None], want[0][None])
    # one pixel more is refused; so is a size whose byte count overflows 32 bits
    small = np.zeros((1, 1, 4, 3), dtype=np.uint8)
    _launch(model, small, rec[:1], 0, 127.5, 128.0, W=W + 1, expect=abi.SYN_ERR_INVALID)
    assert b'LDS' in model._lib.syn_last_error()
    _launch(model, small, rec[:1], 0, 127.5, 128.0, H=1 << 16, W=1 << 16, expect=abi.SYN_ERR_INVALID)
    with pytest.raises(ValueError, match='does not fit'):
        import torch
        augment.TrainTransform(model)(torch.zeros((1, 1, W + 1, 3), dtype=torch.uint8))


def test_train_transform_end_to_end(model, gold):
    import torch
    from synergynet_amd import augment
    g = gold[0]['p120']
    crops = torch.from_numpy(g['src']).cuda()
    t = augment.TrainTransform(model, margin=int(g['margin']), mean=float(g['mean']), std=float(g['std']))
    rec = _records(g)
    f32, u8 = t(crops, records=rec, out='both')
    assert f32.is_cuda and f32.dtype == torch.float32 and tuple(f32.shape) == (5, 3, 120, 120)
    assert u8.is_cuda and u8.dtype == torch.uint8 and tuple(u8.shape) == (5, 120, 120, 3)
    _same(f32.cpu().numpy(), u8.cpu().numpy(), g['f32'], g['u8'])
    assert torch.equal(t(crops, records=rec), f32) and torch.equal(t(crops, records=rec, out='u8'), u8)
    # index overrides the records' sources; host arrays are accepted
    idx = [1, 1, 0, 0, 1]
    got = t(g['src'], index=idx, records=rec, out='u8').cpu().numpy()
    for i in range(5):
        want, _ = ac.train_transform(g['src'][idx[i]], g['op'][i], g['factor'][i], int(g['mask'][i]), int(g['margin']), 127.5, 128.0)
        assert np.array_equal(got[i], want)
    # fresh draws follow the generators handed in: the same seeds, the same batch -- and it is what draw_records + the restatement give
    t1 = augment.TrainTransform(model, prob=0.5, np_random=np.random.RandomState(4), py_random=random.Random(4))
    t2 = augment.TrainTransform(model, prob=0.5, np_random=np.random.RandomState(4), py_random=random.Random(4))
    a, b = t1(crops, index=[0, 1, 1, 0]), t2(crops, index=[0, 1, 1, 0])
    assert torch.equal(a, b) and tuple(a.shape) == (4, 3, 120, 120)
    rec = augment.draw_records(4, prob=0.5, np_random=np.random.RandomState(4), py_random=random.Random(4))
    for i, k in enumerate([0, 1, 1, 0]):
        _, want = ac.train_transform(g['src'][k], rec['op'][i], rec['factor'][i], int(rec['mask'][i]), 5, 127.5, 128.0)
        assert np.array_equal(ac.bits(a[i].cpu().numpy()), ac.bits(want))
    assert t(crops).shape[0] == 2                                                       # no index: the whole set in order
    # the host-side validation names what is wrong
    bad = _records(g)
    bad['op'][2, 0] = 4
    with pytest.raises(ValueError, match='op'):
        t(crops, records=bad)
    with pytest.raises(ValueError, match=r'index must lie in \[0, 2\)'):
        t(crops, index=[0, 2])
    with pytest.raises(ValueError, match='out must be'):
        t(crops, out='f16')
    with pytest.raises(ValueError, match='uint8 crops'):
        t(crops.float())


def test_train_batches_order_drop_last_and_target_slice(model):
    import torch
    from synergynet_amd import augment, synth
    N, bs = 11, 4
    crops = torch.from_numpy(synth.make_crops(N, seed=5)).cuda()
    targets = torch.arange(N * 70, dtype=torch.float64).reshape(N, 70)                  # wider than 62, another dtype, on the host
    t = augment.TrainTransform(model, brightness=0, contrast=0, saturation=0, prob=0.0)  # nothing to draw: the batch is a function of the order
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(8))
    plain = t(crops)
    for drop_last, n_batches in ((True, 2), (False, 3)):
        got = list(augment.train_batches(model, crops, targets, bs, t, generator=torch.Generator().manual_seed(8), drop_last=drop_last))
        assert len(got) == n_batches
        for k, (x, y) in enumerate(got):
            idx = perm[k * bs:(k + 1) * bs]
            assert x.is_cuda and y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (len(idx), 62)
            assert torch.equal(y.cpu(), targets[idx][:, :62].float())
            assert torch.equal(x, plain[idx.cuda()])
    u = next(iter(augment.train_batches(model, crops, targets, bs, t, generator=torch.Generator().manual_seed(8), out='u8')))[0]
    assert u.dtype == torch.uint8 and tuple(u.shape) == (bs, 120, 120, 3)
    want = crops[perm[:bs].cuda()].clone()
    want[:, :5], want[:, -5:], want[:, :, :5], want[:, :, -5:] = 0, 0, 0, 0
    assert torch.equal(u, want)
    with pytest.raises(ValueError, match='targets must be'):
        next(iter(augment.train_batches(model, crops, targets[:, :61], bs, t)))


def test_u8_batch_through_the_train_mode_head(model):
    import torch
    from synergynet_amd import augment, synth
    crops = torch.from_numpy(synth.make_crops(6, seed=6)).cuda()
    target = torch.from_numpy(synth.make_params(6, 3)).cuda()
    t = augment.TrainTransform(model, prob=0.5, np_random=np.random.RandomState(2), py_random=random.Random(2))
    u8 = t(crops, index=[5, 0, 3, 3, 1, 2], out='u8')
    assert not torch.equal(u8, crops[[5, 0, 3, 3, 1, 2]])
    got = model.losses_crops_u8(u8, target, bn='batch', momentum=None)
    by_hand = torch.from_numpy(u8.cpu().numpy().copy()).cuda()
    want = model.losses_crops_u8(by_hand, target, bn='batch', momentum=None)
    running = model.losses_crops_u8(by_hand, target)
    assert set(got) == set(want) == set(running)
    for k in got:
        assert torch.equal(got[k], want[k]), k
    assert any(not torch.equal(got[k], running[k]) for k in got)                        # the keyword selects another head
    with pytest.raises(RuntimeError, match='bn must be'):
        model.losses_crops_u8(u8, target, bn='train')
