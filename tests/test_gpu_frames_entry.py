"""GPU: SynergyNet.get_all_outputs_frames -- frames in, faces out with the detections kept on the device (FaceBoxes.detect_faces ->
syn_compact_detections -> syn_face_tables -> syn_crop_resize_frames) -- against get_all_outputs_batch(frames), the path through the
host tables, array for array and bit for bit.  While the new entry point runs, the host pieces it replaces (detect_all, call_batch,
FaceBoxes._download, SynergyNet._face_tables, inference.lanczos4_tables) are patched to raise."""
import numpy as np
import pytest

import synergy_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def det():
    from synergynet_amd import synth
    from synergynet_amd.faceboxes import FaceBoxes
    return FaceBoxes(state_dict=synth.make_faceboxes_state())


@pytest.fixture(scope='module')
def model(det):
    from synergynet_amd import synth
    from synergynet_amd.synergy3DMM import SynergyNet
    m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(n_vert=640), backbone_state=synth.make_backbone_state(), face_detector=det)
    seed = int(np.load(sc.GOLDEN, allow_pickle=False)['seed'])
    m.load_synergy_state(synth.make_synergy_state(seed))
    return m


@pytest.fixture(scope='module')
def frames():
    from synergynet_amd import synth
    return [synth.make_frame(300, 420, seed=300), synth.make_frame(240, 320, seed=302), synth.make_frame(300, 420, seed=303),
            np.zeros((240, 320, 3), np.uint8)]


@pytest.fixture(scope='module')
def want(model, frames):
    """get_all_outputs_batch(frames) once per (dense, refine), shared and left unchanged."""
    out = {(d, r): model.get_all_outputs_batch(frames, dense=d, refine=r) for d, r in ((True, False), (False, False), (True, True))}
    counts = [len(t[0]) for t in out[(True, False)]]
    assert sum(counts) > 0, counts
    return out


def _same(out, want):
    assert len(out) == len(want)
    for (l, v, p), (l2, v2, p2) in zip(out, want):
        assert len(l) == len(l2) and len(v) == len(v2) and len(p) == len(p2)
        for a, b in zip(l, l2):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        for a, b in zip(v, v2):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        for (a, ta), (b, tb) in zip(p, p2):
            assert a == b and np.array_equal(ta, tb)


def _no_host_tables(mp, det):
    from synergynet_amd import inference
    from synergynet_amd.synergy3DMM import SynergyNet

    def forbidden(name):
        def f(*a, **k):
            raise AssertionError(f'get_all_outputs_frames went through {name}')
        return f
    for name in ('detect_all', 'call_batch', '_download'):
        mp.setattr(det, name, forbidden(name))
    mp.setattr(SynergyNet, '_face_tables', staticmethod(forbidden('_face_tables')))
    mp.setattr(inference, 'lanczos4_tables', forbidden('lanczos4_tables'))
    mp.setattr(inference, '_lanczos4_tables_cached', forbidden('_lanczos4_tables_cached'))


@pytest.mark.parametrize('dense,refine', [(True, False), (False, False), (True, True)])
def test_frames_entry_equals_the_batch_entry(model, det, frames, want, monkeypatch, dense, refine):
    with monkeypatch.context() as mp:
        _no_host_tables(mp, det)
        out = model.get_all_outputs_frames(frames, dense=dense, refine=refine)
    _same(out, want[(dense, refine)])
    assert model.last_timing['faces'] == sum(len(t[0]) for t in out)


def test_device_resident_result_equals_the_host_arrays(model, det, frames, want, monkeypatch):
    import torch
    with monkeypatch.context() as mp:
        _no_host_tables(mp, det)
        out = model.get_all_outputs_frames(frames, to_host=False)
        lmk_only = model.get_all_outputs_frames(frames, dense=False, to_host=False)
    w = want[(True, False)]
    counts = [len(t[0]) for t in w]
    n = sum(counts)
    assert out['frame_faces'] == counts and lmk_only['frame_faces'] == counts and lmk_only['mesh'] is None
    for k in ('lmk', 'angles', 't3d', 'mesh', 'roi', 'face_frame'):
        assert isinstance(out[k], torch.Tensor) and out[k].is_cuda and out[k].shape[0] == n, k
    assert np.array_equal(out['face_frame'].cpu().numpy(), np.repeat(np.arange(4), counts))
    assert np.array_equal(out['lmk'].cpu().numpy(), np.stack([a for t in w for a in t[0]]))
    assert np.array_equal(out['mesh'].cpu().numpy(), np.stack([a for t in w for a in t[1]]))
    assert out['angles'].cpu().numpy().tolist() == [p[0] for t in w for p in t[2]]
    assert np.array_equal(out['t3d'].cpu().numpy(), np.stack([p[1] for t in w for p in t[2]]))
    assert np.array_equal(lmk_only['lmk'].cpu().numpy(), out['lmk'].cpu().numpy())
    # the ROI is the one the host path computes from the detector's rows
    rects = det.call_batch(frames)
    from synergynet_amd.synergy3DMM import SynergyNet
    roi = SynergyNet._face_tables(rects, n)[0]
    assert np.array_equal(out['roi'].cpu().numpy().view(np.uint32), roi.view(np.uint32))


def test_detect_faces_equals_call_batch(det, frames):
    import torch
    want = det.call_batch(frames)
    rows, face_frame, frame_faces = det.detect_faces(frames)
    assert rows.is_cuda and face_frame.is_cuda and frame_faces.is_cuda
    torch.cuda.synchronize()
    counts = [len(r) for r in want]
    assert frame_faces.cpu().tolist() == counts + [sum(counts)]
    n = sum(counts)
    assert np.array_equal(rows[:n].cpu().numpy(), np.array([r for fr in want for r in fr], dtype=np.float32).reshape(n, 5))
    assert np.array_equal(face_frame[:n].cpu().numpy(), np.repeat(np.arange(4), counts))
    # one [m,H,W,3] block on the device is used in place
    block = torch.from_numpy(np.stack([frames[0], frames[2]])).cuda()
    rows2, _, ff2 = det.detect_faces(block)
    torch.cuda.synchronize()
    assert ff2.cpu().tolist() == [counts[0], counts[2], counts[0] + counts[2]]
    assert np.array_equal(rows2[:counts[0]].cpu().numpy(), rows[:counts[0]].cpu().numpy())


def test_a_single_frame(model, det, frames, monkeypatch):
    """(Against the batch entry on the same single frame: the backbone's schedule, and with it the last bits, depends on the batch.)"""
    with monkeypatch.context() as mp:
        _no_host_tables(mp, det)
        out = model.get_all_outputs_frames(frames[:1])
    assert len(out[0][0]) > 0
    _same(out, model.get_all_outputs_batch(frames[:1]))


def test_no_face_anywhere_gives_empty_triples(model, det, frames, monkeypatch):
    """No score exceeds a visualisation threshold of 2, so no frame yields a face (a synthetic detector finds faces anywhere)."""
    from synergynet_amd import faceboxes
    two = frames[:2]
    empties = model.get_all_outputs_batch(two, rects=[[], []])
    assert empties == [([], [], []), ([], [], [])]

    def no_launch(*a, **k):
        raise AssertionError('a launch after n == 0')
    with monkeypatch.context() as mp:
        _no_host_tables(mp, det)
        mp.setattr(faceboxes, 'vis_thres', 2.0)
        mp.setattr(model, 'face_tables', no_launch)
        assert model.get_all_outputs_frames(two) == empties
        dev = model.get_all_outputs_frames(two, to_host=False)
    assert dev['frame_faces'] == [0, 0] and dev['lmk'].shape[0] == 0 and dev['mesh'].shape[0] == 0
    assert model.get_all_outputs_frames([]) == []


def test_a_degenerate_box_raises_where_the_host_path_raises(model, det, frames, want):
    """A detector that hands over a zero-height row next to a good one: the flag comes down with the results and raises the host
    path's error; the model is usable afterwards."""
    import torch
    rows = [[10.0, 20.0, 90.0, 100.0, 0.9], [10.0, 40.0, 60.0, 40.0, 0.9]]

    class Stub:
        def detect_faces(self, views, max_frames=16):
            return (torch.tensor(rows, dtype=torch.float32, device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda'),
                    torch.tensor([2, 2], dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='degenerate detection box'):
        model.get_all_outputs_batch(frames[:1], rects=[[[np.float32(v) for v in r] for r in rows]])
    model.face_detector = Stub()
    try:
        with pytest.raises(ValueError, match='degenerate detection box'):
            model.get_all_outputs_frames(frames[:1])
    finally:
        model.face_detector = det
    _same(model.get_all_outputs_frames(frames, dense=False), want[(False, False)])


def test_a_plain_callable_detector_falls_back(model, det, frames, want):
    model.face_detector = lambda f: det(f)
    try:
        _same(model.get_all_outputs_frames(frames), want[(True, False)])
        with pytest.raises(RuntimeError, match='detect_faces'):
            model.get_all_outputs_frames(frames, to_host=False)
    finally:
        model.face_detector = det
