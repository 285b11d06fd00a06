"""features.15-17 (fused_block_lb4.hip): the weight pipeline of the 4x4 kernels -- a group's weights are parked into LDS during the
depthwise of the group in front and fetched two groups ahead, its expand operands are requested during the previous group's project.
Batch sizes chosen for what that pipeline can get wrong (prologue and epilogue with nothing between them, the parity of the two buffer
halves, ragged workgroups, the hand-over between the chain's stages), through the public forward against the oracle: every face
within 1e-4 relative.  The chain against the blocks launched one by one: the SAME BITS."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4
CROPS_SEED = 7150
N_MAX = 580


@pytest.fixture(scope='module')
def model(pack, backbone_sd):
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from synergynet_amd.synergy3DMM import SynergyNet
    return SynergyNet(device='cuda:0', pack=pack, backbone_state=backbone_sd)


@pytest.fixture(scope='module')
def crops():
    from synergynet_amd import synth
    return synth.make_crops(N_MAX, seed=CROPS_SEED)


@pytest.fixture(scope='module')
def want(backbone_sd, crops):
    """the oracle's parameters of all N_MAX faces, computed once: every batch below is a prefix of the same crops"""
    import torch
    from oracle import backbone_torch
    from synergynet_amd import synth
    with torch.no_grad():
        out = [backbone_torch.mobilenet_v2_forward(backbone_sd, synth.normalize_crops(crops[i:i + 116]))[0].numpy() for i in range(0, N_MAX, 116)]
    return np.concatenate(out)


def per_face_rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


# B: workgroups of four faces x slices of the 30 hidden groups (launch_lb4_sliced: the fewest slices that give 192 workgroups)
@pytest.mark.parametrize('B,what', [
    (3, 'one workgroup, 30 slices of ONE group: prologue and epilogue with nothing between them'),
    (52, '15 slices of two groups'),
    (78, '10 slices of three groups: odd, the buffer half differs at the end'),
    (130, '6 slices of five groups, ragged last workgroup'),
    (386, '2 slices of 15 groups, the slices added by the tail (head_sliced_in)'),
    (577, 'the chain past its threshold of 576: a last workgroup of one real face, the stage hand-overs, the 320-channel stage'),
    (580, 'the chain, whole workgroups only'),
], ids=lambda v: f'B{v}' if isinstance(v, int) else '')
def test_every_face_within_tolerance_of_the_oracle(model, crops, want, B, what):
    import torch
    got = model.forward_crops_u8(torch.from_numpy(crops[:B]).cuda()).cpu().numpy()
    assert got.shape == (B, 62) and np.isfinite(got).all()
    err = per_face_rel(got, want[:B])
    print(f'B={B} ({what}): worst face {int(err.argmax())} rel err {err.max():.3e}')
    assert err.max() <= TOL, (B, int(err.argmax()), float(err.max()))


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from synergynet_amd import synth
from synergynet_amd.synergy3DMM import SynergyNet
m = SynergyNet(device='cuda:0', pack=synth.make_3dmm(int(sys.argv[4])), backbone_state=synth.make_backbone_state(int(sys.argv[3])))
B = int(sys.argv[5])
np.save(sys.argv[2], m.forward_crops_u8(torch.from_numpy(synth.make_crops(int(sys.argv[7]), seed=int(sys.argv[6]))[:B]).cuda()).cpu().numpy())
'''


def test_chain_equals_blocks_launched_one_by_one_bit_for_bit(model, crops, golden, tmp_path):
    """B = 577: the three stages in one launch (weights and expand operands handed from stage to stage) against test knob lb4_chain=0, one
    launch per block -- the same arithmetic in the same order.  The knobs are read once per process, hence the child."""
    import subprocess
    import sys
    import torch
    B = 577
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'p.npy')
    r = subprocess.run([sys.executable, '-c', _CHILD, root, out, str(int(golden['seeds'][0])), str(int(golden['seeds'][1])), str(B), str(CROPS_SEED), str(N_MAX)],
                       env=dict(os.environ, SYNERGY_HIP_TEST_KNOBS='lb4_chain=0'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = model.forward_crops_u8(torch.from_numpy(crops[:B]).cuda()).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(np.load(out), got)
