"""features.15-17 (fused_block_lb4.hip) with the weights loaded global -> LDS directly: nothing orders such a load but the counted wait and the
barrier behind it, so a wait lost on a stage's first group, on its last group, on the hand-over between two stages of the chain or at the end
of the kernel shows as wrong weights in some workgroup.  Through syn_mobilenet2_span from features.15, the probes of mobilenet2_cases (helpers
and cached references of tests/test_gpu_mobilenet2_spans.py): the integer probe bit for bit with the launch codes of expected_tags, the gaussian
checkpoint within span_bound, at
  B = 1     the hidden-sliced instantiation (thirty slices of ONE group: prologue and last group with nothing between), seven of eight waves idle
  B = 4     one full workgroup
  B = 5     a second workgroup of one real face and three clamped ones
  B = 576   the smallest batch at which the launcher selects fused_chain_lb4_kernel (read from the launcher), and 577: a ragged last workgroup
on the spans 15-15, 16-16, 17-17 (single blocks: no next stage) and 15-17 (the chain from 576 faces: two hand-overs, the 320-channel stage)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mobilenet2_cases as mc
import test_gpu_mobilenet2_spans as sp
from test_gpu_mobilenet2_spans import handles  # noqa: F401  (the module-scoped fixture: schedule -> handle)

pytestmark = pytest.mark.gpu
SPANS = [(15, 15), (16, 16), (17, 17), (15, 17)]
SPAN_IDS = [f'{a}-{b}' for a, b in SPANS]


def chain_min_batch():
    """lb4_min_batch() of the launcher, from its source"""
    from conftest import ROOT
    src = open(os.path.join(ROOT, 'synergynet_amd', 'csrc', 'fused_block_lb4.hip')).read()
    body = src[src.index('static int lb4_min_batch()'):]
    return int(re.search(r'constexpr int min_b = (\d+);', body[:body.index('}')]).group(1))


def batches():
    t = chain_min_batch()
    return [1, 4, 5, t, t + 1]


def test_the_threshold_is_the_one_the_schedule_table_knows():
    assert chain_min_batch() == mc.LB4_MIN


@pytest.mark.parametrize('first,last', SPANS, ids=SPAN_IDS)
def test_integer_probe_bit_for_bit(handles, first, last):
    m, _ = handles('default', 'integer')
    faces, refs = sp._integer_probe(first, last, True)
    t = chain_min_batch()
    for B in batches():
        idx = sp._index(B)
        out, _, tags = sp.call_span(m, first, last, faces[idx])
        what = f'features {first}-{last} B={B} launches {tags}'
        assert tags == mc.expected_tags(first, last, B), what
        assert tags == ([1517] if (first, last) == (15, 17) and B >= t else list(range(first, last + 1))), what
        sp._assert_equal(out, refs[0][idx], what)


@pytest.mark.parametrize('first,last', SPANS, ids=SPAN_IDS)
def test_gaussian_checkpoint_within_span_bound(handles, first, last):
    m, sd = handles('default', 'gaussian')
    worst = {}
    for name, x, xd in sp._gaussian_inputs(sd, first):
        refs, bound = sp._gaussian_reference(sd, first, last, name, x, 'f16x2')
        for B in batches():
            idx = sp._index(B)
            out, _, tags = sp.call_span(m, first, last, xd[idx])
            worst[name, B] = sp._ratio(out, refs[0][idx], bound[idx])
    print(f'features {first}-{last} max(err / bound): ' + ', '.join(f'{k} {r:.3g}' for k, r in worst.items()))
    bad = {k: r for k, r in worst.items() if not r < 1.0}
    assert not bad, f'features {first}-{last}: err / bound {bad}'


@pytest.mark.parametrize('B', [5, 'chain + 1'], ids=['sliced', 'chain'])
def test_two_forwards_back_to_back_on_one_handle(handles, B):
    """Two calls of features.15-17 queued on one stream with nothing between them, each into its own output: a load still in flight when a
    kernel ends, or across the loop's back edge, lands in the LDS of whatever runs next.  Both outputs equal the reference."""
    import torch
    m, _ = handles('default', 'integer')
    B = chain_min_batch() + 1 if B == 'chain + 1' else B
    faces, refs = sp._integer_probe(15, 17, True)
    idx = sp._index(B)
    x = faces[idx].contiguous()
    n_in, out_shape, _ = mc.span_counts(15, 17, B)
    outs = [torch.full((int(np.prod(out_shape)),), float('nan'), dtype=torch.float32, device=m.device) for _ in range(2)]
    tags = (ctypes.c_int * 64)()
    for o in outs:
        n = m._lib.syn_mobilenet2_span(m._h, 15, 17, x.data_ptr(), 0, B, n_in, o.data_ptr(), o.numel(), None, 0, tags, 64, m._stream())
        assert n > 0, n
    torch.cuda.synchronize()
    assert list(tags[:n]) == mc.expected_tags(15, 17, B)
    for i, o in enumerate(outs):
        sp._assert_equal(o.view(out_shape), refs[0][idx], f'features 15-17 B={B} call {i}')
