"""CPU-side tests of the texture completion (no GPU): the numpy definition the GPU tests compare against
(tests/texture_fill_cases.py) satisfies the properties it was designed for on the whole case list, the merged own value is the
rounded mean of the seeing views, the result does not depend on the order of the pyramid's sums, and header / ctypes table / library
agree on the new entry point."""
import ctypes
import os

import numpy as np
import pytest

import texture_fill_cases as fc
from conftest import ROOT

SMALL = [c[0] for c in fc.SIZE_CASES if c[2] * c[3] <= 300 * 200]


def test_new_symbol_in_header_ctypes_table_and_library():
    from synergynet_amd import abi
    from synergynet_amd.build import build_library
    hdr = open(os.path.join(ROOT, 'include', 'synergy_hip.h')).read()
    import torch  # noqa: F401
    l = ctypes.CDLL(build_library())
    assert 'syn_texture_fill(' in hdr and 'syn_texture_fill' in abi.EXPORTED_SYMBOLS and hasattr(l, 'syn_texture_fill')
    assert len(abi._SIGS['syn_texture_fill'][1]) == 10
    l.syn_abi_version.restype = ctypes.c_int
    assert l.syn_abi_version() == 1
    from synergynet_amd import sim3dr
    import inspect
    assert callable(sim3dr.fill_texture)
    assert inspect.signature(sim3dr.texture_from_image).parameters['fill'].default is False


@pytest.mark.parametrize('name', SMALL)
def test_definition_keeps_valid_texels_and_stays_within_their_range(name):
    tex, mask = fc.size_case(name)
    out = fc.fill(tex, mask)
    assert out.shape == tex.shape and out.dtype == np.uint8
    fc.invariants(tex, mask, out)
    # rank 3 is the same texture without the batch axis
    assert np.array_equal(fc.fill(tex[0], mask[0]), out[0])


def test_definition_on_the_mask_cases():
    for name, (tex, mask) in fc.mask_cases().items():
        out = fc.fill(tex, mask)
        fc.invariants(tex, mask, out)
        if name == 'all_valid':
            assert np.array_equal(out, tex)
        if name == 'empty':
            assert not out.any()
        if name == 'single_corner_130':
            assert (out == tex[0, 129, 129]).all() and tex[0, 129, 129].any()
        if name == 'left100':
            assert len(np.unique(out[0, :, 100:].reshape(-1, 3), axis=0)) > 100      # the hole is not one flat colour
    # a single valid texel floods a 64 x 64 texture, an empty mask gives zeros, also on odd sizes
    for H, W in ((64, 64), (5, 1), (37, 53)):
        tex, mask = fc.random_case(9, 1, H, W, 3, 0.0)
        assert not fc.fill(tex, mask).any()
        mask[0, H // 3, W // 2] = 255
        assert (fc.fill(tex, mask) == tex[0, H // 3, W // 2]).all()


@pytest.mark.parametrize('hw', [(1, 1), (5, 1), (37, 53), (64, 64), (300, 200)])
def test_constant_colour_comes_back_constant(hw):
    rng = np.random.default_rng(hw[0])
    for colour in ((0, 0, 0), (255, 255, 255), (1, 128, 254)):
        tex = np.broadcast_to(np.array(colour, np.uint8), (1,) + hw + (3,)).copy()
        mask = (rng.uniform(0, 1, (1,) + hw) < 0.2).astype(np.uint8)
        mask[0, hw[0] - 1, 0] = 1                                              # any non-empty mask
        tex[mask == 0] = 99                                                     # what invalid texels hold must not leak
        assert (fc.fill(tex, mask) == np.array(colour, np.uint8)).all()


@pytest.mark.parametrize('T', [1, 2, 5])
def test_merged_own_value_is_the_rounded_mean_of_the_seeing_views(T):
    tex, mask = fc.merge_case(T)
    out = fc.fill(tex, mask, merge=True)
    assert out.shape == tex.shape[1:]
    seen = (mask != 0).sum(0)
    assert (seen == 0).any() and (seen == T).any()
    total = (tex.astype(np.int64) * (mask != 0)[..., None]).sum(0)
    mean = np.floor(total / np.maximum(seen, 1)[..., None] + 0.5).astype(np.int64)     # exact in float64 at these magnitudes
    assert np.array_equal(out[seen > 0], mean[seen > 0].astype(np.uint8))
    lo, hi = tex[mask != 0].min(0), tex[mask != 0].max(0)
    assert (out >= lo).all() and (out <= hi).all()
    if T == 1:
        assert np.array_equal(out, fc.fill(tex, mask)[0])
    # the holes are filled from the merged sums, not from one view
    c0, w0 = fc.level0(tex, mask, merge=True)
    assert np.array_equal(out, fc.pull(*fc.pyramid(c0[0], w0[0])))


@pytest.mark.parametrize('name', ['5x1', '37x53', '65x130', '300x200'])
def test_reduction_order_does_not_change_a_byte(name):
    tex, mask = fc.size_case(name)
    want = fc.fill(tex, mask)
    for order in ('rows', 'cols'):
        assert fc.fill(tex, mask, order=order).tobytes() == want.tobytes(), order
    # and a pyramid whose level-2 sums, colours and weight, are taken straight from level 0 (4 x 4 blocks at once) and pushed on
    # from there: the same bytes again
    c0, w0 = fc.level0(tex, mask)
    cs, ws = fc.pyramid(c0[0], w0[0])
    if len(ws) > 2:
        H, W = w0[0].shape

        def blocks4(a):
            p = np.zeros(((H + 3) // 4 * 4, (W + 3) // 4 * 4) + a.shape[2:], np.uint64)
            p[:H, :W] = a
            return p.reshape((p.shape[0] // 4, 4, p.shape[1] // 4, 4) + a.shape[2:]).sum((1, 3), dtype=np.uint64)

        cs4, ws4 = fc.pyramid(blocks4(c0[0]), blocks4(w0[0]))
        assert np.array_equal(ws4[0], ws[2]) and np.array_equal(cs4[0], cs[2])
        assert fc.pull(cs[:2] + cs4, ws[:2] + ws4).tobytes() == want[0].tobytes()


def test_case_list_reaches_both_forms_of_the_pyramid_top():
    """The device code holds the sums above the tiles in one of two sizes, the threshold being 512 sums; the list must straddle it
    and reach the 5461 sums of 4096 x 4096."""
    sums = {c[0]: fc.top_sums(c[2], c[3]) for c in fc.SIZE_CASES}
    assert sums['1100x1100_ch1'] == 444 and sums['4096x70'] == 191 and sums['1024x512_2pct'] <= 512
    assert sums['1300x1300_ch1'] == 612 and sums['4096x4096_ch1'] == 5461
