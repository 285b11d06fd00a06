"""CPU-side tests of the mesh-consumer edge cases (no GPU): the oracle the GPU tests compare against (oracle/sim3dr.py) is held to the
fixture the reference's own code produced on the inputs of tests/mesh_edge_cases.py (tests/golden/mesh_edges_golden.npz, written by
tests/golden/make_mesh_edges_golden.py), and every non-vacuity condition of the cases is asserted on the oracle's output.

Bars: images and normals byte for byte; vertex colours to 1e-6 (numpy's float32 power differs in the last bit between CPU back
ends, as in tests/test_render_cpu.py)."""
import os

import numpy as np
import pytest

import mesh_edge_cases as mc
from conftest import ROOT
from oracle import sim3dr as osim

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mesh_edges_golden.npz')


@pytest.fixture(scope='module')
def mgold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope='module')
def oracle_out():
    return mc.expected_images(osim), mc.expected_lights(osim)


def test_fixture_is_small_and_holds_expected_outputs_only(mgold, oracle_out):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert set(mgold) == set(oracle_out[0]) | set(oracle_out[1])
    assert all(v.dtype in (np.uint8, np.float32) for v in mgold.values())


def test_oracle_images_and_normals_equal_the_reference_fixture(mgold, oracle_out):
    img, lit = oracle_out
    for k, v in img.items():
        assert v.dtype == np.uint8 and np.array_equal(v, mgold[k]), k
    for k in ('c_normal', 'c_flat_normal'):
        assert lit[k].tobytes() == mgold[k].tobytes(), k                # bytes: NaN rows and the sign of a zero count


def test_oracle_lights_equal_the_reference_fixture(mgold, oracle_out):
    lit = oracle_out[1]
    for k, v in lit.items():
        if 'normal' in k:
            continue
        assert np.array_equal(np.isnan(v), np.isnan(mgold[k])), k
        np.testing.assert_allclose(v, mgold[k], rtol=0, atol=mc.LIGHT_ATOL, equal_nan=True, err_msg=k)


def test_every_case_tests_what_it_is_there_for(oracle_out):
    figures = mc.check_nonvacuity(osim, *oracle_out)
    for k, v in figures.items():
        print(k, v)


def test_flat_colour_table_is_the_low_byte_of_a_32_bit_integer():
    """The measured values of the reference's conversion against plain integer arithmetic on 255 * p in float32."""
    for value, byte in mc.FLAT_COLOURS:
        assert int(np.float32(255) * np.float32(value)) & 0xff == byte


@pytest.mark.skipif(not osim.ref_available(), reason='oracle/_ref (the reference compiled where it lies) is not on this machine')
def test_fixture_images_are_the_reference_librarys(mgold):
    for k, v in mc.expected_images(osim, impl='ref').items():
        assert np.array_equal(v, mgold[k]), k
    lit = mc.expected_lights(osim, impl='ref')
    for k in ('c_normal', 'c_flat_normal'):
        assert lit[k].tobytes() == mgold[k].tobytes(), k
