"""Back-propagation, Adam and Polyak on the MI355X: the cases of tests/grad_cases.py on libpmg_hip.so (pmg_k_mlp_grad_rows and
pmg_k_mlp_grad_weights as gfx950 code, both matrix steps the f32-input MFMA; pmg_k_adam, pmg_k_polyak), through the C ABI.  The exact-integer
case is the proof of the A / B / C lane maps of the transposed step and of the weights step."""
import pytest

import grad_cases as GC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('hidden', GC.HIDDEN)
def test_cat_rows_are_bit_exact(hip_library, hidden):
    GC.case_bit_exact(hip_library, GC.cat_cases(hidden))


def test_raw_rows_are_bit_exact(hip_library):
    GC.case_bit_exact(hip_library, GC.RAW_CASES)


def test_extreme_shapes_are_bit_exact(hip_library):
    GC.case_bit_exact(hip_library, GC.EXTREME_CASES)


def test_every_batch(hip_library):
    GC.case_every_batch(hip_library)


def test_tanh_output(hip_library):
    GC.case_tanh(hip_library)


def test_lane_maps_name_themselves(hip_library):
    GC.case_lane_maps(hip_library)


def test_heads(hip_library):
    GC.case_heads(hip_library)


def test_stale_tile_and_masks(hip_library):
    GC.case_stale_tile(hip_library)


def test_order_and_independence(hip_library):
    GC.case_independence(hip_library)


def test_adam(hip_library):
    GC.case_adam(hip_library)


def test_polyak(hip_library):
    GC.case_polyak(hip_library)


def test_whole_update_through_the_faces(hip_library):
    GC.case_whole_update(hip_library)


def test_invalid_calls(hip_library):
    GC.case_invalid_calls(hip_library)
