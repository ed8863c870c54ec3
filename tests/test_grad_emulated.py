"""Back-propagation, Adam and Polyak on the CPU tier: the cases of tests/grad_cases.py on the g++ build of the product sources
(pmg_k_mlp_grad_rows, pmg_k_mlp_grad_weights with the fmaf bodies of the two matrix steps, pmg_k_adam, pmg_k_polyak) over the fiber emulator,
through the C ABI.  The emulator proves the chains' orders, the masks, the heads, the padding and the workspace layout; the lane maps of
the two new MFMA steps are proven by tests/test_gpu_grad.py."""
import pytest

import grad_cases as GC


@pytest.mark.parametrize('hidden', GC.HIDDEN)
def test_cat_rows_are_bit_exact(emu_library, hidden):
    GC.case_bit_exact(emu_library, GC.cat_cases(hidden))


def test_raw_rows_are_bit_exact(emu_library):
    GC.case_bit_exact(emu_library, GC.RAW_CASES)


def test_extreme_shapes_are_bit_exact(emu_library):
    GC.case_bit_exact(emu_library, GC.EXTREME_CASES)


def test_every_batch(emu_library):
    GC.case_every_batch(emu_library)


def test_tanh_output(emu_library):
    GC.case_tanh(emu_library)


def test_lane_maps_name_themselves(emu_library):
    GC.case_lane_maps(emu_library)


def test_heads(emu_library):
    GC.case_heads(emu_library)


def test_stale_tile_and_masks(emu_library):
    GC.case_stale_tile(emu_library)


def test_order_and_independence(emu_library):
    GC.case_independence(emu_library)


def test_adam(emu_library):
    GC.case_adam(emu_library)


def test_polyak(emu_library):
    GC.case_polyak(emu_library)


def test_invalid_calls(emu_library):
    GC.case_invalid_calls(emu_library)
