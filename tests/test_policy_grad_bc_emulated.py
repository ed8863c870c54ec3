"""The policy gradient with the behaviour-cloning term on the CPU tier: the cases of tests/policy_grad_bc_cases.py on the g++ build of the
product sources (pmg_k_policy_grad_bc_rows with the fmaf bodies of the matrix steps, then pmg_k_mlp_grad_weights or the partials / merge
pair) over the fiber emulator, through the C ABI.  The emulator proves the demonstration pass in front of the actor's forward, the filter's
hand-over through LDS, the head, the padding and the workspace layout; tests/test_gpu_policy_grad_bc.py repeats these cases on the gfx950
build."""
import pytest

import policy_grad_bc_cases as BC


@pytest.mark.parametrize('hidden', BC.HIDDEN)
def test_bit_equal_to_the_sequence_and_the_model(emu_library, hidden):
    BC.case_bit_exact(emu_library, hidden)


def test_every_switch(emu_library):
    BC.case_every_switch(emu_library)


def test_chunk_rows(emu_library):
    BC.case_chunks(emu_library)


def test_tanh_outputs(emu_library):
    BC.case_tanh(emu_library)


def test_demo_begin_against_the_tile(emu_library):
    BC.case_demo_begin(emu_library)


def test_the_equal_case(emu_library):
    BC.case_equal(emu_library)


def test_pure_cloning_is_the_mse_head(emu_library):
    BC.case_pure_cloning(emu_library)


def test_nan(emu_library):
    BC.case_nan(emu_library)


def test_stale_tile(emu_library):
    BC.case_stale_tile(emu_library)


def test_order_and_independence(emu_library):
    BC.case_independence(emu_library)


def test_invalid_calls(emu_library):
    BC.case_invalid_calls(emu_library)
