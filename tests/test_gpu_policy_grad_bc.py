"""The policy gradient with the behaviour-cloning term on the MI355X: the cases of tests/policy_grad_bc_cases.py on libpmg_hip.so
(pmg_k_policy_grad_bc_rows as gfx950 code, every matrix step the f32-input MFMA, then the weights kernel or the partials / merge pair of the
earlier gradients), through the C ABI."""
import pytest

import policy_grad_bc_cases as BC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('hidden', BC.HIDDEN)
def test_bit_equal_to_the_sequence_and_the_model(hip_library, hidden):
    BC.case_bit_exact(hip_library, hidden)


def test_every_switch(hip_library):
    BC.case_every_switch(hip_library)


def test_chunk_rows(hip_library):
    BC.case_chunks(hip_library)


def test_tanh_outputs(hip_library):
    BC.case_tanh(hip_library)


def test_demo_begin_against_the_tile(hip_library):
    BC.case_demo_begin(hip_library)


def test_the_equal_case(hip_library):
    BC.case_equal(hip_library)


def test_pure_cloning_is_the_mse_head(hip_library):
    BC.case_pure_cloning(hip_library)


def test_nan(hip_library):
    BC.case_nan(hip_library)


def test_stale_tile(hip_library):
    BC.case_stale_tile(hip_library)


def test_order_and_independence(hip_library):
    BC.case_independence(hip_library)


def test_through_the_faces(hip_library):
    BC.case_through_the_faces(hip_library)


def test_invalid_calls(hip_library):
    BC.case_invalid_calls(hip_library)
