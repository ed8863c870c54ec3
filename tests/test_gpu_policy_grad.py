"""The policy gradient in one call on the MI355X: the cases of tests/policy_grad_cases.py on libpmg_hip.so (pmg_k_policy_grad_rows as gfx950
code, every matrix step the f32-input MFMA, then the weights kernel or the partials / merge pair of the earlier gradients), through the C ABI."""
import pytest

import policy_grad_cases as PC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('hidden', PC.HIDDEN)
def test_bit_equal_to_the_sequence_of_existing_calls(hip_library, hidden):
    PC.case_bit_exact(hip_library, hidden)


def test_chunk_rows(hip_library):
    PC.case_chunks(hip_library)


def test_every_batch(hip_library):
    PC.case_every_batch(hip_library)


def test_tanh_outputs(hip_library):
    PC.case_tanh(hip_library)


def test_clip_edges(hip_library):
    PC.case_clip_edges(hip_library)


def test_stale_tile_both_directions(hip_library):
    PC.case_stale_tile(hip_library)


def test_order_and_independence(hip_library):
    PC.case_independence(hip_library)


def test_through_the_faces(hip_library):
    PC.case_through_the_faces(hip_library)


def test_invalid_calls(hip_library):
    PC.case_invalid_calls(hip_library)
