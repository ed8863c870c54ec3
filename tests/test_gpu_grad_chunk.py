"""The chunked batch reduction on the MI355X: cases 1-7 and 9 of tests/grad_chunk_cases.py on libpmg_hip.so (pmg_k_mlp_grad_rows,
pmg_k_mlp_grad_partials and pmg_k_mlp_grad_merge as gfx950 code, the weights step the f32-input MFMA on a chunk's rows), through the C ABI
and, for the whole update, through env.actor / env.critic."""
import pytest

import grad_chunk_cases as CC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B', CC.GC.BATCHES)
@pytest.mark.parametrize('R', CC.CHUNKS)
@pytest.mark.parametrize('group', CC.GROUPS)
def test_chunked_gradients_are_bit_exact(hip_library, group, R, B):
    CC.case_bit_exact(hip_library, group, R, B)


@pytest.mark.parametrize('R', CC.CHUNKS)
def test_tanh_output(hip_library, R):
    CC.case_tanh(hip_library, R)


def test_chunk_edges(hip_library):
    CC.case_chunk_edges(hip_library)


def test_nothing_stale_is_read_and_everything_is_overwritten(hip_library):
    CC.case_nothing_stale(hip_library)


def test_order_within_chunks_and_chunk_length(hip_library):
    CC.case_order(hip_library)


def test_masks_and_inf(hip_library):
    CC.case_masks_and_inf(hip_library)


def test_input_only(hip_library):
    CC.case_input_only(hip_library)


def test_invalid_calls(hip_library):
    CC.case_invalid_calls(hip_library)


def test_whole_update_through_the_faces(hip_library):
    CC.case_whole_update(hip_library)
