"""The policy gradient in one call on the CPU tier: the cases of tests/policy_grad_cases.py on the g++ build of the product sources
(pmg_k_policy_grad_rows with the fmaf bodies of the matrix steps, then pmg_k_mlp_grad_weights or the partials / merge pair) over the fiber
emulator, through the C ABI.  The emulator proves the two hand-overs, the head, the padding, the order of the chains and the workspace layout;
the lane maps of the MFMA steps the kernel shares with its siblings are proven by tests/test_gpu_grad.py, and tests/test_gpu_policy_grad.py
repeats these cases on the gfx950 build."""
import pytest

import policy_grad_cases as PC


@pytest.mark.parametrize('hidden', PC.HIDDEN)
def test_bit_equal_to_the_sequence_of_existing_calls(emu_library, hidden):
    PC.case_bit_exact(emu_library, hidden)


def test_chunk_rows(emu_library):
    PC.case_chunks(emu_library)


def test_every_batch(emu_library):
    PC.case_every_batch(emu_library)


def test_tanh_outputs(emu_library):
    PC.case_tanh(emu_library)


def test_clip_edges(emu_library):
    PC.case_clip_edges(emu_library)


def test_stale_tile_both_directions(emu_library):
    PC.case_stale_tile(emu_library)


def test_order_and_independence(emu_library):
    PC.case_independence(emu_library)


def test_invalid_calls(emu_library):
    PC.case_invalid_calls(emu_library)
