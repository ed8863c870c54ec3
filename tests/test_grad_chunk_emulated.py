"""The chunked batch reduction on the CPU tier: cases 1-7 of tests/grad_chunk_cases.py on the g++ build of the product sources
(pmg_k_mlp_grad_rows, pmg_k_mlp_grad_partials with the fmaf body of the weights step, pmg_k_mlp_grad_merge) over the fiber emulator, through
the C ABI.  The emulator proves the chunk bounds, the order of the chains and of the merge, the layout of the partials and the validation;
the lane maps of the MFMA step on a chunk's rows are proven by tests/test_gpu_grad_chunk.py."""
import pytest

import grad_chunk_cases as CC


@pytest.mark.parametrize('B', CC.GC.BATCHES)
@pytest.mark.parametrize('R', CC.CHUNKS)
@pytest.mark.parametrize('group', CC.GROUPS)
def test_chunked_gradients_are_bit_exact(emu_library, group, R, B):
    CC.case_bit_exact(emu_library, group, R, B)


@pytest.mark.parametrize('R', CC.CHUNKS)
def test_tanh_output(emu_library, R):
    CC.case_tanh(emu_library, R)


def test_chunk_edges(emu_library):
    CC.case_chunk_edges(emu_library)


def test_nothing_stale_is_read_and_everything_is_overwritten(emu_library):
    CC.case_nothing_stale(emu_library)


def test_order_within_chunks_and_chunk_length(emu_library):
    CC.case_order(emu_library)


def test_masks_and_inf(emu_library):
    CC.case_masks_and_inf(emu_library)


def test_input_only(emu_library):
    CC.case_input_only(emu_library)


def test_invalid_calls(emu_library):
    CC.case_invalid_calls(emu_library)
