"""The critic and the TD target on the CPU tier: the cases of tests/td_cases.py on the g++ build of the product sources (pmg_k_mlp over
MlpCatRows, pmg_k_td_target with the fmaf body of the matrix step) over the fiber emulator, through the C ABI.  The emulator proves the
concatenation, the tile hand-over between the two networks, the padding and the epilogue; the lane maps of the MFMA are proven by
tests/test_gpu_td.py."""
import pytest

import td_cases as TC


@pytest.mark.parametrize('x_dim', TC.Q_XDIMS)
def test_q_is_the_forward_on_concatenated_rows(emu_library, x_dim):
    TC.case_q_is_forward(emu_library, (x_dim,))


def test_exact_integers_name_the_column(emu_library):
    TC.case_exact_integers(emu_library)


@pytest.mark.parametrize('hidden', TC.TD_HIDDEN)
def test_td_identity_actor_is_bit_exact(emu_library, hidden):
    TC.case_td_identity(emu_library, hidden)


def test_td_every_batch(emu_library):
    TC.case_td_batches(emu_library)


def test_td_tanh_actor(emu_library):
    TC.case_td_tanh(emu_library)


def test_stale_tile_contents(emu_library):
    TC.case_stale_tile(emu_library)


def test_epilogue(emu_library):
    TC.case_epilogue(emu_library)


def test_from_the_sampler(emu_library):
    TC.case_from_the_sampler(emu_library)


def test_invalid_calls(emu_library):
    TC.case_invalid_calls(emu_library)
