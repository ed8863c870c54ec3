"""The critic and the TD target on the MI355X: the cases of tests/td_cases.py on libpmg_hip.so (pmg_k_mlp over MlpCatRows and
pmg_k_td_target as gfx950 code, the matrix step the f32-input MFMA), through the C ABI."""
import pytest

import td_cases as TC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('x_dim', TC.Q_XDIMS)
def test_q_is_the_forward_on_concatenated_rows(hip_library, x_dim):
    TC.case_q_is_forward(hip_library, (x_dim,))


def test_exact_integers_name_the_column(hip_library):
    TC.case_exact_integers(hip_library)


@pytest.mark.parametrize('hidden', TC.TD_HIDDEN)
def test_td_identity_actor_is_bit_exact(hip_library, hidden):
    TC.case_td_identity(hip_library, hidden)


def test_td_every_batch(hip_library):
    TC.case_td_batches(hip_library)


def test_td_tanh_actor(hip_library):
    TC.case_td_tanh(hip_library)


def test_stale_tile_contents(hip_library):
    TC.case_stale_tile(hip_library)


def test_epilogue(hip_library):
    TC.case_epilogue(hip_library)


def test_from_the_sampler(hip_library):
    TC.case_from_the_sampler(hip_library)


def test_invalid_calls(hip_library):
    TC.case_invalid_calls(hip_library)
