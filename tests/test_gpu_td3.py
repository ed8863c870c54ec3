"""TD3's target on the MI355X: the cases of tests/td3_cases.py on libpmg_hip.so (pmg_k_td3_target as gfx950 code, the matrix step the
f32-input MFMA, the smoothing term through the device's logf / sqrtf / cosf), through the C ABI."""
import pytest

import td3_cases as T3

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('hidden', T3.HIDDEN)
def test_one_critic_without_noise_is_td_target(hip_library, hidden):
    T3.case_degenerate(hip_library, hidden)                      # every pair (Dx, A) x every batch x both actor activations


def test_twin_critics_without_noise(hip_library):
    T3.case_twin(hip_library)


def test_smoothing(hip_library):
    T3.case_smoothing(hip_library)


def test_stale_tile_contents(hip_library):
    T3.case_stale_tile(hip_library)


def test_epilogue(hip_library):
    T3.case_epilogue(hip_library)


def test_invalid_calls(hip_library):
    T3.case_invalid_calls(hip_library)


def test_env_critic_td3_target_equals_the_model(hip_library):
    T3.case_host_face(hip_library)
