"""SAC's Gaussian head and soft target on the MI355X: the cases of tests/sac_cases.py on libpmg_hip.so (pmg_k_sac and pmg_k_sac_target as gfx950
code, the matrix step the f32-input MFMA, the head through the device's logf / sqrtf / cosf / expf / tanhf / log1pf), through the C ABI."""
import pytest

import sac_cases as SC

pytestmark = pytest.mark.gpu


def test_sample(hip_library):
    SC.case_sample(hip_library)                                  # every (Dx, A) x every hidden shape; the clamp's three sides and |a| == 1 occur


def test_sample_properties(hip_library):
    SC.case_sample_properties(hip_library)


def test_env_acting(hip_library):
    SC.case_env(hip_library, 'push')


def test_target(hip_library):
    SC.case_target(hip_library)


def test_target_without_noise_and_temperature_is_td3(hip_library):
    SC.case_target_is_td3(hip_library)


def test_epilogue(hip_library):
    SC.case_epilogue(hip_library)


def test_stale_tile_contents(hip_library):
    SC.case_stale_tile(hip_library)


def test_invalid_calls(hip_library):
    SC.case_invalid_calls(hip_library)


def test_gaussian_actor_and_the_sac_step_equal_the_model(hip_library):
    SC.case_host_face(hip_library)
