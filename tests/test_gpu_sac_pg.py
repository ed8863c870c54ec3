"""The fused SAC actor update on the MI355X: the cases of tests/sac_pg_cases.py on libpmg_hip.so (pmg_k_sac_policy_grad_rows and pmg_k_sac_alpha
as gfx950 code, the matrix step the f32-input MFMA, the head through the device's expf / tanhf), through the C ABI."""
import pytest

import sac_pg_cases as SP

pytestmark = pytest.mark.gpu


def test_against_the_sequence_of_existing_calls(hip_library):
    SP.case_sequence(hip_library)                                # every (Dx, A); q1 < q2, q2 < q1 and the clamp's three sides occur


def test_against_float64_autograd(hip_library):
    SP.case_autograd(hip_library)


def test_without_noise_and_entropy_is_the_ddpg_kernel(hip_library):
    SP.case_is_policy_grad(hip_library)


def test_edges(hip_library):
    SP.case_edges(hip_library)


def test_stale_tile_contents(hip_library):
    SP.case_stale_tile(hip_library)


def test_properties(hip_library):
    SP.case_properties(hip_library)


def test_temperature(hip_library):
    SP.case_alpha(hip_library)


def test_through_the_faces(hip_library):
    SP.case_host_face(hip_library)


def test_invalid_calls(hip_library):
    SP.case_invalid_calls(hip_library)
