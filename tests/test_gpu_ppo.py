"""The PPO calls on the MI355X: the cases of tests/ppo_cases.py on libpmg_hip.so (pmg_k_gae, pmg_k_adv_stats, pmg_k_adv_apply,
pmg_k_ppo_policy_grad_rows and pmg_k_ppo_stats as gfx950 code, the matrix step the f32-input MFMA, the head through the device's expf, the
normaliser through its double sqrt and division), through the C ABI."""
import pytest

import ppo_cases as PP

pytestmark = pytest.mark.gpu


def test_gae_is_the_fmaf_chain(hip_library):
    PP.case_gae(hip_library)                                     # every T x N; cuts at both ends and mid-rollout, terminals with and without


def test_advantage_statistics_and_apply(hip_library):
    PP.case_adv(hip_library)


def test_against_existing_calls_and_the_float32_model(hip_library):
    PP.case_sequence(hip_library)                                # every (Dx, A); every branch of the clip and of the clamp occurs on the device's own outputs


def test_against_float64_autograd(hip_library):
    PP.case_autograd(hip_library)


def test_the_samplers_own_records_give_a_ratio_of_one(hip_library):
    PP.case_same_weights(hip_library)


def test_edges(hip_library):
    PP.case_edges(hip_library)


def test_stale_tile_contents(hip_library):
    PP.case_stale_tile(hip_library)


def test_properties(hip_library):
    PP.case_properties(hip_library)


def test_minibatch_statistics(hip_library):
    PP.case_stats(hip_library)


def test_through_the_faces(hip_library):
    PP.case_host_face(hip_library)


def test_invalid_calls(hip_library):
    PP.case_invalid_calls(hip_library)
