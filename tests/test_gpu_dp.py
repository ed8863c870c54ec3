"""The data-parallel learner on the MI355X (tests/dp_cases.py) on libpmg_hip.so, one device: pmg_k_params_pack, pmg_k_params_merge_ranks and
pmg_k_adam_merge_ranks as gfx950 code with ranks simulated as slots, at the shapes of the CPU tier, and the collectives over a one-rank RCCL
communicator, where each is its single-rank call.  More than one rank on hardware is not tested here."""
import pytest

import dp_cases as DP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B_local', DP.B_LOCALS)
@pytest.mark.parametrize('R', DP.RANKS)
def test_merged_slices_are_the_chunked_gradient_of_the_whole_batch(hip_library, R, B_local):
    DP.case_simulated_ranks(hip_library, R, B_local)


def test_policy_gradient_slices(hip_library):
    DP.case_policy_grad_ranks(hip_library)


def test_sac_policy_gradient_slices(hip_library):
    DP.case_sac_policy_grad_ranks(hip_library)


def test_zeros_infinities_and_nans_follow_the_order_of_the_sum(hip_library):
    DP.case_special_values(hip_library)


def test_pack_then_merge_of_one_slot_returns_the_input_bits(hip_library):
    DP.case_one_slot_is_a_copy(hip_library)


def test_fused_merge_and_adam_against_merge_then_adam(hip_library):
    DP.case_fused_adam(hip_library)


def test_one_rank_rccl_collectives_are_the_single_rank_calls(hip_library):
    DP.case_one_rank(hip_library)
