"""The data-parallel learner on the CPU tier (tests/dp_cases.py) on the g++ build of the product sources over the fiber emulator, through the C
ABI: pmg_k_params_pack, pmg_k_params_merge_ranks and pmg_k_adam_merge_ranks with ranks simulated as slots in one process, and the collectives
(pmg_mlp_grad_allreduce_device, pmg_mlp_adam_allreduce_device, pmg_norm_update_ranks_device, pmg_norm_update_env_ranks_device,
pmg_allgather_device) in 2 and 4 real processes over the emulator's shared-memory stand-in for RCCL.  The emulator proves the flat order, the
order of the sum, the slot stride, the chunk arithmetic of the collective normaliser update and the control flow of every rank; the gfx950
code of the three kernels is proven by tests/test_gpu_dp.py."""
import os

import pytest

import dp_cases as DP


@pytest.mark.parametrize('B_local', DP.B_LOCALS)
@pytest.mark.parametrize('R', DP.RANKS)
def test_merged_slices_are_the_chunked_gradient_of_the_whole_batch(emu_library, R, B_local):
    DP.case_simulated_ranks(emu_library, R, B_local)


def test_policy_gradient_slices(emu_library):
    DP.case_policy_grad_ranks(emu_library)


def test_sac_policy_gradient_slices(emu_library):
    DP.case_sac_policy_grad_ranks(emu_library)


def test_zeros_infinities_and_nans_follow_the_order_of_the_sum(emu_library):
    DP.case_special_values(emu_library)


def test_pack_then_merge_of_one_slot_returns_the_input_bits(emu_library):
    DP.case_one_slot_is_a_copy(emu_library)


def test_fused_merge_and_adam_against_merge_then_adam(emu_library):
    DP.case_fused_adam(emu_library)


def test_one_rank_collectives_are_the_single_rank_calls(emu_library):
    DP.case_one_rank(emu_library)


@pytest.mark.parametrize('world', (2, 4))
def test_real_ranks_end_with_the_single_process_bits(emu_library, world):
    """gradient all-reduce, fused all-reduce + Adam, the collective normaliser update (rows, masked rows; with two ranks a chunk of 192 and
    the env's rows) and the temperature step from gathered log-probabilities, on every rank against the single-process call"""
    DP.run_ranks(world, os.path.abspath(emu_library.path))
