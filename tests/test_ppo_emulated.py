"""The PPO calls on the CPU tier: the cases of tests/ppo_cases.py on the g++ build of the product sources (pmg_k_gae, pmg_k_adv_stats,
pmg_k_adv_apply, pmg_k_ppo_policy_grad_rows with the fmaf body of the matrix step, pmg_k_ppo_stats) over the fiber emulator, through the C ABI.
The emulator proves the addressing of GAE's tables, the two-level chains, the head's column map, the stash in the workspace and in d_ghead and
the hand-back; the lane maps of the MFMA, the build's expf and its double sqrt and division are proven by tests/test_gpu_ppo.py."""
import pytest

import ppo_cases as PP


@pytest.mark.parametrize('T', PP.GAE_T)
def test_gae_is_the_fmaf_chain(emu_library, T):
    PP.case_gae(emu_library, [(T, N) for N in PP.GAE_N])


def test_gae_cases_cover_the_boundaries(emu_library):
    assert PP.case_gae(emu_library, [(7, 65)]) == PP.GAE_COVERAGE


def test_advantage_statistics_and_apply(emu_library):
    PP.case_adv(emu_library)


@pytest.mark.parametrize('k', range(len(PP.CASES)))
def test_against_existing_calls_and_the_float32_model(emu_library, k):
    PP.case_sequence(emu_library, (k,))


def test_the_cases_cover_every_branch_on_the_own_outputs(emu_library):
    """all cases in one call: case_sequence asserts on the call's own rho, d_clipped and the log-stds that clipped rows on both sides, unclipped
    rows on both sides of 1 and log-stds below, inside and above the clamp occur for both policies"""
    assert PP.case_sequence(emu_library)[1] == PP.COVERAGE


def test_against_float64_autograd(emu_library):
    PP.case_autograd(emu_library)


@pytest.mark.parametrize('pair', PP.PAIRS)
def test_the_samplers_own_records_give_a_ratio_of_one(emu_library, pair):
    PP.case_same_weights(emu_library, (pair,))


def test_edges(emu_library):
    PP.case_edges(emu_library)


def test_stale_tile_contents(emu_library):
    PP.case_stale_tile(emu_library)


def test_properties(emu_library):
    PP.case_properties(emu_library)


def test_minibatch_statistics(emu_library):
    PP.case_stats(emu_library)


def test_through_the_faces(emu_library):
    PP.case_host_face(emu_library)


def test_invalid_calls(emu_library):
    PP.case_invalid_calls(emu_library)
