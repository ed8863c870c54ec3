"""The HER sampler on the MI355X: the cases of tests/her_cases.py on libpmg_hip.so (pmg_k_her_draw, pmg_k_her_rows as gfx950
code), through the C ABI."""
import pytest

import her_cases as HC

pytestmark = pytest.mark.gpu

TASKS = pytest.mark.parametrize('task', HC.TASK_NAMES)


def test_draws(hip_library):
    HC.case_draws(hip_library)


@TASKS
def test_raw_gather(hip_library, task):
    HC.case_raw_gather(hip_library, task)


@TASKS
def test_normalised_rows(hip_library, task):
    HC.case_normalised_rows(hip_library, task)


@TASKS
def test_reward_and_flag(hip_library, task):
    HC.case_reward_and_flag(hip_library, task)


@pytest.mark.parametrize('task', ['push', 'block_stack'])
def test_reward_is_the_reward_kernels(hip_library, task):
    HC.case_reward_is_the_reward_kernels(hip_library, task)


def test_sweep_edges(hip_library):
    HC.case_sweep_edges(hip_library)


def test_determinism_and_independence(hip_library):
    HC.case_determinism(hip_library)


def test_handle_untouched(hip_library):
    HC.case_handle_untouched(hip_library)


@pytest.mark.parametrize('overlap', [False, True])
def test_with_the_env(hip_library, overlap):
    HC.case_with_the_env(hip_library, overlap)


def test_invalid_calls(hip_library):
    HC.case_invalid_calls(hip_library)
