"""The HER sampler on the CPU tier: the cases of tests/her_cases.py on the g++ build of the product sources (pmg_k_her_draw,
pmg_k_her_rows, pmg_her_sample_device, pmg_device_copy) over the fiber emulator, through the C ABI."""
import pytest

import her_cases as HC

TASKS = pytest.mark.parametrize('task', HC.TASK_NAMES)


def test_draws(emu_library):
    HC.case_draws(emu_library)


@TASKS
def test_raw_gather(emu_library, task):
    HC.case_raw_gather(emu_library, task)


@TASKS
def test_normalised_rows(emu_library, task):
    HC.case_normalised_rows(emu_library, task)


@TASKS
def test_reward_and_flag(emu_library, task):
    HC.case_reward_and_flag(emu_library, task)


@pytest.mark.parametrize('task', ['push', 'block_stack'])
def test_reward_is_the_reward_kernels(emu_library, task):
    HC.case_reward_is_the_reward_kernels(emu_library, task)


def test_sweep_edges(emu_library):
    HC.case_sweep_edges(emu_library)


def test_determinism_and_independence(emu_library):
    HC.case_determinism(emu_library)


def test_handle_untouched(emu_library):
    HC.case_handle_untouched(emu_library)


@pytest.mark.parametrize('overlap', [False, True])
def test_with_the_env(emu_library, overlap):
    HC.case_with_the_env(emu_library, overlap)


def test_invalid_calls(emu_library):
    HC.case_invalid_calls(emu_library)
