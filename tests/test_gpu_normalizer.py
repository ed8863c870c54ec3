"""The running normaliser / policy-input rows on the MI355X: the cases of tests/normalizer_cases.py on libpmg_hip.so
(pmg_k_norm_partial, pmg_k_norm_merge, pmg_k_policy_input as gfx950 code), through the C ABI."""
import pytest

import normalizer_cases as NC

pytestmark = pytest.mark.gpu

TASKS = pytest.mark.parametrize('task', NC.TASK_NAMES)


@TASKS
def test_fresh_handle(hip_library, task):
    NC.case_fresh_handle(hip_library, task)


@TASKS
def test_update_against_float64(hip_library, task):
    NC.case_update_against_float64(hip_library, task)


@TASKS
def test_catches_float32_accumulators(hip_library, task):
    NC.case_catches_float32_accumulators(hip_library, task)


@TASKS
def test_floors_and_clips(hip_library, task):
    NC.case_floors_and_clips(hip_library, task)


@TASKS
def test_stride_and_alignment(hip_library, task):
    NC.case_stride_and_alignment(hip_library, task)


@TASKS
def test_mask(hip_library, task):
    NC.case_mask(hip_library, task)


@TASKS
def test_incremental_and_deterministic(hip_library, task):
    NC.case_incremental_and_deterministic(hip_library, task)


@TASKS
def test_policy_input_exact(hip_library, task):
    NC.case_policy_input_exact(hip_library, task)


def test_with_the_env(hip_library):
    NC.case_with_the_env(hip_library)


@TASKS
def test_state_dict_round_trip(hip_library, task):
    NC.case_state_dict_round_trip(hip_library, task)


@TASKS
def test_write_and_configure(hip_library, task):
    NC.case_write_and_configure(hip_library, task)


@TASKS
def test_invalid_calls(hip_library, task):
    NC.case_invalid_calls(hip_library, task)
