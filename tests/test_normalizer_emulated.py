"""CPU tier of the running normaliser / policy-input rows: the cases of tests/normalizer_cases.py on the g++ build of
pmg_api.cpp + pmg_kernels.hip over the fiber emulator, through the C ABI."""
import pytest

import normalizer_cases as NC

TASKS = pytest.mark.parametrize('task', NC.TASK_NAMES)


@TASKS
def test_fresh_handle(emu_library, task):
    NC.case_fresh_handle(emu_library, task)


@TASKS
def test_update_against_float64(emu_library, task):
    NC.case_update_against_float64(emu_library, task)


@TASKS
def test_catches_float32_accumulators(emu_library, task):
    NC.case_catches_float32_accumulators(emu_library, task)


@TASKS
def test_floors_and_clips(emu_library, task):
    NC.case_floors_and_clips(emu_library, task)


@TASKS
def test_stride_and_alignment(emu_library, task):
    NC.case_stride_and_alignment(emu_library, task)


@TASKS
def test_mask(emu_library, task):
    NC.case_mask(emu_library, task)


@TASKS
def test_incremental_and_deterministic(emu_library, task):
    NC.case_incremental_and_deterministic(emu_library, task)


@TASKS
def test_policy_input_exact(emu_library, task):
    NC.case_policy_input_exact(emu_library, task)


@pytest.mark.parametrize('overlap', [False, True], ids=['one_row_buffer', 'overlapped_row_buffers'])
def test_with_the_env(emu_library, overlap):
    """overlapped_row_buffers: pmg_comm_overlap double-buffers the packed rows (no communicator needed to switch it on);
    the _env_ calls must follow the buffer of the last step"""
    NC.case_with_the_env(emu_library, overlap=overlap)


@TASKS
def test_state_dict_round_trip(emu_library, task):
    NC.case_state_dict_round_trip(emu_library, task)


@TASKS
def test_write_and_configure(emu_library, task):
    NC.case_write_and_configure(emu_library, task)


@TASKS
def test_invalid_calls(emu_library, task):
    NC.case_invalid_calls(emu_library, task)
