"""The actor on the CPU tier: the cases of tests/actor_cases.py on the g++ build of the product sources (pmg_k_mlp with the fmaf
body of its matrix step, pmg_mlp_forward_device, pmg_act_env_device) over the fiber emulator, through the C ABI.  The emulator
proves the tiling, the padding and the epilogue; the lane maps of the MFMA are proven by tests/test_gpu_actor.py."""
import pytest

import actor_cases as AC

TASKS = pytest.mark.parametrize('task', AC.TASK_NAMES)


@pytest.mark.parametrize('k', AC.KS)
def test_one_layer(emu_library, k):
    AC.case_one_layer(emu_library, (k,))


def test_batches_and_strides(emu_library):
    AC.case_batches_and_strides(emu_library)


def test_deep_networks(emu_library):
    AC.case_deep(emu_library)


def test_exact_integers_and_subnormals(emu_library):
    AC.case_exact_integers(emu_library)


@TASKS
def test_act(emu_library, task):
    AC.case_act(emu_library, task)


def test_handle_untouched(emu_library):
    AC.case_handle_untouched(emu_library)


@pytest.mark.parametrize('overlap', [False, True])
def test_with_the_env(emu_library, overlap):
    AC.case_with_the_env(emu_library, overlap)


def test_invalid_calls(emu_library):
    AC.case_invalid_calls(emu_library)
