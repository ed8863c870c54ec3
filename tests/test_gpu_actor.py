"""The actor on the MI355X: the cases of tests/actor_cases.py on libpmg_hip.so (pmg_k_mlp as gfx950 code, its matrix step the
f32-input MFMA), through the C ABI.  The exact-integer case names a wrong lane map by the integer it returns."""
import pytest

import actor_cases as AC

pytestmark = pytest.mark.gpu

TASKS = pytest.mark.parametrize('task', AC.TASK_NAMES)


@pytest.mark.parametrize('k', AC.KS)
def test_one_layer(hip_library, k):
    AC.case_one_layer(hip_library, (k,))


def test_batches_and_strides(hip_library):
    AC.case_batches_and_strides(hip_library)


def test_deep_networks(hip_library):
    AC.case_deep(hip_library)


def test_exact_integers_and_subnormals(hip_library):
    AC.case_exact_integers(hip_library)


@TASKS
def test_act(hip_library, task):
    AC.case_act(hip_library, task)


def test_handle_untouched(hip_library):
    AC.case_handle_untouched(hip_library)


@pytest.mark.parametrize('overlap', [False, True])
def test_with_the_env(hip_library, overlap):
    AC.case_with_the_env(hip_library, overlap)


def test_invalid_calls(hip_library):
    AC.case_invalid_calls(hip_library)
