"""TD3's target on the CPU tier: the cases of tests/td3_cases.py on the g++ build of the product sources (pmg_k_td3_target with the fmaf body
of the matrix step) over the fiber emulator, through the C ABI.  The emulator proves the hand-over with the noise in it, the restore of
x' | a~ between the critics from d_next_action and from the workspace, the padding, the min and the epilogue; the lane maps of the MFMA and
the build's logf / sqrtf / cosf are proven by tests/test_gpu_td3.py."""
import pytest

import td3_cases as T3


@pytest.mark.parametrize('pair', T3.PAIRS)
@pytest.mark.parametrize('hidden', T3.HIDDEN)
def test_one_critic_without_noise_is_td_target(emu_library, hidden, pair):
    T3.case_degenerate(emu_library, hidden, (pair,))


def test_twin_critics_without_noise(emu_library):
    T3.case_twin(emu_library)


def test_smoothing(emu_library):
    T3.case_smoothing(emu_library)


def test_stale_tile_contents(emu_library):
    T3.case_stale_tile(emu_library)


def test_epilogue(emu_library):
    T3.case_epilogue(emu_library)


def test_invalid_calls(emu_library):
    T3.case_invalid_calls(emu_library)
