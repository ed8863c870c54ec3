"""CPU tier of the kernel-level cases of tests/reach_mfma_cases.py: the three reach kernels with the row set-up on the matrix pipe
(wv::mfma_32x32x2 through its emulator branch), on the fiber emulator -- bit-equal to each other after one substep and after the
full step, within the existing bars of the float64 oracle, and the two-wavefront kernel bit-equal under both wavefront orders
on a pressed env (the coupling table goes through the row store, which is wavefront 0's between barrier B and the next barrier A:
a helper that touched it there would show as a difference between the orders)."""
import numpy as np
import pytest

import pybullet_multigoal_gym_amd as pmg
import reach_mfma_cases as KC
from test_substep_emulated import emu_library_one_substep  # noqa: F401  (the fixture: the emulator's one-substep build)
from test_wave_order import PAIR, _rollout, _under_orders, waves  # noqa: F401


def test_reach_kernels_agree_and_match_the_oracle_after_the_full_step(emu_library, capsys):
    with capsys.disabled():
        runs = KC.check_kernels_agree(pmg, emu_library)
        KC.check_full_step_against_oracle(runs)


def test_reach_kernels_agree_and_match_the_oracle_after_one_substep(emu_library_one_substep, capsys):
    with capsys.disabled():
        KC.check_kernels_agree(pmg, emu_library_one_substep)
        KC.check_one_substep_against_oracle(pmg, emu_library_one_substep)


def test_two_wavefront_reach_kernel_on_a_pressed_env_is_bit_equal_under_both_orders(emu_library, waves):
    """pmg_k_step_reach2, two envs pressed flat on the table (eight contacts: the full 24 x 24 table) and one hovering"""
    st = KC.scenes(False)[[0, 7, 2]]
    act = KC.ACT_LOW[[0, 7, 2]]
    base = _under_orders(waves, PAIR, lambda: _rollout(emu_library, 'reach', 3, {'max_episode_steps': 1000}, st, [act], [(2, 1, 0)]))
    assert (base['0 observation'][[0, 2], 2] > 0.17).all() and np.isfinite(base['state']).all()
