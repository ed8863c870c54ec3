"""Device tier of the kernel-level cases of tests/reach_mfma_cases.py: pmg_k_step_reach, pmg_k_step_reach2 and pmg_k_redo with the
row set-up on the matrix pipe, eight envs, one env step -- bit-equal to each other after the full step (libpmg_hip.so) and after
one substep (gpu_probe/libpmg_hip_substep.so), and within the existing bars of the float64 oracle.  tests/test_reach_mfma_emulated.py
is the CPU twin."""
import os

import pytest

import pybullet_multigoal_gym_amd as pmg
import reach_mfma_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_reach_kernels_agree_and_match_the_oracle_after_the_full_step(hip_library, capsys):
    with capsys.disabled():
        runs = KC.check_kernels_agree(pmg, hip_library)
        KC.check_full_step_against_oracle(runs)


def test_reach_kernels_agree_and_match_the_oracle_after_one_substep(built, capsys):
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    lib = PmgLibrary(os.path.join(ROOT, 'gpu_probe', 'libpmg_hip_substep.so'))
    with capsys.disabled():
        KC.check_kernels_agree(pmg, lib)
        KC.check_one_substep_against_oracle(pmg, lib)
