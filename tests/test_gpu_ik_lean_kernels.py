"""Device tier of PMG_IK_LEAN at kernel level (tests/ik_lean_cases.py): one env step of pmg_k_step_reach2, pmg_k_step_reach and
pmg_k_redo on four pressed and four hovering envs, of the packed reach list on 13 envs (a ragged last wavefront) and of push on 8
envs -- states, observations, goals and rewards of libpmg_hip.so (the switch on, as shipped) bit-equal to those of
gpu_probe/libpmg_hip_iklean0.so (the product's sources, flags and link line with -DPMG_IK_LEAN=0).
tests/test_ik_lean_kernels_emulated.py is the CPU twin."""
import ctypes as C
import os

import pytest

import pybullet_multigoal_gym_amd as pmg
import ik_lean_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_step_kernels_give_the_bits_of_the_switch_off_library_on_the_device(hip_library, capsys):
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    off_path = os.path.join(ROOT, 'gpu_probe', 'libpmg_hip_iklean0.so')
    assert (C.CDLL(hip_library.path).pmg_ik_lean(), C.CDLL(off_path).pmg_ik_lean()) == (1, 0)
    with capsys.disabled():
        LC.check_kernels(pmg, hip_library, PmgLibrary(off_path), 'gpu')
