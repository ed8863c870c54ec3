"""CPU tier of PMG_IK_LEAN at kernel level, on the fiber emulator (tests/ik_lean_cases.py): one env step of pmg_k_step_reach2,
pmg_k_step_reach and pmg_k_redo on four pressed and four hovering envs, of the packed reach list on 13 envs (a ragged last wavefront)
and of push on 8 envs -- states, observations, goals and rewards of tests/emu/libpmg_emu.so (the switch on) bit-equal to those of an
emulator build with -DPMG_IK_LEAN=0.  tests/test_gpu_ik_lean_kernels.py is the device twin."""
import ctypes as C
import os

import pybullet_multigoal_gym_amd as pmg
import ik_lean_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_kernels_give_the_bits_of_the_switch_off_library_on_the_emulator(emu_library, tmp_path_factory, capsys):
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    off = PmgLibrary(LC.emu_library_switch_off(ROOT, tmp_path_factory))
    assert (C.CDLL(emu_library.path).pmg_ik_lean(), C.CDLL(off.path).pmg_ik_lean()) == (1, 0)
    with capsys.disabled():
        LC.check_kernels(pmg, emu_library, off, 'emu')
