"""env.critic (pybullet_multigoal_gym_amd/critic.py) over the emulator build of the C ABI: load errors, q and td_target round trips
against the numpy model of tests/td_cases.py, close(); and the bindings."""
import ctypes as C

import td_cases as TC
from pybullet_multigoal_gym_amd._lib import PmgLibrary, PmgTdTarget


def test_abi_symbols_and_struct_size():
    for name in ('pmg_q_device', 'pmg_td_target_device'):
        assert name in PmgLibrary.SYMBOLS
    assert C.sizeof(PmgTdTarget) == 88                                 # as sizeof(pmg_td_target) in include/pmg.h on LP64


def test_env_critic_equals_the_model(emu_library):
    TC.case_host_face(emu_library)
