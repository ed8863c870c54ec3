"""env.actor (pybullet_multigoal_gym_amd/actor.py) over the emulator build of the C ABI, its argument errors, the bindings, and the
numpy model of tests/actor_cases.py on its own: fmaf against libm, the pinned draws and their statistics."""
import ctypes as C

import actor_cases as AC
from pybullet_multigoal_gym_amd._lib import PmgExplore, PmgLibrary, PmgMlp


def test_abi_symbols_and_struct_sizes():
    for name in ('pmg_mlp_forward_device', 'pmg_act_env_device'):
        assert name in PmgLibrary.SYMBOLS
    assert C.sizeof(PmgMlp) == 96 and C.sizeof(PmgExplore) == 32      # as sizeof() in include/pmg.h on LP64


def test_model_fmaf_is_libm():
    AC.test_model_fmaf_is_libm()


def test_model_pinned_draws():
    AC.test_model_pinned_draws()


def test_model_statistics():
    AC.test_model_statistics()


def test_env_actor_equals_the_model(emu_library):
    AC.case_host_face(emu_library)
