"""env.her (pybullet_multigoal_gym_amd/her.py) over the emulator build of the C ABI, its argument errors, the bindings, and
the statistics of the draw specification on the numpy model alone (tests/her_cases.py)."""
import ctypes as C

import her_cases as HC
from pybullet_multigoal_gym_amd._lib import PmgHerBatch, PmgHerSource, PmgLibrary


def test_abi_symbols_and_struct_sizes():
    for name in ('pmg_her_sample_device', 'pmg_device_copy'):
        assert name in PmgLibrary.SYMBOLS
    assert C.sizeof(PmgHerSource) == 64 and C.sizeof(PmgHerBatch) == 88      # as sizeof() in include/pmg.h on LP64


def test_model_pinned_vector():
    HC.test_model_pinned_vector()


def test_model_statistics():
    HC.test_model_statistics()


def test_env_her_sample_equals_the_pointer_call(emu_library):
    HC.case_host_face(emu_library)
