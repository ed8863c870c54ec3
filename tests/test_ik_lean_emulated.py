"""CPU tier of PMG_IK_LEAN at primitive and function level, on the fiber emulator (tests/ik_lean_cases.py): the emulator branches of
affine_shr, half_gram6 and half_max against their numpy models, every lane of all four rows; ik_solve (32 cases, both layouts) and
fk (16 poses, both layouts) of tests/emu/libpmg_emu.so (the switch on) bit-equal to an emulator build with -DPMG_IK_LEAN=0, and
ik_solve within tests/device_cases.py's bar of the float64 oracle.  tests/test_gpu_ik_lean.py is the device twin."""
import ctypes as C
import os

import pytest

import ik_lean_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def libs(built, tmp_path_factory):
    on = C.CDLL(os.path.join(ROOT, 'tests', 'emu', 'libpmg_emu.so'))
    off = C.CDLL(LC.emu_library_switch_off(ROOT, tmp_path_factory))
    assert (on.pmge_ik_lean(), off.pmge_ik_lean(), on.pmg_ik_lean(), off.pmg_ik_lean()) == (1, 0, 1, 0)
    return on, off


def test_fma32_of_the_models_rounds_once():
    import numpy as np
    f = np.float32
    assert LC.fma32(f(1 + 2 ** -23), f(1 + 2 ** -23), f(-1)) == f(2 ** -22 + 2 ** -46)             # the product's low bits survive
    # 3 (1 + 2^-23) lies half way between 3 + 2^-22 and 3 + 2^-21: a tie goes to even, an addend far below the float64 sum's last bit decides
    assert LC.fma32(f(3), f(1 + 2 ** -23), f(0)) == f(3 + 2 ** -21)
    assert LC.fma32(f(3), f(1 + 2 ** -23), f(-2 ** -60)) == f(3 + 2 ** -22) and LC.fma32(f(3), f(1 + 2 ** -23), f(2 ** -60)) == f(3 + 2 ** -21)
    assert LC.fma32(f(3), f(0), f(-0.0)).view(np.uint32) == 0 and LC.fma32(f(-3), f(0), f(-0.0)).view(np.uint32) == 0x80000000


def test_lean_primitives_give_their_models_bits_on_the_emulator(libs, capsys):
    with capsys.disabled():
        for lib in libs:                                    # (the primitives do not depend on the switch: both builds hold them)
            LC.check_primitives(lib.pmge_lean_prim, False, 'emu')


def test_ik_solve_gives_the_bits_of_the_switch_off_build_on_the_emulator(libs, capsys):
    with capsys.disabled():
        LC.check_ik(libs[0].pmge_ik, libs[1].pmge_ik, 'emu')


def test_fk_gives_the_bits_of_the_switch_off_build_on_the_emulator(libs, capsys):
    with capsys.disabled():
        LC.check_fk(libs[0].pmge_fk, libs[1].pmge_fk, 'emu')
