"""Device tier of PMG_IK_LEAN at primitive and function level (tests/ik_lean_cases.py), on the gfx950 probe builds of gpu_probe/:
affine_shr, half_gram6 and half_max of the shipped pmg_wave.h -- the hand-written DPP blocks and the plain C++ branches -- against
their numpy models, every lane of all four rows; ik_solve (32 cases, both layouts) and fk (16 poses, both layouts) of
libpmg_gpu_probe.so (the switch on, as shipped) bit-equal to libpmg_gpu_probe_iklean0.so (-DPMG_IK_LEAN=0), and ik_solve within
tests/device_cases.py's bar of the float64 oracle.  tests/test_ik_lean_emulated.py is the CPU twin."""
import ctypes as C
import os

import pytest

import ik_lean_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def libs(built):
    on, off, plain = [C.CDLL(os.path.join(ROOT, 'gpu_probe', n)) for n in ('libpmg_gpu_probe.so', 'libpmg_gpu_probe_iklean0.so', 'libpmg_gpu_probe_plain.so')]
    assert (on.pmgd_ik_lean(), off.pmgd_ik_lean(), plain.pmgd_ik_lean()) == (1, 0, 1) and (on.pmgd_variant(), off.pmgd_variant(), plain.pmgd_variant()) == (0, 0, 1)
    return on, off, plain


def test_lean_primitives_give_their_models_bits_on_the_device(libs, capsys):
    with capsys.disabled():
        for lib, label in zip(libs, ('gpu', 'gpu, switch-off build', 'gpu, plain C++ branches')):
            LC.check_primitives(lib.pmgd_lean_prim, True, label)


def test_ik_solve_gives_the_bits_of_the_switch_off_build_on_the_device(libs, capsys):
    with capsys.disabled():
        LC.check_ik(libs[0].pmgd_ik, libs[1].pmgd_ik, 'gpu')


def test_fk_gives_the_bits_of_the_switch_off_build_on_the_device(libs, capsys):
    with capsys.disabled():
        LC.check_fk(libs[0].pmgd_fk, libs[1].pmgd_fk, 'gpu')
