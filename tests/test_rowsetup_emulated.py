"""CPU tier of the reach row set-up at function level: pmg::reach_rowspace_setup<0, 8> on the fiber emulator against float64
(tests/rowsetup_cases.py: cases, reference, derived bounds).  Both builds of the set-up -- the matrix-pipe products
(PMG_ROWSPACE_MFMA=1, the default; wv::mfma_32x32x2 through its emulator branch) and the VALU build (=0) -- must meet the same
bounds, and in the matrix-pipe build the DoF lanes' coefficients are, bit for bit, the responses the row lanes publish."""
import ctypes as C
import os
import subprocess

import pytest

import rowsetup_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emu_valu(built, tmp_path_factory):
    """the emulator build of the product sources with the VALU row set-up (conftest.emu_library_small_rowspace's recipe)"""
    out = str(tmp_path_factory.mktemp('emu') / 'libpmg_emu_valu.so')
    emu, src = os.path.join(ROOT, 'tests', 'emu'), os.path.join(ROOT, 'pybullet_multigoal_gym_amd', 'csrc')
    subprocess.check_call(['g++', '-O2', '-fPIC', '-std=c++17', '-I' + emu, '-I' + src, '-Wno-unknown-pragmas', '-DPMG_ROWSPACE_MFMA=0',
                           '-shared', '-o', out, os.path.join(emu, 'hip_emu.cpp'), os.path.join(emu, 'pmg_probe.cpp'),
                           os.path.join(src, 'pmg_api.cpp'), '-x', 'c++', os.path.join(src, 'pmg_kernels.hip'), '-lrt'])
    return C.CDLL(out)


def test_case_set_has_every_contact_count_and_scene():
    cs = RC.cases()
    assert sorted(set(cs['nc'].tolist())) == [1, 4, 5, 8] and len(cs['name']) == 2 * len(RC.SCENES)
    assert all(any(n.startswith(s) for n in cs['name']) for s in RC.SCENES)


def test_matrix_pipe_set_up_meets_the_float64_bounds_on_the_emulator(emu_library, capsys):
    lib = C.CDLL(emu_library.path)
    assert lib.pmge_rowspace_mfma() == 1
    with capsys.disabled():
        RC.check(lib.pmge_rowsetup, 'emu mfma=1', dof_equals_published=True)


def test_valu_set_up_meets_the_same_bounds_on_the_emulator(emu_valu, capsys):
    assert emu_valu.pmge_rowspace_mfma() == 0
    with capsys.disabled():
        RC.check(emu_valu.pmge_rowsetup, 'emu mfma=0')
