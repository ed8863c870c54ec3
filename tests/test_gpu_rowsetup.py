"""Device tier of the reach row set-up at function level: pmg::reach_rowspace_setup<0, 8> on the gfx950 builds of gpu_probe/ against
float64 (tests/rowsetup_cases.py: cases, reference, derived bounds; tests/test_rowsetup_emulated.py is the CPU twin).
libpmg_gpu_probe.so carries the matrix-pipe set-up that ships (PMG_ROWSPACE_MFMA=1), libpmg_gpu_probe_valu.so the VALU build it
replaced: one bound for both."""
import ctypes as C
import os

import numpy as np
import pytest

import rowsetup_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _lib(built, name, mfma):
    lib = C.CDLL(os.path.join(ROOT, 'gpu_probe', name))
    assert lib.pmgd_rowspace_mfma() == mfma
    return lib


def test_matrix_pipe_set_up_meets_the_float64_bounds_on_the_device(built, capsys):
    with capsys.disabled():
        got = RC.check(_lib(built, 'libpmg_gpu_probe.so', 1).pmgd_rowsetup, 'gpu mfma=1', dof_equals_published=True)
    assert np.isfinite(got['coef']).all()


def test_valu_set_up_meets_the_same_bounds_on_the_device(built, capsys):
    with capsys.disabled():
        RC.check(_lib(built, 'libpmg_gpu_probe_valu.so', 0).pmgd_rowsetup, 'gpu mfma=0')
