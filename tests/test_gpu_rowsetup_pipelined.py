"""Device tier of the pipelined front of the reach row set-up (PMG_ROWSETUP_PIPELINE, csrc/pmg_step_body.inc) at function level:
pmg::reach_rowspace_setup<0, 8> on the gfx950 probe builds of gpu_probe/ -- libpmg_gpu_probe.so (the switch on, as shipped) against
libpmg_gpu_probe_setup0.so (-DPMG_ROWSETUP_PIPELINE=0): the same bits in every lane on the thirteen cases of
tests/rowsetup_pipelined_cases.py (contact counts 0, 1, 4, 5, 8, finger 2 only, tilted normals).  The float64 bounds of the shipped
build are tests/test_gpu_rowsetup.py's; tests/test_rowsetup_pipelined_emulated.py is the CPU twin."""
import ctypes as C
import os

import pytest

import rowsetup_pipelined_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_pipelined_set_up_gives_the_bits_of_the_switch_off_build_on_the_device(built, capsys):
    on = C.CDLL(os.path.join(ROOT, 'gpu_probe', 'libpmg_gpu_probe.so'))
    off = C.CDLL(os.path.join(ROOT, 'gpu_probe', 'libpmg_gpu_probe_setup0.so'))
    assert (on.pmgd_rowsetup_pipeline(), off.pmgd_rowsetup_pipeline()) == (1, 0)
    assert (on.pmgd_rowspace_mfma(), off.pmgd_rowspace_mfma()) == (1, 1)
    with capsys.disabled():
        PC.check_set_up_bit_equal(on.pmgd_rowsetup, off.pmgd_rowsetup, 'gpu')
