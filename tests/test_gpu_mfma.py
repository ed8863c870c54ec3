"""Device tier of the matrix-pipe primitive: wv::mfma_32x32x2 of the shipped header, i.e. v_mfma_f32_32x32x2_f32 on the gfx950 build
of gpu_probe/, against the numpy model of tests/mfma_cases.py -- the operand and result lane maps, the k order and the exact-f32
claim, bit for bit (tests/test_mfma_emulated.py holds the header's emulator branch to the same model)."""
import ctypes as C
import os

import pytest

import mfma_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu_mfma(built):
    return C.CDLL(os.path.join(ROOT, 'gpu_probe', 'libpmg_gpu_probe.so')).pmgd_mfma


@pytest.mark.parametrize('name', list(MC.SETS))
def test_device_mfma_matches_the_fmaf_chain_bit_for_bit(gpu_mfma, name, capsys):
    with capsys.disabled():
        MC.check(gpu_mfma, name)
