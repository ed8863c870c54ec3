"""CPU tier of the matrix-pipe primitive: the PMG_EMULATE branch of wv::mfma_32x32x2 in the SHIPPED header (csrc/pmg_wave.h; it goes
through the emulator's exchange buffer and wave barrier) against the numpy model of tests/mfma_cases.py, bit for bit."""
import ctypes as C

import pytest

import mfma_cases as MC
from mfma_cases import test_the_model_tells_the_k_order_and_the_row_map_apart  # noqa: F401


@pytest.fixture(scope='module')
def emu_mfma(emu_library):
    return C.CDLL(emu_library.path).pmge_mfma


@pytest.mark.parametrize('name', list(MC.SETS))
def test_emulated_mfma_matches_the_fmaf_chain_bit_for_bit(emu_mfma, name, capsys):
    with capsys.disabled():
        MC.check(emu_mfma, name)


def test_probe_refuses_chains_and_batches_beyond_its_buffers(emu_mfma):
    z = C.c_void_p(0)
    assert emu_mfma(C.c_int(0), C.c_int(1), z, z, z, z) == -1 and emu_mfma(C.c_int(1), C.c_int(9), z, z, z, z) == -1
