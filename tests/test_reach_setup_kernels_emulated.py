"""CPU tier of the kernel-level cases of tests/rowsetup_pipelined_cases.py on the fiber emulator: pmg_k_step_reach2, pmg_k_step_reach
and pmg_k_redo with PMG_ROWSETUP_PIPELINE on (tests/emu/libpmg_emu.so) on the four pressed states, one env step -- bit-equal to each
other, and each bit-equal to the same kernel of an emulator build with -DPMG_ROWSETUP_PIPELINE=0.  And the two-wavefront kernel
under both wavefront orders (pmge_set_wave_order, as tests/test_wave_order.py): the switch moves LDS reads of the contact store to
the front of the set-up, behind barrier B, where the helper wavefront has handed the contacts over -- a read that slipped in front
of a hand-over would show as a difference between the orders.  tests/test_gpu_reach_setup_kernels.py is the device twin."""
import ctypes as C
import os

import numpy as np
import pytest

import pybullet_multigoal_gym_amd as pmg
import reach_mfma_cases as KC
import rowsetup_pipelined_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emu_off(built, tmp_path_factory):
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    return PmgLibrary(PC.emu_library_switch_off(ROOT, tmp_path_factory))


def test_reach_kernels_give_the_bits_of_the_switch_off_library_on_the_emulator(emu_library, emu_off, capsys):
    assert (C.CDLL(emu_library.path).pmg_rowsetup_pipeline(), C.CDLL(emu_off.path).pmg_rowsetup_pipeline()) == (1, 0)
    with capsys.disabled():
        PC.check_kernels_bit_equal(pmg, emu_library, emu_off, 'emu')


def test_two_wavefront_kernel_with_the_pipelined_set_up_is_bit_equal_under_both_wavefront_orders(emu_library):
    """pmg_k_step_reach2 on the four pressed envs (one env per workgroup, the helper wavefront colliding): the default scheduler, the
    list 01 and the list 10 give the same bits"""
    lib = C.CDLL(emu_library.path)
    lib.pmge_wave_order_launches.restype = C.c_longlong
    assert lib.pmg_rowsetup_pipeline() == 1
    low = PC.scenes(False)

    def run(order):
        arr = (C.c_int * max(len(order), 1))(*order)
        lib.pmge_set_wave_order(arr, C.c_int(len(order)))
        try:
            before = int(lib.pmge_wave_order_launches())
            got = KC.step(pmg, emu_library, low, PC.ACT_LOW, {'PMG_REACH_TWO_WAVES': '1'})
            assert (int(lib.pmge_wave_order_launches()) > before) == bool(order), order
            return got
        finally:
            lib.pmge_set_wave_order((C.c_int * 1)(0), C.c_int(0))
    base = run(())
    assert np.array_equal(base['prone'], np.arange(PC.N_ENVS)) and (base['nc'] == 8).all(), (base['prone'], base['nc'])
    for order in ((0, 1), (1, 0)):
        KC._same_bits(run(order), base, 'wavefront order %s against the default scheduler' % (order,))
