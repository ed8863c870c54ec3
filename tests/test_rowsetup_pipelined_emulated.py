"""CPU tier of the pipelined front of the reach row set-up (PMG_ROWSETUP_PIPELINE, csrc/pmg_step_body.inc) at function level:
pmg::reach_rowspace_setup<0, 8> on the fiber emulator, the build with the switch on (the default, tests/emu/libpmg_emu.so) against a
build with -DPMG_ROWSETUP_PIPELINE=0 -- the same bits in every lane on the thirteen cases of tests/rowsetup_pipelined_cases.py
(contact counts 0, 1, 4, 5, 8, finger 2 only, tilted normals).  tests/test_gpu_rowsetup_pipelined.py is the device twin."""
import ctypes as C
import os

import rowsetup_pipelined_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_set_adds_the_empty_list_to_every_scene():
    names, cs = PC.cases()
    assert sorted(set(cs['nc'].tolist())) == [0, 1, 4, 5, 8] and len(names) == 13 and int(cs['nc'][-1]) == 0
    assert (cs['con'][-1] == 0).all() and (cs['mu'][-1] == 0).all()


def test_pipelined_set_up_gives_the_bits_of_the_switch_off_build_on_the_emulator(emu_library, tmp_path_factory, capsys):
    on, off = C.CDLL(emu_library.path), C.CDLL(PC.emu_library_switch_off(ROOT, tmp_path_factory))
    assert (on.pmge_rowsetup_pipeline(), off.pmge_rowsetup_pipeline()) == (1, 0)
    assert (on.pmge_rowspace_mfma(), off.pmge_rowspace_mfma()) == (1, 1)
    with capsys.disabled():
        PC.check_set_up_bit_equal(on.pmge_rowsetup, off.pmge_rowsetup, 'emu')
