"""The reach contact step on the device, through the product library (tests/contact_step_cases.py): the shipped schedule against
PMG_REACH_TWO_WAVES=0 and PMG_PACKED=0 bit for bit, the redo list, and the wavefront trace (PMG_WAVE_TRACE).
tests/test_contact_step_emulated.py is the CPU twin, which also runs the batch under both wavefront orders."""
import pytest

import contact_step_cases as CC
import schedule_cases as SC

pytestmark = pytest.mark.gpu


def test_the_shipped_contact_step_is_the_other_kernels_step_bit_for_bit(built):
    CC.check_shipped_schedule()


def test_every_env_given_up_comes_back_through_the_redo_pass(built):
    SC.check_redo_saturation_reach()


def test_every_live_wavefront_leaves_one_trace_record(built):
    CC.check_trace()
