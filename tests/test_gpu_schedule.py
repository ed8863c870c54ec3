"""Whole steps through the public API on the device, held to what the schedule promises (tests/schedule_cases.py): batch composition at
ragged sizes for every task family, a redo list that holds the whole batch, and the same step under either plan.
tests/test_schedule_emulated.py is the CPU twin at the sizes the emulator runs in seconds."""
import pytest

import schedule_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('family', list(SC.FAMILIES))
def test_an_envs_step_does_not_depend_on_its_batch(built, family):
    SC.check_batch_composition(family)


def test_every_env_of_a_reach_batch_through_the_redo_pass(built):
    SC.check_redo_saturation_reach()


def test_every_env_of_a_push_batch_through_the_redo_pass(built):
    from test_gpu_parity import _max_or_count
    SC.check_redo_saturation_push(_max_or_count)


def test_either_plan_gives_the_same_step(built):
    """PMG_PLAN_TWO_PASS is read once per process: two fresh child processes, one after the other, each under its own time limit."""
    SC.check_either_plan_same_step()
