"""Emulated twin of tests/test_gpu_schedule.py (tests/schedule_cases.py): the product's kernels on the CPU emulator, at the sizes and
for the families it runs in seconds."""
import pytest

import schedule_cases as SC


@pytest.mark.parametrize('family', ['reach', 'push'])
def test_emulated_envs_step_does_not_depend_on_its_batch(emu_library, family):
    SC.check_batch_composition(family, library=emu_library, warm=0, N=7, planted=(5,), near=(3,))


def test_emulated_every_env_of_a_reach_batch_through_the_redo_pass(emu_library):
    SC.check_redo_saturation_reach(library=emu_library, N=5)
