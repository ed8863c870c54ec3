"""One substep of every step kernel against the float64 oracle, on the device: gpu_probe/libpmg_hip_substep.so is the
product's own sources, flags and link line with -DPMG_RUN_SIM_STEPS=1 -DPMG_RUN_SUBSTEPS=1 (one substep() per env step).
Cases, bars and checks are those of the CPU tier (tests/substep_cases.py, tests/test_substep_emulated.py): per task and column
group max(1e-6, 4 x the worst distance of the float32 oracle from the float64 oracle on the same cases), computed from the
two oracle builds, never from the device."""
import os

import pytest

import pybullet_multigoal_gym_amd as pmg
import substep_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip_library_one_substep(built):
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    return PmgLibrary(os.path.join(ROOT, 'gpu_probe', 'libpmg_hip_substep.so'))


@pytest.mark.parametrize('packed', [1, 0])
@pytest.mark.parametrize('name', list(SC.TASKS) + SC.AWAY)
def test_one_substep_matches_the_float64_oracle(hip_library_one_substep, name, packed, capsys):
    with capsys.disabled():
        SC.check_task(pmg, hip_library_one_substep, name, packed)


@pytest.mark.parametrize('name', ['reach', 'push', 'pick_and_place'])
def test_a_case_gives_the_same_bits_in_every_row(hip_library_one_substep, name, capsys):
    with capsys.disabled():
        SC.check_row_independence(pmg, hip_library_one_substep, name)


@pytest.mark.parametrize('name', ['push/away', 'slide/away', 'block_rearrange5/away', 'chest_push5/away'])
def test_redone_envs_equal_the_full_store_kernel(hip_library_one_substep, name, capsys):
    with capsys.disabled():
        SC.check_redo_equals_full_store(pmg, hip_library_one_substep, name)


def test_two_wavefront_reach_kernel_equals_the_one_wavefront_kernel_after_one_substep(hip_library_one_substep, capsys):
    with capsys.disabled():
        SC.check_two_wavefront_reach(pmg, hip_library_one_substep)
