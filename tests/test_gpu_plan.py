"""Device tier of the plan model (tests/plan_cases.py): the bodies of pmg_k_plan, pmg_k_plan_reach and pmg_k_plan_count +
pmg_k_plan_scatter on gfx950 through pmgd_plan (gpu_probe/pmg_gpu_probe.hip: the product's flags, the grids of pmg_launch_plan), every
word of the schedule buffer against the model, at every size from 1 env to 65 792 -- a ragged last wavefront, a ragged last workgroup,
the single-workgroup limit and one env past it.  tests/test_plan_emulated.py is the CPU twin."""
import ctypes as C
import os

import pytest

import plan_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def plan(built):
    return C.CDLL(os.path.join(ROOT, 'gpu_probe', 'libpmg_gpu_probe.so')).pmgd_plan


@pytest.mark.parametrize('family,N', PC.CASES, ids=[PC.case_id(fn) for fn in PC.CASES])
def test_plan_writes_the_models_schedule_on_the_device(plan, family, N):
    PC.check(plan, family, N, 'gpu')


@pytest.mark.parametrize('N', [65, 4097, 16385])
def test_derived_threshold_over_three_plans_on_the_device(plan, N):
    PC.check_lpt_sequence(plan, N, 'gpu')


def test_probe_refuses_what_it_cannot_run(plan):
    PC.check_refusals(plan)
