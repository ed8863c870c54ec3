"""Emulated tier of the plan model (tests/plan_cases.py): plan_all, plan_all<true> and plan_count + plan_scatter of csrc/pmg_kernels.h
on the CPU emulator through pmge_plan (tests/emu/pmg_probe.cpp), every word of the schedule buffer against the model.  The sizes up
to 4097 envs, and 16 384 (sixteen chunks: every class bit of the single-workgroup plan in use) once for reach; tests/test_gpu_plan.py
runs every case on the device."""
import ctypes as C
import os

import pytest

import plan_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMULATED = [fn for fn in PC.CASES if fn[1] <= PC.EMULATED_MAX or fn == ('reach', 16384)]


@pytest.fixture(scope='module')
def plan(built):
    return C.CDLL(os.path.join(ROOT, 'tests', 'emu', 'libpmg_emu.so')).pmge_plan


@pytest.mark.parametrize('family,N', EMULATED, ids=[PC.case_id(fn) for fn in EMULATED])
def test_emulated_plan_writes_the_models_schedule(plan, family, N):
    PC.check(plan, family, N, 'emu')


@pytest.mark.parametrize('N', [65, 4097])
def test_emulated_derived_threshold_over_three_plans(plan, N):
    PC.check_lpt_sequence(plan, N, 'emu')


def test_emulated_probe_refuses_what_it_cannot_run(plan):
    PC.check_refusals(plan)
