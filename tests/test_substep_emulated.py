"""One substep of every step kernel against the float64 oracle, CPU tier: the product's sources on the emulator, built to run
ONE substep() per env step (-DPMG_RUN_SIM_STEPS=1 -DPMG_RUN_SUBSTEPS=1).  After one substep there is no contact chaos, so the
bars are exact ones: per task and column group max(1e-6, 4 x the worst distance of the float32 oracle from the float64
oracle on the same cases), computed here from the two oracle builds (tests/substep_cases.py has the cases and the checks; the
same ones run on the device in tests/test_gpu_substep.py).

Measured on the emulator (worst distance of a kept case / the float32 oracle's own worst distance, both PMG_PACKED settings
alike; the table of DESIGN.md section 5.2 has the distances): joint qd 0.8 ... 3.2, block linear velocity 0.02 ... 2.3,
angular velocity 0.14 ... 2.0, door qd 0.02 ... 1.1; no case left out, by the emulator or by the float32 oracle; every contact
count equal to the oracle's."""
import os
import subprocess

import pytest

import pybullet_multigoal_gym_amd as pmg
import substep_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emu_library_one_substep(built, tmp_path_factory):
    """The emulator build of the product sources that runs one substep per env step."""
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    out = str(tmp_path_factory.mktemp('emu') / 'libpmg_emu_substep.so')
    emu = os.path.join(ROOT, 'tests', 'emu')
    src = os.path.join(ROOT, 'pybullet_multigoal_gym_amd', 'csrc')
    subprocess.check_call(['g++', '-O2', '-fPIC', '-std=c++17', '-I' + emu, '-I' + src, '-Wno-unknown-pragmas', '-w', '-DPMG_RUN_SIM_STEPS=1',
                           '-DPMG_RUN_SUBSTEPS=1', '-shared', '-o', out, os.path.join(emu, 'hip_emu.cpp'), os.path.join(emu, 'pmg_probe.cpp'),
                           os.path.join(src, 'pmg_api.cpp'), '-x', 'c++', os.path.join(src, 'pmg_kernels.hip'), '-lrt'])
    return PmgLibrary(out)


def test_the_substep_switches_of_the_oracle_bound_loops_only(built):
    """sim_steps x substeps = 5 x 20 one-substep steps are one ordinary env step, to the bit (the joint damping is latched
    per stepSimulation, so the 100 are run as 5 steps of 20); `elapsed` counts env steps, not substeps"""
    import numpy as np
    import oracle_lib as O
    a = np.zeros((4, 7), np.float32)
    whole = O.OracleEnv('push', 4, seed_base=5, seed_stride=1, joint_control=True)
    parts = O.SubstepOracle('push', 4, substeps=20, seed_base=5, seed_stride=1, joint_control=True)
    for o in (whole, parts):
        o.reset(), o.reset()
    st = whole.get_state().copy()
    st[:, 21:28] += np.float32(0.02)
    whole.set_state(st), parts.set_state(st)
    whole.step(a)
    for _ in range(5):
        parts.step(a)
    sw, sp = whole.get_state(), parts.get_state()
    assert sw[0, 29] == 1 and sp[0, 29] == 5
    sp[:, 29] = sw[:, 29]
    assert np.array_equal(sw, sp)
    assert O.get_prior('substeps') == 20 and O.get_prior('sim_steps') == 5        # back at their defaults
    info = parts.last_substep()
    assert (info['nc'] >= 4).all() and (info['iterations'] >= 1).all() and (info['iterations'] <= 5).all()
    assert ((info['a'][:, 0] == 0) & (info['b'][:, 0] == -1)).all()               # object x table first


@pytest.mark.parametrize('name', list(SC.TASKS) + SC.AWAY)
def test_case_set_is_clear_of_knife_edges(built, name, capsys):
    with capsys.disabled():
        SC.check_case_set(name)


@pytest.mark.parametrize('mutant', list(SC.MUTANTS))
@pytest.mark.parametrize('name', list(SC.TASKS) + SC.AWAY)
def test_harness_catches_a_wrong_solver(built, name, mutant, capsys):
    with capsys.disabled():
        SC.check_mutant(name, mutant)


@pytest.mark.parametrize('packed', [1, 0])
@pytest.mark.parametrize('name', list(SC.TASKS) + SC.AWAY)
def test_one_substep_matches_the_float64_oracle(emu_library_one_substep, name, packed, capsys):
    with capsys.disabled():
        SC.check_task(pmg, emu_library_one_substep, name, packed)


@pytest.mark.parametrize('name', ['reach', 'push', 'pick_and_place'])
def test_a_case_gives_the_same_bits_in_every_row(emu_library_one_substep, name, capsys):
    with capsys.disabled():
        SC.check_row_independence(pmg, emu_library_one_substep, name)


@pytest.mark.parametrize('name', ['push/away', 'slide/away', 'block_rearrange5/away', 'chest_push5/away'])
def test_redone_envs_equal_the_full_store_kernel(emu_library_one_substep, name, capsys):
    with capsys.disabled():
        SC.check_redo_equals_full_store(pmg, emu_library_one_substep, name)


def test_two_wavefront_reach_kernel_equals_the_one_wavefront_kernel_after_one_substep(emu_library_one_substep, capsys):
    with capsys.disabled():
        SC.check_two_wavefront_reach(pmg, emu_library_one_substep)
