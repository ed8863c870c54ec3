"""-m gpu: the slide puck tumbling in free flight, on each of the three kernels that carry it, against the float64 oracle.

The puck is the one free body whose inertia is not isotropic, so its unconstrained update has a gyroscopic term w x (I w) that
needs the body's rotation.  With the spin along or across the puck's axis -- every other slide test -- the term is zero.  Here 32
envs spin about random axes at up to 10 rad/s, fall for one env step (100 substeps) without touching anything, and the pose and the
twist of EVERY env are held to the oracle.

What this can and cannot catch.  It catches any error in the gyroscopic term, the damping or the quaternion integration of the
three kernels.  It would catch a rotation read one substep late (the list-0 kernel's wavefront 0 once read the helper wavefront's
copy with no barrier in between) IF the hardware's timing produced one on the day -- it usually does not.  That the kernels'
hand-overs are ordered at all is proven on the emulator, under permuted wavefront order (tests/test_wave_order.py), not here."""
import os

import numpy as np
import pytest

import oracle_lib
import pybullet_multigoal_gym_amd as pmg

pytestmark = pytest.mark.gpu

N = 32
# The bars of tests/test_wave_order.py's free-flight case: at least ten times the float32-state oracle's spread on the scene (asserted
# below), at most a tenth of what a rotation one substep stale costs (pose 8.6e-3, twist 6.7e-2 measured on the emulator).
POSE_BAR, TWIST_BAR = 1e-4, 1e-3


def _spins():
    rs = np.random.RandomState(7)
    w = rs.uniform(1.0, 10.0, (N, 3)) * rs.choice([-1.0, 1.0], (N, 3))     # every component at least 1 rad/s: no spin along a principal axis
    return w.astype(np.float32)


def _scene(st, placement):
    if placement == 'list0':                     # the tip target within near_r = 0.065 of the puck: the plan sends the env to list 0
        st[:, 18:21] = [-0.52, 0.0, 0.40]
        st[:, 64:67] = [-0.52, 0.06, 0.40]
    else:                                        # the tip target where the reset left it, the puck far from it: the packed list
        st[:, 64:67] = [-0.45, 0.12, 0.40]
    st[:, 67:71] = [0, 0, 0, 1]; st[:, 71:74] = 0; st[:, 74:77] = _spins()


@pytest.fixture(scope='module')
def oracle_states(built):
    """placement -> (start state, float64 oracle's state, float32-state oracle's state) after one zero-action step; computed once"""
    out = {}
    for placement in ('list0', 'packed'):
        res = []
        for cls in (oracle_lib.OracleEnv, oracle_lib.FloorOracle):
            ora = cls('slide', N, seed_base=0, seed_stride=1, threads=8)
            ora.reset(), ora.reset()
            st = ora.get_state().copy()
            _scene(st, placement)
            ora.set_state(st)
            ora.step(np.zeros((N, 3), np.float32))
            res.append(ora.get_state())
        out[placement] = (st, res[0], res[1])
        for a in out[placement]:
            a.setflags(write=False)
    return out


def _errors(s, ref):
    return float(np.abs(s[:, 64:71] - ref[:, 64:71]).max()), float(np.abs(s[:, 71:77] - ref[:, 71:77]).max())


@pytest.mark.parametrize('kernel,placement,packed', [('list 0 (three wavefronts)', 'list0', '1'), ('packed list (four envs per wavefront)', 'packed', '1'),
                                                     ('one env per wavefront (PMG_PACKED=0)', 'list0', '0')])
def test_tumbling_puck_in_free_flight_matches_the_oracle(built, oracle_states, kernel, placement, packed):
    """One zero-action step of 32 tumbling pucks on pmg_k_step_list<1, 24, 0, 1> / pmg_k_step_obj4<true> / pmg_k_step<1, 24, true>:
    the maximum over all 32 envs of the puck's pose error <= 1e-4 and twist error <= 1e-3 against the float64 oracle (measured on the
    MI355X: DESIGN.md 3.2; the float32-state oracle is printed beside it)."""
    st, s64, s32 = oracle_states[placement]
    os.environ['PMG_PACKED'] = packed
    try:
        env = pmg.make_env(task='slide', num_envs=N, seed=0, seed_stride=1)
    finally:
        del os.environ['PMG_PACKED']
    env.reset()
    env.set_state(st)
    env.step(np.zeros((N, 3), np.float32))
    sch = env.handle.schedule()
    se = env.get_state()
    env.close()
    if packed == '1':
        assert sch['prone' if placement == 'list0' else 'free'].size == N and sch['redo'].size == 0, sch      # the kernel meant is the one that ran
    assert (s64[:, 66] > 0.19).all() and (s64[:, 66] < 0.22).all()          # still falling: nothing was touched
    fp, ft = _errors(s32, s64)
    ep, et = _errors(se, s64)
    print('%s: puck pose error %.3g, twist error %.3g over %d envs (float32-state oracle: %.3g, %.3g)' % (kernel, ep, et, N, fp, ft))
    assert 10 * fp <= POSE_BAR and 10 * ft <= TWIST_BAR
    assert ep <= POSE_BAR and et <= TWIST_BAR, (kernel, ep, et)
