"""Kernel-level cases of the reach row set-up on the matrix pipe -- TEST INFRASTRUCTURE, shared by tests/test_reach_mfma_emulated.py
and tests/test_gpu_reach_mfma.py.  Eight envs, one env step: the four pressed states of tests/rowsetup_cases.py (both fingers flat
on the table), three of them again with the wrist rolled (one finger lower than the other: fewer contacts), and one hovering env.

All three reach kernels run reach_contact_pgs_rowspace, so they must give each other's bits:
  * tip target at the table (the plan's list 0): pmg_k_step_reach2 (PMG_REACH_TWO_WAVES=1) against pmg_k_step_reach (=0);
  * the same envs with the tip target 12 cm up, zero action (the plan's list 1: a misprediction the packed kernel gives up):
    pmg_k_redo (PMG_PACKED=1) against pmg_k_step_reach on every env (PMG_PACKED=0).
Against the float64 oracle: after the full step every run within the reach rollout bars of tests/test_gpu_parity.py (tip control:
observation 2e-4, state 5e-4); after ONE substep (a one-substep build), under joint control -- where the oracle and the product
start from bit-equal motor targets -- the one-wavefront kernel within the bars of tests/substep_cases.py for reach (4 x the
float32 oracle's own distance from the float64 oracle, per column group), near-exit cases left out as there; the other two
kernels are held to it through their bit-equality after one substep under tip control."""
import os
import warnings

import numpy as np

import oracle_lib as O
import rowsetup_cases as RC
import substep_cases as SC

N = 8
PRESSED = np.arange(7)
OBS_TOL, STATE_TOL = 2e-4, 5e-4          # tests/test_gpu_parity.py::test_reach_rollout_matches_oracle, tip control
ACT_LOW = np.float32([[0.2, 0.1, -1.0], [-0.3, 0.2, -1.0], [0.1, -0.2, -1.0], [-0.1, -0.1, -1.0], [0.3, 0.0, -1.0], [0.0, 0.3, -1.0], [-0.2, 0.2, -1.0],
                      [0.3, -0.2, 0.4]])


def scenes(high):
    """-> states [8, D] float32.  high: the pressed envs' tip target 12 cm above the table (the plan sends them to the packed list)"""
    pressed, _ = RC.pressed_states()
    ora = O.OracleEnv('reach', N, seed_base=11, seed_stride=1, max_episode_steps=1000)
    ora.reset(), ora.reset()
    st = ora.get_state().copy()
    ora.close()
    st[0:4] = pressed
    st[4:7] = pressed[0:3]
    st[4:7, 5] += np.float32([0.10, -0.15, 0.07])            # wrist rolled
    st[4:7, 21:28] = st[4:7, 0:7]
    st[:, 29] = 0                                           # elapsed
    if high:
        st[PRESSED, 20] = np.float32(0.30)
    return st


def _env(pmg, library, n, switches, **kw):
    keys = ('PMG_REACH_TWO_WAVES', 'PMG_PACKED', 'PMG_ENV_CYCLES')
    saved = {k: os.environ.get(k) for k in keys}
    os.environ.update(dict({'PMG_REACH_TWO_WAVES': '1', 'PMG_PACKED': '1', 'PMG_ENV_CYCLES': '1'}, **switches))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            env, banner = SC._handle_banner(lambda: pmg.make_env(task='reach', num_envs=n, seed=11, seed_stride=1, max_episode_steps=1000, _library=library, **kw))
        for k, v in switches.items():
            assert '%s=%s' % (k, v) in banner, banner
        return env
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def step(pmg, library, st, act, switches, **kw):
    """one env step -> dict(state, obs..., nc: largest contact count of the step per env, lists)"""
    env = _env(pmg, library, len(st), switches, **kw)
    try:
        env.reset()
        env.set_state(st)
        o, r, d, info = env.step(act)
        sch = env.handle.schedule()
        return dict(state=env.get_state(), obs=o['observation'], ag=o['achieved_goal'], reward=r, nc=env.handle.env_cycles()[:, 1].copy(),
                    prone=np.sort(sch['prone']), free=np.sort(sch['free']), redo=np.sort(sch['redo']))
    finally:
        env.close()


def _same_bits(a, b, label):
    for k in ('state', 'obs', 'ag', 'reward'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (label, k, np.argwhere(x != y)[:4].tolist())


def check_kernels_agree(pmg, library, out=print):
    """-> the four runs (two-wavefront, one-wavefront | redo, one-wavefront on every env), bit-equal in pairs"""
    low, high = scenes(False), scenes(True)
    two = step(pmg, library, low, ACT_LOW, {'PMG_REACH_TWO_WAVES': '1'})
    one = step(pmg, library, low, ACT_LOW, {'PMG_REACH_TWO_WAVES': '0'})
    assert set(PRESSED) <= set(two['prone']) and np.array_equal(two['prone'], one['prone']), (two['prone'], one['prone'])
    assert (two['nc'][PRESSED] >= 1).all() and (two['nc'][:4] == 8).all() and np.array_equal(two['nc'][two['prone']], one['nc'][one['prone']]), two['nc']
    _same_bits(two, one, 'pmg_k_step_reach2 against pmg_k_step_reach')
    zero = np.zeros((N, 3), np.float32)
    redo = step(pmg, library, high, zero, {'PMG_PACKED': '1'})
    full = step(pmg, library, high, zero, {'PMG_PACKED': '0'})
    assert np.array_equal(redo['redo'], PRESSED) and len(redo['prone']) == 0 and len(full['redo']) == 0, (redo['redo'], redo['prone'], full['redo'])
    assert (redo['nc'][:4] == 8).all()
    _same_bits(redo, full, 'pmg_k_redo against pmg_k_step_reach')
    out('reach kernels: %d envs in contact (counts %s); two-wavefront = one-wavefront and redo = one-wavefront, bit for bit' % (len(PRESSED), two['nc'][PRESSED].tolist()))
    return dict(two=(low, ACT_LOW, two), one=(low, ACT_LOW, one), redo=(high, zero, redo), full=(high, zero, full))


def check_full_step_against_oracle(runs, out=print):
    for name, (st, act, got) in runs.items():
        ora = O.OracleEnv('reach', N, seed_base=11, seed_stride=1, max_episode_steps=1000)
        ora.reset(), ora.reset()
        ora.set_state(st)
        oo = ora.step(act)[0]
        eo, es = float(np.abs(got['obs'] - oo['observation']).max()), float(np.abs(got['state'] - ora.get_state()).max())
        ora.close()
        out('reach kernels, full step, %-5s observation error %.3g (bar %.0e), state error %.3g (bar %.0e)' % (name + ':', eo, OBS_TOL, es, STATE_TOL))
        assert eo < OBS_TOL and es < STATE_TOL, (name, eo, es)


def check_one_substep_against_oracle(pmg, library_one_substep, out=print):
    """the one-wavefront kernel after one substep, joint control, at the reach bars of substep_cases"""
    st = scenes(False)
    act = np.zeros((N, 7), np.float32)
    got = step(pmg, library_one_substep, st, act, {'PMG_PACKED': '0'}, joint_control=True)
    ora = O.SubstepOracle('reach', N, substeps=1, seed_base=11, seed_stride=1, max_episode_steps=1000, joint_control=True)
    ora.reset(), ora.reset()
    ora.set_state(st)
    ora.step(act)
    s64, info = ora.get_state(), ora.last_substep()
    ora.close()
    res = info['residual'][:, :4]
    ran = np.arange(4)[None, :] < info['iterations'][:, None]
    near_exit = (ran & (res >= SC.RESIDUAL_THRESHOLD / 4) & (res <= SC.RESIDUAL_THRESHOLD * 4)).any(1)
    assert np.array_equal(got['nc'][PRESSED], info['nc'][PRESSED]), (got['nc'], info['nc'])
    keep = ~near_exit
    assert keep.sum() >= N - 2, near_exit
    bars = SC.reference('reach')['bars']
    for g, cols in SC.groups('reach').items():
        d = np.abs(got['state'][:, cols].astype(np.float64) - s64[:, cols]).max(1)
        out('reach one-wavefront kernel, one substep, %-3s worst %.3g  bar %.3g  (%d of %d envs kept)' % (g, d[keep].max(), bars[g], keep.sum(), N))
        assert (d[keep] <= bars[g]).all(), (g, d, bars[g])
