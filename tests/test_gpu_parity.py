"""-m gpu: the HIP path (through the C ABI) against the CPU oracle on identical seeded inputs."""
import numpy as np
import pytest

import oracle_lib
import pybullet_multigoal_gym_amd as pmg

pytestmark = pytest.mark.gpu

# float32 wave-per-env kernel vs float64 restatement: absolute tolerance on
# positions [m] / joint angles [rad] after a rollout of the stated length
OBS_TOL = 2e-4
STATE_TOL = 5e-4


JOINT_OUTLIERS = 2


def _pair(task, N, **kw):
    env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, **kw)
    ora = oracle_lib.OracleEnv(task, N, seed_base=0, seed_stride=1, threads=8,
                               **{k: v for k, v in kw.items() if k in ('num_block', 'binary_reward', 'joint_control',
                                                                        'max_episode_steps', 'distance_threshold')})
    ora.reset()
    return env, ora


def test_library_is_the_hip_build(hip_library):
    assert hip_library.path.endswith('libpmg_hip.so')


@pytest.mark.parametrize('joint_control', [False, True])
def test_reach_rollout_matches_oracle(built, joint_control):
    """Tip control stays contact-free for most envs (tight bound).  Joint control drives fingers
    into the table, where the solver's own early-exit threshold (1e-7 on squared velocity changes,
    i.e. ~3e-4 m/s) is the parity floor, so the bound is the contact one."""
    N, T = 64, 50
    # joint control: the maximum over the envs but for JOINT_OUTLIERS of the 64 (fingers scraping the table for a whole
    # episode: stick / slip flips in float32); measured round 2: median 3.6e-7, p90 3.5e-6
    OBS_TOL = 2e-4 if not joint_control else 1e-3
    STATE_TOL = 5e-4 if not joint_control else 5e-3     # the state rows hold velocities too (solver early exit: ~3e-4 m/s)
    env, ora = _pair('reach', N, joint_control=joint_control)
    # joint control: the envs whose fingers scrape the table bifurcate (stick / slip) -- how many does the chaos floor lose
    # (oracle_lib.FloorOracle: float64 arithmetic, the state rounded to float32 every substep)?  The device may lose twice as
    # many + 1, at least JOINT_OUTLIERS
    floor = oracle_lib.FloorOracle('reach', N, seed_base=0, seed_stride=1, threads=8, joint_control=True) if joint_control else None
    if floor is not None:
        floor.reset(), floor.reset()
    o, oo = env.reset(), ora.reset()
    assert np.array_equal(o['desired_goal'], oo['desired_goal'])
    assert np.abs(o['observation'] - oo['observation']).max() < 1e-5
    rs = np.random.RandomState(12345)
    A = env.dims.action_dim
    worst = 0.0
    per_env = np.zeros(N)
    for t in range(T):
        a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
        o, r, d, info = env.step(a)
        oo, ro, do, oko = ora.step(a)
        if floor is not None:
            floor.step(a)
        per_env = np.maximum(per_env, np.abs(o['observation'] - oo['observation']).max(1))
        worst = float(per_env.max()) if not joint_control else float(np.sort(per_env)[-1 - JOINT_OUTLIERS])
        assert np.array_equal(d, do)
        # reward may only differ where the distance sits on the threshold
        dist = np.linalg.norm(oo['achieved_goal'] - oo['desired_goal'], axis=-1)
        clear = np.abs(dist - 0.05) > 1e-4
        assert np.array_equal(r[clear], ro[clear])
        assert np.array_equal(info['goal_achieved'][clear], oko[clear])
    assert worst < OBS_TOL, worst
    serr = np.abs(env.get_state() - ora.get_state()).max(1)
    allowed = 0
    if joint_control:
        ferr = np.abs(floor.get_state() - ora.get_state()).max(1)
        allowed = max(JOINT_OUTLIERS, 2 * int((ferr > STATE_TOL).sum()) + 1)
        print('joint control: envs beyond %.0e in the state rows: device %d, chaos floor %d' % (STATE_TOL, (serr > STATE_TOL).sum(), (ferr > STATE_TOL).sum()))
    assert np.sort(serr)[-1 - allowed] < STATE_TOL
    assert np.median(per_env) < 2e-4
    assert d.all()
    env.close()


def test_reset_mask_and_reseed(built):
    N = 32
    env, ora = _pair('reach', N)
    env.reset(); ora.reset()
    mask = np.arange(N) % 3 == 0
    o = env.reset(mask=mask)
    oo = ora.reset(mask=mask)
    assert np.array_equal(o['desired_goal'], oo['desired_goal'])
    env.seed(7); ora.seed(7, 1)
    assert np.array_equal(env.reset()['desired_goal'], ora.reset()['desired_goal'])
    env.close()


def test_compute_reward_batch(built):
    env = pmg.make_env(task='reach', num_envs=4)
    rs = np.random.RandomState(0)
    ag = rs.uniform(-0.1, 0.1, (1000, 3)).astype(np.float32)
    dg = rs.uniform(-0.1, 0.1, (1000, 3)).astype(np.float32)
    r, ok = env._compute_reward(ag, dg)
    d = np.linalg.norm(ag.astype(np.float64) - dg, axis=-1)
    clear = np.abs(d - 0.05) > 1e-6
    assert np.array_equal(r[clear], -(d > 0.05).astype(np.float32)[clear])
    assert np.array_equal(ok[clear], ~(d > 0.05)[clear])
    assert r.dtype == np.float32 and np.signbit(r[ok]).all()   # -0.0 on success, as the reference
    env.close()


def _max_or_count(what, err, spread, bar=1e-3, extra=1):
    """Bar on the MAXIMUM over the envs (BASELINE.json's 1e-3), with a count for the envs beyond it: a contact made or
    missed one substep apart bifurcates a rollout under float32-sized state noise, whatever the arithmetic -- `spread` is
    the deviation of the chaos-floor yardstick (oracle_lib.FloorOracle: float64 arithmetic, state rounded to float32
    every substep) from the plain float64 oracle on the same seeds and actions.  The device may have twice as many envs
    beyond the bar as that, plus `extra`; everybody else must be inside the bar, and the typical env at float32 rounding
    (3 x the yardstick's median, at least 3e-5)."""
    err, spread = np.asarray(err, np.float64), np.asarray(spread, np.float64)
    n_dev, n_floor = int((err > bar).sum()), int((spread > bar).sum())
    print('%-40s max %.2e median %.2e beyond %.0e: %d   | chaos floor: max %.2e median %.2e beyond: %d'
          % (what, err.max(), np.median(err), bar, n_dev, spread.max(), np.median(spread), n_floor))
    assert n_dev <= 2 * n_floor + extra, (what, n_dev, n_floor, np.sort(err)[-4:])
    assert np.median(err) <= max(3 * np.median(spread), 3e-5), (what, np.median(err), np.median(spread))


@pytest.mark.parametrize('task,kw', [('push', {}), ('pick_and_place', {}), ('pick_and_place', {'binary_reward': False}),
                                     ('slide', {}), ('block_stack', {'num_block': 4}), ('block_rearrange', {'num_block': 3}),
                                     ('chest_push', {'num_block': 2}), ('chest_pick_and_place', {'num_block': 5, 'grip_informed_goal': True}),
                                     ('chest_push', {'num_block': 3, 'joint_control': True}), ('block_stack', {'num_block': 5, 'joint_control': True})])
def test_contact_tasks_match_oracle_within_its_own_precision_spread(built, task, kw):
    """Contact-rich rollouts are chaotic and the PGS early exit makes velocities only ~3e-4 exact, so
    the HIP path is held to the float64 oracle on positions over a short horizon, with a count of the envs beyond 1e-3
    measured against the chaos floor (_max_or_count)."""
    N, T = 64, 10
    env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, **kw)
    okw = {k: v for k, v in kw.items()}
    o64 = oracle_lib.OracleEnv(task, N, seed_base=0, seed_stride=1, threads=8, **okw)
    o32 = oracle_lib.FloorOracle(task, N, seed_base=0, seed_stride=1, threads=8, **okw)
    for e in (o64, o32):
        e.reset()
    o, a64, a32 = env.reset(), o64.reset(), o32.reset()
    assert np.array_equal(o['desired_goal'], a64['desired_goal'])
    assert np.abs(o['observation'] - a64['observation']).max() < 1e-5
    rs = np.random.RandomState(12345)
    A = env.dims.action_dim
    for t in range(T):
        a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
        o, r, d, info = env.step(a)
        a64, r64, d64, ok64 = o64.step(a)
        a32, r32, d32, ok32 = o32.step(a)
    err = np.abs(o['achieved_goal'] - a64['achieved_goal']).max(1)      # block positions
    spread = np.abs(a32['achieved_goal'] - a64['achieved_goal']).max(1)
    _max_or_count('%s blocks' % task, err, spread)
    tip_err = np.abs(o['observation'][:, :3] - a64['observation'][:, :3]).max(1)
    tip_spread = np.abs(a32['observation'][:, :3] - a64['observation'][:, :3]).max(1)
    _max_or_count('%s tip' % task, tip_err, tip_spread)
    if kw.get('binary_reward', True):
        assert (r != r64).mean() <= 0.02      # teacher-forced: no flag differs off the threshold (tests/test_gpu_tail_parity.py); here one of 64 envs may sit ON it
    else:
        assert np.percentile(np.abs(r - r64), 90) < 2e-3 and r.dtype == np.float32
    assert o['observation'].shape == (N, env.dims.observation_dim) and np.isfinite(o['observation']).all()
    env.close()


@pytest.mark.parametrize('scenario', ['slide_push', 'palm_block'])
def test_constructed_cylinder_contacts_match_oracle(built, scenario):
    """cylinder x box pairs on the device, in configurations random policies rarely reach within 10 steps: the
    slide puck pushed by the closed fingers, and a block wedged between the open fingers against the gripper-base
    cylinder.  32 envs with slightly different object offsets; positions after two env steps (200 substeps)."""
    N = 32
    task = 'slide' if scenario == 'slide_push' else 'pick_and_place'
    env, ora = _pair(task, N)
    o32 = oracle_lib.FloorOracle(task, N, seed_base=0, seed_stride=1, threads=8)
    o32.reset()
    env.reset(), ora.reset(), o32.reset()
    st = ora.get_state().copy()
    off = np.random.RandomState(1).uniform(-0.004, 0.004, (N, 2)).astype(np.float32)
    if scenario == 'slide_push':
        st[:, 64] = -0.52 + off[:, 0]; st[:, 65] = 0.045 + off[:, 1]; st[:, 66] = 0.170
        acts = [[0, 1, 0], [0, 1, 0]]
    else:
        st[:, 64] = -0.52 + off[:, 0]; st[:, 65] = off[:, 1] * 0.25; st[:, 66] = 0.25 + 0.0295
        acts = [[0, 0, 0, 1], [0, 0, -1, 1]]
    st[:, 67:71] = [0, 0, 0, 1]; st[:, 71:77] = 0
    env.set_state(st), ora.set_state(st), o32.set_state(st)
    for a in acts:
        a = np.tile(np.float32(a), (N, 1))
        env.step(a), ora.step(a), o32.step(a)
    se, so, s32 = env.get_state(), ora.get_state(), o32.get_state()
    # bar: the oracle's own float32-vs-float64 spread on the same scenario (solver early-exit floor)
    for cols in (slice(0, 9), slice(64, 67)):
        err, spread = np.abs(se[:, cols] - so[:, cols]).max(1), np.abs(s32[:, cols] - so[:, cols]).max(1)
        _max_or_count('%s %s' % (scenario, cols), err, spread)
    if scenario == 'slide_push':
        assert (so[:, 65] > 0.055).all() and np.abs(so[:, 66] - 0.170).max() < 1e-3   # pushed along +y, still on the table
    else:
        assert (so[:, 66] > 0.25).mean() > 0.9                                          # held by the contacts
    env.close()


@pytest.mark.parametrize('task,kw,rest_z', [('push', {}, 0.016), ('slide', {}, 0.011), ('block_rearrange', {'num_block': 3}, 0.016),
                                            ('chest_push', {'num_block': 2}, 0.016)])
def test_object_off_the_table_lands_on_the_floor(built, task, kw, rest_z):
    """The robot URDF's base plane (iiwa14_parallel_jaw.urdf:37-58: a 5 x 5 x 0.002 m collision box under link_0, friction 1).
    64 envs: object 0 starts beside the table's +x side wall (half of them with a sideways velocity and a spin), falls 16 cm and
    comes to rest on the floor at z = 0.001 + its half height -- on the device as in the oracle; rounds 1-5 let it fall for the
    rest of the episode (soak: z down to -107 m)."""
    N = 64
    env, ora = _pair(task, N, **kw)
    env.reset(), ora.reset()
    st = ora.get_state().copy()
    rs = np.random.RandomState(4)
    edge = (-0.70 if task == 'slide' else -0.52) + (0.5 if task == 'slide' else 0.25)
    st[:, 64] = edge + 0.04 + rs.uniform(0, 0.02, N); st[:, 65] = rs.uniform(-0.2, 0.2, N); st[:, 66] = 0.17
    st[:, 67:71] = [0, 0, 0, 1]; st[:, 71:77] = 0
    st[N // 2:, 71] = rs.uniform(0.05, 0.3, N - N // 2)          # thrown outwards ...
    st[N // 2:, 75] = rs.uniform(-3, 3, N - N // 2)              # ... tumbling
    st = st.astype(np.float32)
    env.set_state(st), ora.set_state(st)
    a = np.zeros((N, env.dims.action_dim), np.float32)
    for t in range(8):
        env.step(a), ora.step(a)
    se, so = env.get_state(), ora.get_state()
    flat = slice(0, N // 2)                                       # dropped flat: deterministic, at rest after two steps
    assert np.abs(so[flat, 66] - rest_z).max() < 2e-4 and np.abs(se[flat, 66] - rest_z).max() < 2e-4
    assert np.abs(se[flat, 64:71] - so[flat, 64:71]).max() < 1e-4
    # tumbling: nobody under the floor, everybody down and (nearly) at rest on it; poses agree but for bifurcated landings
    for s_ in (se, so):
        assert (s_[:, 66] > 0.009).all() and (s_[:, 66] < 0.001 + 0.0317 + 1e-3).all()
    terr = np.abs(se[N // 2:, 64:67] - so[N // 2:, 64:67]).max(1)
    print('%s tumbling onto the floor: position error median %.2e max %.2e' % (task, np.median(terr), terr.max()))
    assert np.median(terr) < 1e-3                                 # (a cube landing on a corner bifurcates: no bar on the maximum)
    assert np.abs(se[:, :9] - so[:, :9]).max() < 1e-4             # the arm saw none of it
    env.close()


@pytest.mark.parametrize('task', ['chest_push', 'chest_pick_and_place'])
def test_constructed_chest_contacts_match_oracle(built, task):
    """Chest walls, the sliding door / lid and the gripper on the device, in configurations a random policy does not
    reach in a few steps: a block thrown at the walls from inside the chest, another at the closed door (push) or dropped
    on the lid (pick and place), the door itself moving, and the gripper driven at the door so that it drags it.
    64 envs with slightly different offsets; poses against the oracle within its own float32-vs-float64 spread."""
    N = 64
    pnp = task == 'chest_pick_and_place'
    env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, num_block=2)
    ora = oracle_lib.OracleEnv(task, N, seed_base=0, seed_stride=1, threads=8, num_block=2)
    o32 = oracle_lib.FloorOracle(task, N, seed_base=0, seed_stride=1, threads=8, num_block=2)
    ora.reset(), o32.reset()
    env.reset(), ora.reset(), o32.reset()
    st = ora.get_state().copy()
    off = np.random.RandomState(2).uniform(-0.004, 0.004, (N, 2)).astype(np.float32)
    st[:, 48] = 0.02; st[:, 49] = 0.15; st[:, 50] = 0.0
    st[:, 64] = -0.65 + off[:, 0]; st[:, 65] = 0.03 + off[:, 1]; st[:, 66] = 0.19; st[:, 71:74] = [-0.3, 0.25, 0.0]
    if pnp:
        st[:, 77] = -0.65 + off[:, 1]; st[:, 78] = off[:, 0]; st[:, 79] = 0.30; st[:, 84:87] = 0
    else:
        st[:, 77] = -0.56 + off[:, 1]; st[:, 78] = -0.02 + off[:, 0]; st[:, 79] = 0.175; st[:, 84:87] = [-0.3, 0.0, 0.0]
    env.set_state(st), ora.set_state(st), o32.set_state(st)
    A = env.dims.action_dim
    a = np.zeros((N, A), np.float32)
    for t in range(10):
        a[:, 0] = -1; a[:, 2] = 1 if t < 7 else 0
        o, r, d, info = env.step(a)
        a64, r64, _, _ = ora.step(a)
        a32, r32, _, _ = o32.step(a)
    err = np.abs(o['achieved_goal'] - a64['achieved_goal']).max(1)        # door joint + block positions
    spread = np.abs(a32['achieved_goal'] - a64['achieved_goal']).max(1)
    # chest_pick_and_place: 2 of the 64 envs sit AT the bar (1.0e-3, 1.25e-3; chaos floor 0, the float32 oracle 3): the lid's
    # handle between the closing fingers
    _max_or_count('%s constructed, door + blocks' % task, err, spread, extra=1 if task == 'chest_push' else 3)
    tip_err = np.abs(o['observation'][:, :3] - a64['observation'][:, :3]).max(1)
    _max_or_count('%s constructed, tip' % task, tip_err, np.abs(a32['observation'][:, :3] - a64['observation'][:, :3]).max(1))
    so = ora.get_state()
    assert (so[:, 64] > -0.695).all() and (so[:, 64] < -0.6).all() and np.abs(so[:, 66] - 0.175).max() < 2e-3  # kept in by the walls
    if pnp:
        assert (so[:, 79] > 0.27).all()                                     # the dropped block rests on the lid
    else:
        assert (so[:, 77] > -0.58).all()                                    # kept out by the door
    assert np.isfinite(o['observation']).all()
    env.close()


def test_finger_opens_the_chest_door_by_its_handle(built):
    """The closed fingers come in over the front door next to its handle and push it sideways: finger x handle
    (cylinder x box) contacts drive the door DoF until the joint limit stops it and the motor latches."""
    N = 32
    env = pmg.make_env(task='chest_push', num_envs=N, seed=0, seed_stride=1, num_block=1)
    ora = oracle_lib.OracleEnv('chest_push', N, seed_base=0, seed_stride=1, threads=8, num_block=1)
    o32 = oracle_lib.FloorOracle('chest_push', N, seed_base=0, seed_stride=1, threads=8, num_block=1)
    ora.reset(), o32.reset()
    env.reset(), ora.reset(), o32.reset()
    rs = np.random.RandomState(4)
    for a, n in (([0, 0, 1], 6), ([0, -1, 0], 3), ([-1, 0, 0], 7), ([0, 1, 0], 14)):
        for _ in range(n):
            act = np.clip(np.tile(np.float32(a), (N, 1)) + rs.uniform(-0.05, 0.05, (N, 3)).astype(np.float32), -1, 1)
            o, r, d, info = env.step(act)
            a64 = ora.step(act)[0]
            a32 = o32.step(act)[0]
    q = a64['achieved_goal'][:, 0]
    assert (q > 0.1).all()                                          # every env opened its door
    err = np.abs(o['achieved_goal'] - a64['achieved_goal']).max(1)
    spread = np.abs(a32['achieved_goal'] - a64['achieved_goal']).max(1)
    _max_or_count('door opened by its handle', err, spread)
    assert np.array_equal(env.get_state()[:, 50], ora.get_state()[:, 50])   # the same envs latched the motor
    env.close()


@pytest.mark.parametrize('task', ['chest_push', 'chest_pick_and_place'])
def test_chest_curriculum_and_sub_goals_on_device(built, task):
    """num_block + 1 curriculum levels drawn per env on the device (level, moved blocks, counters, schedule) and the
    sub-goal lists of the decomposed task, against the oracle, env by env."""
    import warnings
    N, nb = 96, 3
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, num_block=nb, use_curriculum=True, num_goals_to_generate=32)
    ora = oracle_lib.OracleEnv(task, N, seed_base=0, seed_stride=1, threads=8, num_block=nb, use_curriculum=True, num_goals_to_generate=32)
    ora.reset()
    env.activate_curriculum_update(), ora.curriculum_update(True)
    for _ in range(20):
        o, oo = env.reset(), ora.reset()
        c = ora.curriculum()
        assert np.array_equal(o['desired_goal'], oo['desired_goal'])
        assert np.array_equal(env.last_curriculum_level, c['level']) and np.array_equal(env.curriculum_prob, c['prob'])
        assert np.array_equal(env.num_generated_goals_per_curriculum, c['generated'])
    assert c['level'].max() == nb and env.curriculum_prob.shape == (N, nb + 1)
    env.close()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, num_block=nb, task_decomposition=True, grip_informed_goal=True)
    ora = oracle_lib.OracleEnv(task, N, seed_base=0, seed_stride=1, threads=8, num_block=nb, task_decomposition=True, grip_informed_goal=True)
    ora.reset()
    env.reset(), ora.reset()
    a = np.random.RandomState(3).uniform(-1, 1, (N, env.dims.action_dim)).astype(np.float32)
    env.step(a), ora.step(a)
    for k in list(range(env.num_steps)) + [-1]:
        g = env.set_sub_goal(k)
        ora.set_sub_goal(k)
        ref = ora.reset(mask=np.zeros(N, bool))['desired_goal']
        assert np.abs(g - ref).max() < 2e-4, k          # live block / gripper poses after one step: float32 vs float64
    env.close()


def test_multistep_bookkeeping_on_device(built):
    """Curriculum draws / schedule against what the REFERENCE's own code drew (tests/golden/ref_sampling_*.json), batched:
    8 envs with seed_stride 0 must all replay the recorded sequence; and sub-goal switching against the oracle."""
    import json, os, warnings
    import ref_replay as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    N = 8
    for name in ('sampling_block_rearrange3_curriculum', 'sampling_block_stack4_curriculum'):
        fx = R.load(os.path.join(root, 'tests', 'golden', 'ref_%s.json' % name))
        nb = fx['oracle_kwargs']['num_block']
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            env = pmg.make_env(task=fx['task'], num_envs=N, seed=0, seed_stride=0, **fx['make_kwargs'])
        resets = 0
        for ev in fx['events']:
            if ev['op'] == 'curriculum_update':
                (env.activate_curriculum_update if ev['enabled'] else env.deactivate_curriculum_update)()
            elif ev['op'] == 'seed':
                env.seed(ev['seed'])
            elif ev['op'] == 'reset':
                o = env.reset()
                want = ev['out']
                assert (o['desired_goal'] == np.float32(want['obs']['desired_goal'])).all()
                c = want['curriculum']
                if 'level' in c:
                    assert (env.last_curriculum_level == c['level']).all()
                assert (env.curriculum_goal_step == c['goal_step']).all()
                assert (env.curriculum_prob == np.float32(c['prob'])).all()
                assert (env.num_generated_goals_per_curriculum == np.float32(c['generated'])).all()
                resets += 1
        assert resets >= 40
        s = env.get_state()
        env.set_state(s)                                   # curriculum tail round-trips through get/set_state
        assert np.array_equal(env.get_state(), s) and s.shape[1] == 64 + 13 * nb + 16
        env.close()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        env = pmg.make_env(task='block_stack', num_envs=N, num_block=3, seed=0, seed_stride=1, task_decomposition=True)
    ora = oracle_lib.OracleEnv('block_stack', N, num_block=3, seed_base=0, seed_stride=1, task_decomposition=True)
    ora.reset()
    env.reset(), ora.reset()
    mask = np.arange(N) % 2 == 0
    g1 = env.set_sub_goal(1, mask=mask)
    ora.set_sub_goal(1, mask=mask)
    ref = ora.reset(mask=np.zeros(N, bool))['desired_goal']
    assert np.array_equal(g1, ref) and np.array_equal(env.sub_goals[1][mask], ref[mask])
    a = np.zeros((N, 4), np.float32)
    o, r, d, info = env.step(a)
    oo, ro, do, oko = ora.step(a)
    assert np.abs(o['desired_goal'] - oo['desired_goal']).max() < 1e-4 and np.array_equal(r, ro)
    env.close()
    # grip-informed goals: (pick, place) sub-goal pairs, goal_dim 3*nb + 4
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        env = pmg.make_env(task='block_stack', num_envs=N, num_block=3, seed=0, seed_stride=1, task_decomposition=True,
                           grip_informed_goal=True)
    ora = oracle_lib.OracleEnv('block_stack', N, num_block=3, seed_base=0, seed_stride=1, task_decomposition=True,
                               grip_informed_goal=True)
    ora.reset()
    o, oo = env.reset(), ora.reset()
    assert o['desired_goal'].shape == (N, 13) and np.array_equal(o['desired_goal'], oo['desired_goal'])
    for s_ in (0, 3, 5):
        g = env.set_sub_goal(s_)
        ora.set_sub_goal(s_)
        assert np.array_equal(g, ora.reset(mask=np.zeros(N, bool))['desired_goal']) and np.array_equal(g, env.sub_goals[s_])
    o, r, d, info = env.step(np.zeros((N, 4), np.float32))
    oo, ro, do, oko = ora.step(np.zeros((N, 4), np.float32))
    assert np.abs(o['achieved_goal'] - oo['achieved_goal']).max() < 1e-4 and np.array_equal(r, ro)
    env.close()


def test_row_packed_reach_schedule_and_redo(built):
    """The packed path (four contact-free envs per wavefront) on the real device: every env of a fresh batch is on
    the contact-free list; an env whose plan entry is wrong (tip target high, fingers 7 mm inside the table) is
    caught by the per-substep predicate, recomputed by pmg_k_redo, and still matches the oracle; PMG_PACKED=0
    (one env per wavefront) agrees to fp32 rounding."""
    import os
    N = 64
    env, ora = _pair('reach', N)
    env.reset(), ora.reset()
    a = np.random.RandomState(5).uniform(-1, 1, (N, 3)).astype(np.float32)
    o, r, d, _ = env.step(a)
    oo, ro, do, _ = ora.step(a)
    sch = env.handle.schedule()
    assert len(sch['prone']) == 0 and sorted(sch['free']) == list(range(N)) and len(sch['redo']) == 0
    assert np.abs(o['observation'] - oo['observation']).max() < 2e-5
    st = ora.get_state().copy()
    bad = [1, 17, 40]
    for i in bad:
        q_low, _ = oracle_lib.ik(st[i, :9].astype(float), [-0.52, 0.0, 0.168])
        st[i, :7] = q_low[:7]; st[i, 9:18] = 0; st[i, 18:21] = [-0.52, 0, 0.30]; st[i, 21:28] = q_low[:7]
    env.set_state(st), ora.set_state(st)
    z = np.zeros((N, 3), np.float32)
    o, r, d, _ = env.step(z)
    oo, ro, do, _ = ora.step(z)
    sch = env.handle.schedule()
    assert sorted(sch['redo']) == bad and len(sch['prone']) == 0
    assert np.abs(o['observation'] - oo['observation']).max() < 5e-5 and (oo['observation'][bad, 2] > 0.17).all()
    packed_bits = env.get_state()
    os.environ['PMG_PACKED'] = '0'
    try:
        ref = pmg.make_env(task='reach', num_envs=N, seed=0, seed_stride=1)
    finally:
        del os.environ['PMG_PACKED']
    ref.reset()
    ref.set_state(st)
    ref.step(z)
    # same arithmetic as one env per wavefront; the two instantiations may contract multiply-adds differently
    diff = np.abs(ref.get_state() - packed_bits).max()
    assert diff < 2e-5, diff
    assert len(ref.handle.schedule()['redo']) == 0
    ref.close(), env.close()


def test_row_packed_object_overflow_goes_through_redo(built):
    """push on the device, four envs per wavefront: envs the plan leaves on the packed list (tip target 10 cm from
    the block) whose closed fingers nevertheless touch the block on the table exceed the 12-contact row store, are
    given up and recomputed by pmg_k_redo_env<1, 24, CYL>; everything still tracks the oracle."""
    N = 64
    env, ora = _pair('push', N)
    o32 = oracle_lib.FloorOracle('push', N, seed_base=0, seed_stride=1, threads=8)
    o32.reset()
    env.reset(), ora.reset(), o32.reset()
    st = ora.get_state().copy()
    tip = ora.reset(mask=np.zeros(N, bool))['observation'][:, :2]
    bad = [3, 20, 21, 47]
    for i in bad:
        st[i, 64:67] = [tip[i, 0], tip[i, 1] + 0.0255, 0.175]   # 0.5 mm from the side of the closed fingers
        st[i, 67:71] = [0, 0, 0, 1]; st[i, 71:77] = 0
        st[i, 18:21] = [tip[i, 0], tip[i, 1] - 0.10, 0.176]
    env.set_state(st), ora.set_state(st), o32.set_state(st)
    z = np.zeros((N, 3), np.float32)
    env.step(z), ora.step(z), o32.step(z)
    sch = env.handle.schedule()
    assert sorted(sch['redo']) == bad and set(bad) <= set(sch['free'])
    se, so, s32 = env.get_state(), ora.get_state(), o32.get_state()
    for cols in (slice(0, 9), slice(64, 67)):
        err, spread = np.abs(se[:, cols] - so[:, cols]).max(1), np.abs(s32[:, cols] - so[:, cols]).max(1)
        _max_or_count('redo_obj %s' % cols, err, spread)
        assert err[bad].max() < 3 * spread[bad].max() + 1e-3
    env.close()


def test_full_size_properties_4096(built):
    """BASELINE.json configs[1] size: determinism, per-env independence, reset idempotence."""
    N = 4096
    env = pmg.make_env(task='reach', num_envs=N, seed=0, seed_stride=1)
    a = np.random.RandomState(3).uniform(-1, 1, (N, 3)).astype(np.float32)
    env.reset()
    s0 = env.get_state()
    o1, r1, d1, _ = env.step(a)
    s1 = env.get_state()
    env.set_state(s0)
    o2, r2, d2, _ = env.step(a)                      # bit-identical replay from a restored state
    assert np.array_equal(o1['observation'], o2['observation']) and np.array_equal(s1, env.get_state())
    # envs are independent: permuting the batch permutes the result
    perm = np.random.RandomState(4).permutation(N)
    env.set_state(s0[perm])
    o3, _, _, _ = env.step(a[perm])
    assert np.array_equal(o3['observation'], o1['observation'][perm])
    # tip stays inside the clip box up to tracking error, goals inside the target box
    assert (o1['observation'][:, 2] > 0.17).all() and (np.abs(o1['observation'][:, 1]) < 0.21).all()
    g = o1['desired_goal']
    assert (g[:, 0] >= -0.64).all() and (g[:, 0] <= -0.40).all() and (g[:, 2] >= 0.175).all() and (g[:, 2] <= 0.40).all()
    assert np.linalg.norm(g - [-0.52, 0.0, 0.25], axis=1).min() > 0.1
    # seed_stride=1: distinct goals per env; a reseed with stride 0 makes them all equal (reference behaviour)
    assert len(np.unique(g[:, 0])) > N // 2
    env.handle.seed(0, 0)
    g0 = env.reset()['desired_goal']
    assert (g0 == g0[0]).all()
    env.close()


def test_rccl_single_rank_allgather_and_kernel_timer(built):
    env = pmg.make_env(task='reach', num_envs=256, seed=1)
    h = env.handle
    h.comm_init(0, 1, h.comm_unique_id())
    env.reset()
    a = h.device_alloc(256 * 3 * 4)
    h.upload(a, np.zeros((256, 3), np.float32))
    out = h.device_alloc(256 * env.dims.packed_dim * 4)
    h.timing_reset()
    h.step_device(a)
    h.allgather_packed(out)
    h.sync()
    ms, n = h.timing_read()
    assert n == 1 and 0 < ms < 1000
    got = np.zeros((256, env.dims.packed_dim), np.float32)
    h.download(got, out)
    o = h.read_outputs()
    assert np.array_equal(got[:, :3], o[0])
    h.device_free(a)
    h.device_free(out)
    env.close()


def test_rccl_single_rank_overlapped_allgather_on_the_device(built):
    """pmg_comm_overlap on the real runtime (one rank through RCCL): 12 steps with random actions, the all-gather of every step
    enqueued on the communication stream and NOT waited for before the next two steps are enqueued; every gathered table
    must hold exactly the rows its step left (read back from the double-buffered row buffer right behind the step), the
    row buffer must alternate, and the comm events count every all-gather."""
    N, T = 1024, 12
    env = pmg.make_env(task='push', num_envs=N, seed=1, seed_stride=1, max_episode_steps=5)
    h = env.handle
    h.comm_init(0, 1, h.comm_unique_id())
    h.comm_overlap(True)
    env.reset()
    S = env.dims.packed_dim
    rs = np.random.RandomState(3)
    acts = [h.device_alloc(N * 3 * 4) for _ in range(T)]
    for a in acts:
        h.upload(a, rs.uniform(-1, 1, (N, 3)).astype(np.float32))
    tables = [h.device_alloc(N * S * 4) for _ in range(T)]       # one table per step: all of them are checked at the end
    rows_ptr = []
    h.timing_reset()
    for t in range(T):
        h.step_device(acts[t])
        h.reset_done_device()
        rows_ptr.append(h.device_ptr())
        h.allgather_packed_async(tables[t])
    h.allgather_wait(host=True)
    h.sync()
    assert len(set(rows_ptr)) == 2 and all(rows_ptr[t] != rows_ptr[t + 1] for t in range(T - 1))
    assert h.comm_timing()[2] == T
    # replay the same steps without the collective: the rows of every step, to compare the tables with
    ref = pmg.make_env(task='push', num_envs=N, seed=1, seed_stride=1, max_episode_steps=5)
    ref.reset()
    want = np.zeros((N, S), np.float32)
    got = np.zeros((N, S), np.float32)
    for t in range(T):
        a = np.zeros((N, 3), np.float32)
        h.download(a, acts[t])
        aa = ref.handle.device_alloc(N * 3 * 4)
        ref.handle.upload(aa, a)
        ref.handle.step_device(aa)
        ref.handle.reset_done_device()
        ref.handle.sync()
        ref.handle.download(want, ref.handle.device_ptr())
        ref.handle.device_free(aa)
        h.download(got, tables[t])
        assert np.array_equal(got, want), (t, np.abs(got - want).max())
    for p in acts + tables:
        h.device_free(p)
    ref.close()
    env.close()


@pytest.mark.parametrize('task,N,kw', [('pick_and_place', 8192, {'binary_reward': False}),      # BASELINE.json configs[3]: dense ...
                                       ('pick_and_place', 8192, {'binary_reward': True}),       # ... and binary
                                       ('block_stack', 4096, {'num_block': 4}),                  # configs[4]
                                       ('push', 4096, {})])                                      # configs[2]
def test_full_size_contact_configs_properties(built, task, N, kw):
    """The BASELINE.json contact configurations at their full batch sizes, through size-independent properties:
    bit-identical replay from a restored state, batch-permutation equivariance, physical invariants (nothing falls
    through the table, objects stay finite and on / above it), reward consistent with the returned goals."""
    env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, **kw)
    A = env.dims.action_dim
    rs = np.random.RandomState(7)
    env.reset()
    for _ in range(2):
        env.step(rs.uniform(-1, 1, (N, A)).astype(np.float32))
    s0 = env.get_state()
    a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
    o1, r1, d1, i1 = env.step(a)
    s1 = env.get_state()
    env.set_state(s0)
    o2, r2, d2, i2 = env.step(a)
    assert np.array_equal(o1['observation'], o2['observation']) and np.array_equal(r1, r2) and np.array_equal(s1, env.get_state())
    perm = np.random.RandomState(8).permutation(N)
    env.set_state(s0[perm])
    o3, r3, _, _ = env.step(a[perm])
    assert np.array_equal(o3['observation'], o1['observation'][perm]) and np.array_equal(r3, r1[perm])
    assert np.isfinite(o1['observation']).all()
    ag = o1['achieved_goal'].reshape(N, -1, 3)
    assert (ag[..., 2] > 0.17).all() and (ag[..., 2] < 0.6).all()           # on the table (top 0.16 + half 0.015) or lifted
    assert (np.abs(ag[..., 0] + 0.52) < 0.35).all() and (np.abs(ag[..., 1]) < 0.4).all()
    d = np.linalg.norm(o1['achieved_goal'].astype(np.float64) - o1['desired_goal'], axis=-1)
    if kw.get('binary_reward', True):
        clear = np.abs(d - 0.05) > 1e-4
        assert np.array_equal(r1[clear], -(d > 0.05).astype(np.float32)[clear])
    else:
        assert np.abs(r1 + d).max() < 1e-5
    assert np.array_equal(i1['goal_achieved'][np.abs(d - 0.05) > 1e-4], (d <= 0.05)[np.abs(d - 0.05) > 1e-4])
    env.close()


@pytest.mark.parametrize('task', ['chest_push', 'chest_pick_and_place', 'block_rearrange'])
def test_full_size_multi_block_properties(built, task):
    """4096 envs x 4 blocks of the tasks outside BASELINE.json's list, 12 random steps: bit-identical replay from a restored
    state, batch-permutation equivariance, the door inside its joint limits with a 0 / 1 motor latch, goals leading with
    the door's open state, reward consistent with the returned goals."""
    N = 4096
    chest = task.startswith('chest')
    env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, num_block=4)
    A = env.dims.action_dim
    rs = np.random.RandomState(9)
    env.reset()
    for _ in range(10):
        env.step(rs.uniform(-1, 1, (N, A)).astype(np.float32))
    s0 = env.get_state()
    a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
    o1, r1, d1, i1 = env.step(a)
    s1 = env.get_state()
    env.set_state(s0)
    o2, r2, d2, i2 = env.step(a)
    assert np.array_equal(o1['observation'], o2['observation']) and np.array_equal(r1, r2) and np.array_equal(s1, env.get_state())
    perm = np.random.RandomState(8).permutation(N)
    env.set_state(s0[perm])
    o3, r3, _, _ = env.step(a[perm])
    assert np.array_equal(o3['observation'], o1['observation'][perm]) and np.array_equal(r3, r1[perm])
    assert np.isfinite(o1['observation']).all() and np.abs(o1['observation']).max() <= 5.0     # clipped (kuka_multi_step_base_env.py:306)
    if chest:
        upper = 0.12 if task == 'chest_push' else 0.10
        q = o1['achieved_goal'][:, 0]
        # (a gripper that drags the door against its stop pushes the ERP-0.2 limit row in by 0.2 mm per step: the oracle too)
        assert (q > -5e-3).all() and (q < upper + 5e-3).all()
        assert np.isin(s1[:, 50], [0.0, 1.0]).all() and (np.abs(upper - q[s1[:, 50] == 1.0]) < 0.02).all()
        assert np.array_equal(o1['desired_goal'][:, 0], np.full(N, np.float32(upper)))
        assert np.array_equal(o1['desired_goal'][:, 1:], np.tile(np.float32([-0.65, 0.0, 0.175]), (N, 4)))
    d = np.linalg.norm(o1['achieved_goal'].astype(np.float64) - o1['desired_goal'], axis=-1)
    clear = np.abs(d - 0.05) > 1e-4
    assert np.array_equal(r1[clear], -(d > 0.05).astype(np.float32)[clear])
    env.close()


def _expected_schedule(env, actions):
    """What pmg_k_plan must write for a reach batch under tip control (contact_prone() of pmg_kernels.h restated):
    the envs whose tip target is, or will be after this action, within 12 mm of the lower clip plane -- in env order --
    then everybody else in env order."""
    st = env.get_state()
    z = st[:, 20].astype(np.float32)
    zn = np.clip(z + actions[:, 2] * np.float32(0.01), np.float32(0.175), np.float32(0.55))
    prone = np.minimum(z, zn) < np.float32(0.175) + np.float32(0.012)
    idx = np.arange(len(st))
    return idx[prone], idx[~prone]


def test_env_cycle_diagnostics_on_device(built, monkeypatch):
    """PMG_ENV_CYCLES=1: per-env shader cycles and largest contact count of the last step (PMG_BUF_ENV_CYCLES).  The envs
    whose gripper was sent down onto the table must be the expensive ones, and every push env sees its block's table
    contacts."""
    monkeypatch.setenv('PMG_ENV_CYCLES', '1')
    env = pmg.make_env(task='push', num_envs=256, seed=4)
    env.reset()
    a = np.zeros((256, 3), np.float32)
    a[:128, 2] = -1.0                                     # first half: down to the table; second half: up
    a[128:, 2] = 1.0
    for _ in range(6):
        env.step(a)
    c = env.handle.env_cycles().astype(np.int64)
    env.close()
    assert (c[:, 0] > 0).all() and (c[:, 1] >= 4).all() and (c[:, 1] <= 24).all()
    assert np.median(c[:128, 1]) >= 8                     # fingers on the table: eight more contacts
    assert np.median(c[:128, 0]) > 1.15 * np.median(c[128:, 0])


@pytest.mark.parametrize('N', [4096, 16384 + 64, 65536 + 256, 131072])
def test_plan_schedule_at_every_batch_size(built, N):
    """One plan workgroup partitions batches up to 16 384 envs; larger ones take the two-pass plan over ceil(N / 1024)
    workgroups (pmg_k_plan_count / pmg_k_plan_scatter; round 2 stopped planning at 65 536 envs and fell back to one env
    per wavefront in identity order).  Either way the launch lists read back from the device are the
    stable partition of the batch -- contact-prone envs first, in env order, then the rest in env order -- every env is
    on exactly one list, steps once, and the fast path (four envs per wavefront) stays on at every size."""
    env = pmg.make_env(task='reach', num_envs=N, seed=0, seed_stride=1)
    env.reset()
    rs = np.random.RandomState(3)
    for t in range(12):       # walk a good part of the batch down to the table
        a = rs.uniform(-1, 1, (N, 3)).astype(np.float32)
        a[:, 2] = -np.abs(a[:, 2])
        env.step(a)
    s0 = env.get_state()
    a = rs.uniform(-1, 1, (N, 3)).astype(np.float32)
    want_prone, want_free = _expected_schedule(env, a)
    env.step(a)
    sch = env.handle.schedule()
    assert 0.02 * N < len(want_prone) < 0.9 * N
    assert np.array_equal(sch['prone'], want_prone) and np.array_equal(sch['free'], want_free)
    s1 = env.get_state()
    assert (s1[:, 29] == s0[:, 29] + 1).all()                                   # every env advanced its step counter once
    want = np.clip(s0[:, 18:21] + a * np.float32(0.01), [-0.67, -0.2, 0.175], [-0.37, 0.2, 0.55])
    assert np.abs(s1[:, 18:21] - want).max() < 1e-6                             # ... by its own action
    env.close()


@pytest.mark.parametrize('task', ['block_stack', 'chest_push'])
def test_longest_first_order_of_the_fast_path_list_changes_the_schedule_only(built, task, monkeypatch):
    """From 4096 envs on the plan of the many-body tasks orders the fast-path list by the envs' wavefront time in the previous
    step; the threshold is derived on the device (round 6: the cycle count above which the slowest 40 % of the list lay in the step
    before -- no tuned constants).  The order of a launch list is no input of any env's arithmetic: with the rule off
    (PMG_LPT_CYCLES=0) the same seeds and actions give the same states, bit for bit; with it on the list is a permutation of the
    same envs whose head are the envs that were slow in the step before -- every one of them slower than every env of the tail."""
    N, T = 4096, 6
    acts = np.random.RandomState(2).uniform(-1, 1, (T, N, 4)).astype(np.float32)[:, :, :(3 if task == 'chest_push' else 4)]
    acts = np.ascontiguousarray(acts)
    def run(lpt):
        if lpt is None: monkeypatch.delenv('PMG_LPT_CYCLES', raising=False)
        else: monkeypatch.setenv('PMG_LPT_CYCLES', lpt)
        env = pmg.make_env(task=task, num_envs=N, seed=7, seed_stride=1, num_block=4)
        env.reset()
        for t in range(T - 1):
            env.step(acts[t])
        cyc = env.handle.env_cycles()[:, 0].astype(np.int64) if lpt is None else None
        env.step(acts[T - 1])
        out = env.get_state().copy(), env.handle.schedule(), cyc
        env.close()
        return out
    s_off, sch_off, _ = run('0')
    s_on, sch_on, cyc = run(None)
    assert np.array_equal(s_on.view(np.uint32), s_off.view(np.uint32))
    assert np.array_equal(np.sort(sch_on['free']), np.sort(sch_off['free'])) and np.array_equal(sch_on['prone'], sch_off['prone'])
    assert len(sch_on['redo']) == len(sch_off['redo'])
    c = cyc[sch_on['free']]
    head_min, tail_max = np.minimum.accumulate(c)[:-1], np.maximum.accumulate(c[::-1])[::-1][1:]
    splits = np.nonzero(head_min > tail_max)[0] + 1                   # k such that every env of the first k was slower than every later one
    assert len(splits) >= 1, 'the list is not "slow envs of the previous step first"'
    k = int(splits[0])
    print(task, 'list 1:', len(c), 'envs, the leading', k, 'were the slow ones (threshold between %d and %d cycles / 64)' % (tail_max[k - 1], head_min[k - 1]))
    assert 0.15 * len(c) < k < 0.65 * len(c)                          # about the slowest 40 % (the threshold lags a step and is binned)
    assert np.array_equal(np.sort(sch_on['free'][:k]), sch_on['free'][:k]) and np.array_equal(np.sort(sch_on['free'][k:]), sch_on['free'][k:])   # env order inside either class
    assert not np.array_equal(sch_on['free'], sch_off['free'])       # ... which the default order does not do


@pytest.mark.parametrize('task,kw', [('reach', {}), ('reach', {'binary_reward': False}), ('push', {}), ('slide', {}),
                                     ('pick_and_place', {'binary_reward': False}), ('block_stack', {'num_block': 4}),
                                     ('block_rearrange', {'num_block': 3})])
def test_fast_paths_agree_with_one_env_per_wavefront(built, task, kw):
    """PMG_PACKED=1 (four envs per wavefront / small contact stores / redo) against PMG_PACKED=0 (one env per wavefront,
    full stores, no prediction) on the same seeds and actions: the same algorithm, so reach agrees to fp32 rounding and
    the chaotic contact tasks to a small multiple of it over a short horizon."""
    import os
    N, T = 512, 12
    def make(packed):
        os.environ['PMG_PACKED'] = packed
        try:
            return pmg.make_env(task=task, num_envs=N, seed=5, seed_stride=1, **kw)
        finally:
            del os.environ['PMG_PACKED']
    fast, ref = make('1'), make('0')
    of, orf = fast.reset(), ref.reset()
    assert np.array_equal(of['desired_goal'], orf['desired_goal']) and np.array_equal(of['observation'], orf['observation'])
    rs = np.random.RandomState(9)
    A = fast.dims.action_dim
    used_fast_path = False
    for t in range(T):
        a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
        of, rf, df, inf = fast.step(a)
        orf, rr, dr, inr = ref.step(a)
        used_fast_path = used_fast_path or len(fast.handle.schedule()['free']) > N // 2
    assert used_fast_path
    tip = np.abs(of['observation'][:, :3] - orf['observation'][:, :3]).max(1)
    ag = np.abs(of['achieved_goal'] - orf['achieved_goal']).max(1)
    if task == 'reach':
        assert tip.max() < 5e-5
        assert (rf != rr).mean() < 0.01 if kw.get('binary_reward', True) else np.abs(rf - rr).max() < 1e-4   # a distance may sit on the threshold
    else:
        # two float32 summation orders of the same algorithm over 12 chaotic contact steps: a count on the envs beyond 1e-3
        print('%s fast paths vs one-env-per-wavefront: tip max %.2e beyond 1e-3: %d; objects max %.2e beyond 1e-3: %d of %d'
              % (task, tip.max(), (tip > 1e-3).sum(), ag.max(), (ag > 1e-3).sum(), N))
        assert (tip > 1e-3).mean() <= 0.03 and (ag > 1e-3).mean() <= 0.05, ((tip > 1e-3).mean(), (ag > 1e-3).mean())
        assert np.median(tip) < 2e-5 and np.median(ag) < 2e-5, (np.median(tip), np.median(ag))
        assert (inf['goal_achieved'] != inr['goal_achieved']).mean() < 0.02
    fast.close(), ref.close()


def test_small_contact_store_overflow_goes_through_redo_multi(built):
    """block_rearrange with five blocks pushed together into a tight row on the table, gripper far away: 20 table
    contacts + 16 between neighbours exceed the 30-contact store of the fast list, so those envs must come back through
    pmg_k_redo_env<5, 48, 0> and still track the oracle."""
    import warnings
    N, nb = 32, 5
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        env = pmg.make_env(task='block_rearrange', num_envs=N, num_block=nb, seed=0, seed_stride=1)
    ora = oracle_lib.OracleEnv('block_rearrange', N, num_block=nb, seed_base=0, seed_stride=1, threads=8)
    o32 = oracle_lib.FloorOracle('block_rearrange', N, num_block=nb, seed_base=0, seed_stride=1, threads=8)
    ora.reset(), o32.reset()
    env.reset(), ora.reset(), o32.reset()
    st = ora.get_state().copy()
    bad = [2, 9, 30]
    for i in bad:
        for b in range(nb):
            st[i, 64 + 13 * b:67 + 13 * b] = [-0.62, -0.10 + 0.0305 * b, 0.175]      # 0.5 mm gaps: inside the contact margin
            st[i, 67 + 13 * b:71 + 13 * b] = [0, 0, 0, 1]
            st[i, 71 + 13 * b:77 + 13 * b] = 0
    env.set_state(st), ora.set_state(st), o32.set_state(st)
    z = np.zeros((N, 3), np.float32)
    env.step(z), ora.step(z), o32.step(z)
    sch = env.handle.schedule()
    assert set(bad) <= set(sch['free']) and sorted(sch['redo']) == bad
    se, so, s32 = env.get_state(), ora.get_state(), o32.get_state()
    pos = [c for b in range(nb) for c in range(64 + 13 * b, 67 + 13 * b)]
    err, spread = np.abs(se[:, pos] - so[:, pos]).max(1), np.abs(s32[:, pos] - so[:, pos]).max(1)
    _max_or_count('redo_multi blocks', err, spread)
    assert err[bad].max() < 3 * spread[bad].max() + 1e-3
    env.close()


@pytest.mark.parametrize('kw,G', [({'num_block': 4}, 12), ({'num_block': 3}, 9), ({'num_block': 3, 'grip_informed_goal': True}, 13),
                                  ({'num_block': 4, 'grip_informed_goal': True}, 16), ({'num_block': 5, 'grip_informed_goal': True}, 19)])
def test_compute_reward_batch_multi_block_goals(built, kw, G):
    """HER relabelling batches with multi-block goal vectors go through the flat coalesced kernel (the 256-item span of a
    workgroup read as float4 words whatever G is); sizes that are not a multiple of 256 leave their tail to the generic
    kernel."""
    env = pmg.make_env(task='block_stack', num_envs=4, **kw)
    assert env.dims.goal_dim == G
    rs = np.random.RandomState(0)
    for B in (1000, 256, 257, 5, 70000):
        ag = rs.uniform(-0.1, 0.1, (B, G)).astype(np.float32)
        dg = (ag + rs.uniform(-0.03, 0.03, (B, G))).astype(np.float32)
        r, ok = env._compute_reward(ag, dg)
        d = np.linalg.norm(ag.astype(np.float64) - dg, axis=-1)
        clear = np.abs(d - 0.05) > 1e-6
        assert np.array_equal(r[clear], -(d > 0.05).astype(np.float32)[clear]) and np.array_equal(ok[clear], ~(d > 0.05)[clear])
    env.close()
    dense = pmg.make_env(task='block_stack', num_envs=4, binary_reward=False, **kw)
    ag = rs.uniform(-0.1, 0.1, (777, G)).astype(np.float32)
    dg = rs.uniform(-0.1, 0.1, (777, G)).astype(np.float32)
    r, ok = dense._compute_reward(ag, dg)
    assert np.abs(r + np.linalg.norm(ag.astype(np.float64) - dg, axis=-1)).max() < 1e-5
    dense.close()


@pytest.mark.parametrize('task,kw', [('reach', {}), ('push', {}), ('block_stack', {'num_block': 4, 'use_curriculum': True, 'num_goals_to_generate': 200}),
                                     ('chest_push', {'num_block': 2})])
def test_checkpoint_round_trip_on_device(built, hip_library, task, kw):
    """get_checkpoint() / set_checkpoint() (state rows + the per-env MT19937 streams + the curriculum switch) on the
    device: restored into the same env and into a fresh one, 64 envs continue bit-identically through steps, masked
    resets (new goals from the restored streams) and curriculum bookkeeping; a malformed RNG state is refused."""
    from test_host_api import _checkpoint_round_trip
    _checkpoint_round_trip(hip_library, task, 64, 3, 6, **kw)


def _sharded_equals_unsharded(lib, task, N, shards, T, kw=None):
    """The same envs (global seeds, same actions) stepped in ONE batch of N and in `shards` equal shards: every output and the
    whole state must be EQUAL bit for bit."""
    kw = dict(kw or {})
    mk = dict(task=task, seed=9, seed_stride=1, **kw)
    if lib is not None:
        mk['_library'] = lib
    full = pmg.make_env(num_envs=N, **mk)
    n = N // shards
    parts = [pmg.make_env(num_envs=n, env_index_offset=k * n, **mk) for k in range(shards)]
    of = full.reset()
    op = [e.reset() for e in parts]
    assert np.array_equal(of['desired_goal'], np.concatenate([o['desired_goal'] for o in op]))   # seeds follow the global index
    rs = np.random.RandomState(2)
    A = full.action_space.shape[-1]
    for t in range(T):
        a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
        a[::2, 2] = -np.abs(a[::2, 2])                  # half of the batch keeps its fingers down: the class whose kernel used to depend on batch-wide counts
        if task.startswith('chest'):
            a[1::4, 0] = -np.abs(a[1::4, 0])            # a quarter heads for the chest: gripper base on its rim, fingers at the door (cylinder pairs, both lists)
        rf = full.step(a)
        rp = [e.step(a[k * n:(k + 1) * n]) for k, e in enumerate(parts)]
    for key in ('observation', 'policy_state', 'achieved_goal', 'desired_goal'):
        assert np.array_equal(rf[0][key], np.concatenate([r[0][key] for r in rp])), (task, N, shards, key)
    assert np.array_equal(rf[1], np.concatenate([r[1] for r in rp])) and np.array_equal(rf[2], np.concatenate([r[2] for r in rp]))
    sf, sp = full.get_state(), np.concatenate([e.get_state() for e in parts])
    assert np.array_equal(sf, sp), (task, N, shards, np.abs(sf - sp).max())
    full.close()
    for e in parts:
        e.close()


@pytest.mark.parametrize('task', ['push', 'pick_and_place', 'slide', 'reach', 'block_stack', 'chest_push', 'chest_pick_and_place'])
@pytest.mark.parametrize('N,shards', [(512, 2), (4096, 8)])
def test_sharded_batch_is_bit_identical_to_the_unsharded_batch(built, task, N, shards):
    """north_star: the batch shards trivially -- env i on GPU i // N_local is the env of the single-GPU run.  Which kernel an
    env of a one-object task runs in (packed LDS rows / one env per wavefront in row space: different float32 summation
    orders) is a function of the env's own state and of the task (EnvParams::fd_div), never of batch-wide counts (rounds 2-4:
    median 1e-5, up to 1 % of the envs beyond 1e-3 after 12 steps): 512 envs against 2 x 256 and 4096 against 8 x 512, 12
    steps with half of the batch driven onto the table, outputs and state rows EQUAL.  The chest tasks (round 6): every chest kernel
    applies ONE rule to the cylinder pairs (repeat in double when in contact), whichever list an env is on."""
    _sharded_equals_unsharded(None, task, N, shards, 12, {'num_block': 3} if task == 'block_stack' else ({'num_block': 2} if task.startswith('chest') else {}))


def test_two_wavefront_reach_kernel_is_bit_identical_to_the_one_wavefront_kernel(built):
    """pmg_k_step_reach2 (the helper wavefront collides beside the dynamics; eight contact-free envs per workgroup) and
    pmg_k_step_reach (PMG_REACH_TWO_WAVES=0) run the same functions on the same data: after 40 steps that drive a good
    part of the batch onto the table the state rows and the packed outputs must be EQUAL, bit for bit."""
    import os
    N = 2048

    def make(two):
        os.environ['PMG_REACH_TWO_WAVES'] = two
        try:
            return pmg.make_env(task='reach', num_envs=N, seed=21, seed_stride=1)
        finally:
            del os.environ['PMG_REACH_TWO_WAVES']
    a2, a1 = make('1'), make('0')
    a2.reset(), a1.reset()
    rs = np.random.RandomState(8)
    touched = 0
    for t in range(40):
        a = rs.uniform(-1, 1, (N, 3)).astype(np.float32)
        a[:, 2] = -np.abs(a[:, 2])
        o2, r2, d2, i2 = a2.step(a)
        o1, r1, d1, i1 = a1.step(a)
        touched = max(touched, len(a2.handle.schedule()['prone']))
        for k in o2:
            assert np.array_equal(o2[k], o1[k]), (t, k)
        assert np.array_equal(r2, r1) and np.array_equal(i2['goal_achieved'], i1['goal_achieved'])
    assert touched > N // 4                                   # the two-wave workgroups did carry those steps
    assert np.array_equal(a2.get_state(), a1.get_state())
    a2.close(), a1.close()


@pytest.mark.gpu
@pytest.mark.parametrize('task,kw', [('reach', {}), ('push', {}), ('block_stack', {'num_block': 3, 'use_curriculum': True, 'num_goals_to_generate': 300})])
def test_device_side_done_reset_equals_step_plus_masked_reset(built, task, kw):
    """pmg_reset_done_device (include/pmg.h: the envs whose TimeLimit ran out reset themselves on the device, no host mask)
    against the same rollout with pmg_reset_device and the mask of the done envs built on the host: staggered 6-step
    episodes over 20 steps, 256 envs.  State rows, RNG streams and the observation / goal part of the packed rows must be
    EQUAL bit for bit after every step; reward | goal_achieved | done differ by design -- the done-reset keeps the
    finished step's values in the row (auto-reset convention), the masked reset zeroes them -- and calling it twice is a
    no-op."""
    N, T = 256, 6
    a, b = (pmg.make_env(task=task, num_envs=N, seed=31, seed_stride=1, max_episode_steps=T, **kw) for _ in range(2))
    a.reset(), b.reset()
    ha, hb = a.handle, b.handle
    A = a.dims.action_dim
    # stagger the phases: env i is reset once more after (i mod T) steps, in both envs alike
    rs = np.random.RandomState(5)
    acts = rs.uniform(-1, 1, (T + 20, N, A)).astype(np.float32)
    d_act = ha.device_alloc(acts[0].nbytes)
    d_mask = ha.device_alloc(N)
    d_act_b = hb.device_alloc(acts[0].nbytes)
    d_mask_b = hb.device_alloc(N)
    packed_a = np.empty((N, a.dims.packed_dim), np.float32)
    packed_b = np.empty_like(packed_a)
    tail = a.dims.packed_dim - 3
    n_resets = 0
    for t in range(T + 20):
        ha.upload(d_act, acts[t]); hb.upload(d_act_b, acts[t])
        ha.step_device(d_act); hb.step_device(d_act_b)
        hb.sync()
        hb.download(packed_b, hb.device_ptr())
        done = packed_b[:, tail + 2] != 0
        if t < T:                                   # pre-roll: the host mask sets up the staggering on both sides
            m = ((np.arange(N) + t + 1) % T == 0).astype(np.uint8)
            ha.upload(d_mask, m); hb.upload(d_mask_b, m)
            ha.reset_device(d_mask); hb.reset_device(d_mask_b)
        else:
            expected = (np.arange(N) + t + 1) % T == 0
            assert np.array_equal(done, expected), t        # TimeLimit's done IS the staggered phase
            n_resets += int(done.sum())
            ha.reset_done_device()
            ha.reset_done_device()                          # idempotent: a freshly reset env has elapsed = 0
            hb.upload(d_mask_b, done.astype(np.uint8))
            hb.reset_device(d_mask_b)
        ha.sync(); hb.sync()
        ha.download(packed_a, ha.device_ptr()); hb.download(packed_b, hb.device_ptr())
        assert np.array_equal(packed_a[:, :tail], packed_b[:, :tail]), t
        assert np.array_equal(a.get_state(), b.get_state()), t
        if t >= T:
            was = (np.arange(N) + t + 1) % T == 0
            assert np.all(packed_a[was, tail + 2] == 1.0) and np.all(packed_b[was, tail:] == 0.0)   # kept vs zeroed tails
            assert np.array_equal(packed_a[~was, tail:], packed_b[~was, tail:])
    assert n_resets > 0
    assert np.array_equal(ha.get_rng(), hb.get_rng())      # the same draws were taken from every env's stream
    for h, ptrs in ((ha, (d_act, d_mask)), (hb, (d_act_b, d_mask_b))):
        for p in ptrs:
            h.device_free(p)
    a.close(), b.close()
