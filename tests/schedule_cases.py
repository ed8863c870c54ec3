"""Whole steps through the public API, held to what the schedule promises (csrc/pmg_sched.h): an env's result
does not depend on the batch it is in nor on its place in it, both launch lists partition the batch at ragged sizes, the surplus
rows of the last packed wavefront write nothing, and every env a fast path gives up -- up to all of them at once -- comes back
through the redo pass.  Shared by tests/test_gpu_schedule.py (the device) and tests/test_schedule_emulated.py (the CPU emulator).
No numeric bar of its own: bits, integers, and the two bars of tests/test_gpu_parity.py's redo tests against the oracle."""
import hashlib

import numpy as np

import oracle_lib
import pybullet_multigoal_gym_amd as pmg

# family -> (task, options, the give-up recipe that applies to it)
FAMILIES = {
    'reach': ('reach', {}, 'misplan'),
    'push': ('push', {}, 'overflow'),
    'pick_and_place': ('pick_and_place', {}, None),
    'slide': ('slide', {}, None),
    'block_stack3': ('block_stack', {'num_block': 3}, None),
    'block_rearrange3': ('block_rearrange', {'num_block': 3}, None),
    'block_rearrange5': ('block_rearrange', {'num_block': 5}, 'tight_row'),      # (the tight row overflows the small store with five blocks only)
    'chest_push': ('chest_push', {'num_block': 2}, None),
    'chest_pick_and_place': ('chest_pick_and_place', {'num_block': 2}, None),
    'reach_joint': ('reach', {'joint_control': True}, None),
    'push_joint': ('push', {'joint_control': True}, None),
}
N_FULL, DROPPED = 13, 3
PLANTED, NEAR = [5, 11], [3, 9]          # envs given up by a fast path / sent to list 0 by a block beside the tip target


def _make(library, task, N, kw):
    import warnings
    extra = {} if library is None else {'_library': library}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, **kw, **extra)


def _script(rs, N, A, t):
    """A third of the batch straight down, a third straight up, the rest down at random: every class of the plan within six steps."""
    a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
    a[:, 2] = -np.abs(a[:, 2])
    a[0::3, 2] = -1.0
    a[1::3, 2] = 1.0
    return a


def plant_misplan(st, i):
    """reach: the tip target high, the fingers 7 mm inside the table (test_row_packed_reach_schedule_and_redo)."""
    q_low, _ = oracle_lib.ik(st[i, :9].astype(float), [-0.52, 0.0, 0.168])
    st[i, :7] = q_low[:7]; st[i, 9:18] = 0; st[i, 18:21] = [-0.52, 0, 0.30]; st[i, 21:28] = q_low[:7]


def plant_overflow(st, i, tip):
    """push: the block 0.5 mm from the side of the closed fingers, the tip target 10 cm away (test_row_packed_object_overflow_goes_through_redo)."""
    st[i, 64:67] = [tip[0], tip[1] + 0.0255, 0.175]
    st[i, 67:71] = [0, 0, 0, 1]; st[i, 71:77] = 0
    st[i, 18:21] = [tip[0], tip[1] - 0.10, 0.176]


def plant_tight_row(st, i, nb):
    """five blocks in a row with 0.5 mm gaps (test_small_contact_store_overflow_goes_through_redo_multi)."""
    for b in range(nb):
        st[i, 64 + 13 * b:67 + 13 * b] = [-0.62, -0.10 + 0.0305 * b, 0.175]
        st[i, 67 + 13 * b:71 + 13 * b] = [0, 0, 0, 1]
        st[i, 71 + 13 * b:77 + 13 * b] = 0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _partition(sch, N, label):
    both = np.concatenate([sch['prone'], sch['free']])
    assert sorted(both.tolist()) == list(range(N)), '%s: the lists do not partition the batch: %s | %s' % (label, sch['prone'], sch['free'])


def check_batch_composition(family, library=None, warm=6, N=N_FULL, planted=PLANTED, near=NEAR, out=print):
    """13 envs stepped `warm` times, give-ups and list-0 envs planted, then ONE step in the batch and in a second env that holds the
    batch reversed without its first three envs: state rows and packed output rows of the ten shared envs equal bit for bit.
    (The emulated twin: 7 envs against 4, no warm-up steps -- a third of the tip targets are put down at the table instead.)"""
    task, kw, recipe = FAMILIES[family]
    joint = bool(kw.get('joint_control'))
    env = _make(library, task, N, kw)
    A, nb = env.dims.action_dim, {'reach': 0, 'push': 1, 'pick_and_place': 1, 'slide': 1}.get(task, kw.get('num_block', 0))
    obs = env.reset()
    rs = np.random.RandomState(11)
    for t in range(warm):
        obs = env.step(_script(rs, N, A, t))[0]
    st = env.get_state().copy()
    if warm == 0:
        st[0::3, 20] = 0.18
    a = _script(rs, N, A, warm)
    planted = list(planted) if recipe else []
    for i in planted:
        if recipe == 'misplan':
            plant_misplan(st, i)
        elif recipe == 'overflow':
            plant_overflow(st, i, obs['observation'][i, :2])
        else:
            plant_tight_row(st, i, nb)
        a[i] = 0
    if nb >= 1 and not joint:
        for i in near:                                     # the object at rest 4 cm (one object: 5 cm, the puck is 3 cm wide) beside the tip target, clear of
            st[i, 64:66] = [st[i, 18] + (0.05 if nb == 1 else 0.04), st[i, 19]]   # the finger boxes (1.25 cm): contact-prone by the plan's rule
            st[i, 67:71] = [0, 0, 0, 1]; st[i, 71:77] = 0
            a[i] = 0
    keep = np.arange(N)[DROPPED:][::-1].copy()             # the batch reversed, without its first three envs
    small = _make(library, task, len(keep), kw)
    small.reset()
    env.set_state(st)
    small.set_state(st[keep])
    r1, r2 = env.step(a), small.step(np.ascontiguousarray(a[keep]))
    s1, s2 = env.get_state(), small.get_state()
    sch1, sch2 = env.handle.schedule(), small.handle.schedule()
    env.close(), small.close()
    out('%-22s %d envs: list 0 %s list 1 %s redo %s | %d envs: list 0 %s list 1 %s redo %s'
        % (family, N, sch1['prone'].tolist(), sch1['free'].tolist(), sch1['redo'].tolist(), len(keep), sch2['prone'].tolist(), sch2['free'].tolist(), sch2['redo'].tolist()))
    _partition(sch1, N, family + ' (full)')
    _partition(sch2, len(keep), family + ' (reversed, shorter)')
    assert (s1[:, 29] == st[:, 29] + 1).all() and (s2[:, 29] == st[keep, 29] + 1).all()      # every env stepped once
    if not joint:
        # (joint control steps one env per wavefront in identity order: the plan runs, no kernel reads its lists)
        for sch in (sch1, sch2):
            assert len(sch['prone']) > 0 and len(sch['free']) > 0, (family, sch)
        assert len(sch1['free']) % 4 != 0 or len(sch2['free']) % 4 != 0      # surplus rows in the last packed wavefront
        # the same env on the same list in either batch (a rule of the env's own state and the task)
        assert set(keep[sch2['prone']].tolist()) == set(sch1['prone'].tolist()) - set(range(DROPPED)), family
    assert sorted(sch1['redo'].tolist()) == planted, (family, sch1['redo'])
    assert sorted(keep[sch2['redo']].tolist()) == planted, (family, sch2['redo'])
    assert np.array_equal(_bits(s1[keep]), _bits(s2)), '%s: state rows differ: %s' % (family, np.nonzero((_bits(s1[keep]) != _bits(s2)).any(1))[0])
    for key in ('observation', 'policy_state', 'achieved_goal', 'desired_goal'):
        assert np.array_equal(_bits(r1[0][key][keep]), _bits(r2[0][key])), (family, key)
    assert np.array_equal(_bits(r1[1][keep]), _bits(r2[1])) and np.array_equal(r1[2][keep], r2[2])
    assert np.array_equal(r1[3]['goal_achieved'][keep], r2[3]['goal_achieved'])
    return sch1, sch2


def check_redo_saturation_reach(library=None, N=9):
    """Every env of a reach batch mis-planned: nine envs on list 1 = three packed wavefronts (the last with three surplus rows), all
    four rows of a wavefront give up in the same substep -- four queue entries from one wavefront -- and the redo list is the batch.
    Bar: test_row_packed_reach_schedule_and_redo's."""
    env = _make(library, 'reach', N, {})
    ora = oracle_lib.OracleEnv('reach', N, seed_base=0, seed_stride=1, threads=8)
    ora.reset()
    env.reset(), ora.reset()
    st = ora.get_state().copy()
    for i in range(N):
        plant_misplan(st, i)
    env.set_state(st), ora.set_state(st)
    z = np.zeros((N, 3), np.float32)
    o = env.step(z)[0]
    oo = ora.step(z)[0]
    sch = env.handle.schedule()
    s1 = env.get_state()
    env.close(), ora.close()
    assert len(sch['prone']) == 0 and sch['free'].tolist() == list(range(N))
    assert sorted(sch['redo'].tolist()) == list(range(N)), sch['redo']
    assert (s1[:, 29] == st[:, 29] + 1).all()
    assert np.abs(o['observation'] - oo['observation']).max() < 5e-5 and (oo['observation'][:, 2] > 0.17).all()


def check_redo_saturation_push(max_or_count, library=None, N=6):
    """Every env of a push batch over the 12-contact row store: six envs = two packed wavefronts, the second half empty; the redo list
    is the batch.  Bars: test_row_packed_object_overflow_goes_through_redo's (max_or_count = its _max_or_count)."""
    env = _make(library, 'push', N, {})
    ora = oracle_lib.OracleEnv('push', N, seed_base=0, seed_stride=1, threads=8)
    o32 = oracle_lib.FloorOracle('push', N, seed_base=0, seed_stride=1, threads=8)
    ora.reset(), o32.reset()
    env.reset(), ora.reset(), o32.reset()
    st = ora.get_state().copy()
    tip = ora.reset(mask=np.zeros(N, bool))['observation'][:, :2]
    for i in range(N):
        plant_overflow(st, i, tip[i])
    env.set_state(st), ora.set_state(st), o32.set_state(st)
    z = np.zeros((N, 3), np.float32)
    env.step(z), ora.step(z), o32.step(z)
    sch = env.handle.schedule()
    se, so, s32 = env.get_state(), ora.get_state(), o32.get_state()
    env.close(), ora.close(), o32.close()
    assert sorted(sch['redo'].tolist()) == list(range(N)) and sorted(sch['free'].tolist()) == list(range(N)), sch
    assert (se[:, 29] == st[:, 29] + 1).all()
    for cols in (slice(0, 9), slice(64, 67)):
        err, spread = np.abs(se[:, cols] - so[:, cols]).max(1), np.abs(s32[:, cols] - so[:, cols]).max(1)
        max_or_count('redo saturation %s' % cols, err, spread)
        assert err.max() < 3 * spread.max() + 1e-3


# ---- either plan, same step: one fresh process per setting of PMG_PLAN_TWO_PASS (pmg_launch_plan reads it once) ----------------------
def plan_child_main(emulated=False, N=67):
    """Run in a child process: reach and push at 67 envs, three steps; prints one hash over states, outputs and schedules."""
    import os
    library = None
    if emulated:
        from pybullet_multigoal_gym_amd._lib import PmgLibrary
        library = PmgLibrary(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu', 'libpmg_emu.so'))
    h = hashlib.sha256()
    for task in ('reach', 'push'):
        env = _make(library, task, N, {})
        env.reset()
        rs = np.random.RandomState(4)
        st = env.get_state().copy()
        st[0::3, 20] = 0.18                                # a third of the tip targets down at the table,
        if task == 'push':
            st[1::5, 64] = st[1::5, 18] + 0.05             # a fifth of the blocks beside the tip target: both lists in use from the first step
            st[1::5, 65] = st[1::5, 19]
        env.set_state(st)
        for t in range(3):
            o, r, d, info = env.step(_script(rs, N, env.dims.action_dim, t))
            sch = env.handle.schedule()
            for arr in (env.get_state(), o['observation'], o['achieved_goal'], r, sch['prone'], sch['free'], np.sort(sch['redo'])):
                h.update(np.ascontiguousarray(arr).tobytes())
            assert len(sch['prone']) > 0 and len(sch['free']) > 0 and len(sch['prone']) + len(sch['free']) == N
        env.close()
    print('PLAN_HASH', h.hexdigest())


def check_either_plan_same_step(emulated=False, N=67, timeout=120):
    """Two fresh child processes, one after the other, PMG_PLAN_TWO_PASS=0 and =1: the same hash."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    hashes = []
    for two_pass in ('0', '1'):
        envv = dict(os.environ, PMG_PLAN_TWO_PASS=two_pass)
        code = 'import sys; sys.path[:0] = [%r, %r]; import schedule_cases as S; S.plan_child_main(%r, %d)' % (os.path.dirname(here), here, emulated, N)
        p = subprocess.run([sys.executable, '-c', code], env=envv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, universal_newlines=True)
        assert p.returncode == 0, p.stdout[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('PLAN_HASH')]
        assert len(lines) == 1, p.stdout[-2000:]
        hashes.append(lines[0])
    assert hashes[0] == hashes[1], hashes
    return hashes
