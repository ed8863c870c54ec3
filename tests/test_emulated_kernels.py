"""CPU tier: the product's HIP device code, compiled for the fiber emulator (tests/emu), against
the oracle.  Checks the kernel LOGIC lane by lane; speed and the real gfx950 build are -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest

import device_cases as D
import oracle_lib as O
import pybullet_multigoal_gym_amd as pmg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


class EmuRunners:
    """the runners of tests/device_cases.py on the emulator build: one host call per case"""

    def __init__(self, emu_library):
        self.lib = lib = C.CDLL(emu_library.path)
        lib.pmge_probe_narrowphase.restype = C.c_int
        lib.pmge_probe_cyl_redo64.restype = C.c_int
        lib.pmge_probe_cyl_amb.restype = C.c_int
        lib.pmge_probe_cyl_redo64_pairs.restype = C.c_int

    def dynamics(self, q, qd, tau):
        n = len(q)
        qdd, mi, tip = np.zeros((n, 9), np.float32), np.zeros((n, 81), np.float32), np.zeros((n, 12), np.float32)
        for i in range(n):
            self.lib.pmge_probe_dynamics(_fp(q[i]), _fp(qd[i]), _fp(tau[i]), _fp(qdd[i]), _fp(mi[i]), _fp(tip[i]))
        return qdd, mi, tip

    def ik(self, q, target):
        out = np.zeros((len(q), 9), np.float32)
        for i in range(len(q)):
            self.lib.pmge_probe_ik(_fp(q[i]), _fp(target[i]), _fp(out[i]))
        return out

    def narrowphase(self, kind, pairs, with_amb=False):
        n, out, amb = np.zeros(len(pairs), np.int32), np.zeros((len(pairs), 40), np.float32), np.full(len(pairs), 1e30, np.float32)
        for i, p in enumerate(np.ascontiguousarray(pairs, np.float32)):
            a = [np.ascontiguousarray(x) for x in D.unpack_pair(p)]
            if with_amb:
                v = C.c_float(0)
                n[i] = self.lib.pmge_probe_cyl_amb(_fp(a[0]), _fp(a[1]), C.c_float(a[2][0]), C.c_float(a[2][2]), _fp(a[3]), _fp(a[4]), _fp(a[5]), C.c_float(0.002),
                                                   _fp(out[i]), C.byref(v))
                amb[i] = v.value
            else:
                n[i] = self.lib.pmge_probe_narrowphase(kind, *[_fp(x) for x in a], C.c_float(0.002), _fp(out[i]))
        return n, out, amb

    def narrowphase_amb(self, kind, pairs):
        assert kind == D.NP_CYL
        return self.narrowphase(kind, pairs, with_amb=True)

    def fk64(self, q9, body):
        p, R = np.zeros((len(q9), 3)), np.zeros((len(q9), 9))
        for i in range(len(q9)):
            self.lib.pmge_probe_fk64(_fp(q9[i]), int(body[i]), _fp(p[i]), _fp(R[i]))
        return p, R

    def cyl_redo64(self, blks, kc):
        n, out = np.zeros(len(blks), np.int32), np.zeros((len(blks), 40), np.float32)
        q9, door = np.zeros(9, np.float32), np.zeros(4, np.float32)
        for i in range(len(blks)):
            n[i] = self.lib.pmge_probe_cyl_redo64(-1, 0, -1, -1, _fp(q9), _fp(blks[i]), _fp(door), _fp(kc), C.c_float(0.03), C.c_float(0.01), _fp(out[i]))
        return n, out

    def redo_pairs(self, ck, ids, q9, blk, doorq, kc, lanes=None):
        n, out = np.zeros(len(ids), np.int32), np.zeros((len(ids), 40), np.float32)
        q9, blk, kc = [np.ascontiguousarray(a, np.float32) for a in (q9, blk, kc)]
        for i, (cyl, box, wall, handed) in enumerate(ids):
            door = np.float32([doorq[i], 0, 0, 0])
            n[i] = self.lib.pmge_probe_cyl_redo64_pairs(int(ck), int(cyl), int(box), int(wall), int(handed), _fp(q9[i]), _fp(blk[i]), _fp(door), _fp(kc),
                                                        C.c_float(D.PUCK_R), C.c_float(D.PUCK_HL), _fp(out[i]))
        return n, out

    def double_maths(self, op, x, y):
        x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
        o0, o1 = np.zeros(len(x)), np.zeros(len(x))
        assert self.lib.pmge_probe_double_maths(op, len(x), _fp(x), _fp(y), _fp(o0), _fp(o1)) == 0
        return o0, o1


@pytest.fixture(scope='module')
def emu_run(emu_library):
    return EmuRunners(emu_library)


def test_device_dynamics_functions_match_oracle(emu_run):
    D.check_dynamics(D.dynamics_cases_basic(), emu_run.dynamics)


def test_device_ik_matches_oracle(emu_run):
    D.check_ik(D.ik_cases_basic(), emu_run.ik)


@pytest.mark.parametrize('task,kw,steps,tol', [
    ('reach', {}, 2, 2e-5),
    ('reach', {'joint_control': True}, 2, 2e-5),
    ('push', {}, 1, 2e-3),
    ('block_stack', {'num_block': 2}, 1, 2e-3),
])
def test_emulated_step_kernel_matches_oracle(emu_library, task, kw, steps, tol):
    N = 1
    env = pmg.make_env(task=task, num_envs=N, seed=3, seed_stride=1, _library=emu_library, **kw)
    ora = O.OracleEnv(task, N, seed_base=3, seed_stride=1, **kw)
    ora.reset()
    o, oo = env.reset(), ora.reset()
    assert np.array_equal(o['desired_goal'], oo['desired_goal'])          # device MT19937 == numpy stream
    assert np.abs(env.get_state() - ora.get_state()).max() < 1e-6
    rs = np.random.RandomState(5)
    for _ in range(steps):
        a = rs.uniform(-1, 1, (N, env.dims.action_dim)).astype(np.float32)
        o, r, d, info = env.step(a)
        oo, ro, do, oko = ora.step(a)
    assert np.abs(env.get_state()[:, :9] - ora.get_state()[:, :9]).max() < tol   # joint angles
    assert np.abs(o['achieved_goal'] - oo['achieved_goal']).max() < tol
    assert np.array_equal(r, ro) and np.array_equal(d, do)
    env.close()


def _pair(emu_library, task, **kw):
    env = pmg.make_env(task=task, num_envs=1, seed=3, seed_stride=1, _library=emu_library, **kw)
    ora = O.OracleEnv(task, 1, seed_base=3, seed_stride=1, **kw)
    ora.reset()
    env.reset(), ora.reset()
    assert np.abs(env.get_state() - ora.get_state()).max() < 1e-6
    return env, ora


def _drive(env, ora, actions):
    for a in actions:
        a = np.float32(a).reshape(1, -1)
        o, r, d, _ = env.step(a)
        oo, ro, do, _ = ora.step(a)
    se, so = env.get_state()[0], ora.get_state()[0]
    assert np.abs(se[:9] - so[:9]).max() < 2e-5                 # joint angles
    assert np.abs(se[64:71] - so[64:71]).max() < 5e-5           # object pose
    assert np.abs(se[71:77] - so[71:77]).max() < 2e-3           # object twist (solver early-exit floor)
    assert np.array_equal(r, ro) and np.array_equal(d, do)
    return so


def test_emulated_slide_puck_matches_oracle(emu_library):
    """cylinder x box narrowphase on the device: the puck resting on the long table (mu 0.05), then pushed by
    the closed fingers (kuka_single_step_base_env.py:53-56,66-69; cylinder_bulk.urdf)."""
    env, ora = _pair(emu_library, 'slide')
    assert np.array_equal(env.reset()['desired_goal'], ora.reset()['desired_goal'])
    st = ora.get_state().copy()
    st[0, 64:67] = [-0.52, 0.045, 0.170]
    env.set_state(st), ora.set_state(st)
    so = _drive(env, ora, [[0, 1, 0], [0, 1, 0]])
    assert so[65] > 0.06 and abs(so[66] - 0.170) < 1e-4        # it moved along +y and stayed on the table
    env.close()


@pytest.mark.parametrize('task,kw,rest_z', [('push', {}, 0.016), ('slide', {}, 0.011), ('block_stack', {'num_block': 2}, 0.016)])
def test_emulated_object_off_the_table_lands_on_the_floor(emu_library, task, kw, rest_z):
    """The robot URDF's base plane (iiwa14_parallel_jaw.urdf:37-58: 5 x 5 x 0.002 m box at the origin, friction 1): an object
    that has left the table lands on it at z = 0.001 + its half height and stays there -- on the emulated kernels as in the
    oracle -- instead of falling for the rest of the episode (rounds 1-5)."""
    env, ora = _pair(emu_library, task, **kw)
    st = ora.get_state().copy()
    edge = (-0.70 if task == 'slide' else -0.52) + (0.5 if task == 'slide' else 0.25)       # the table's +x side wall
    st[0, 64:67] = [edge + 0.04, 0.02, 0.17]
    st[0, 67:71] = [0, 0, 0, 1]; st[0, 71:77] = 0
    env.set_state(st), ora.set_state(st)
    A = env.dims.action_dim
    for t in range(4):
        a = np.zeros((1, A), np.float32)
        o, r, d, _ = env.step(a)
        oo, ro, do, _ = ora.step(a)
    se, so = env.get_state()[0], ora.get_state()[0]
    assert abs(so[66] - rest_z) < 2e-4 and abs(se[66] - rest_z) < 2e-4, (se[64:67], so[64:67])   # at rest on the floor, both
    assert np.abs(se[64:71] - so[64:71]).max() < 5e-5 and np.abs(se[71:77] - so[71:77]).max() < 2e-3
    assert np.abs(se[:9] - so[:9]).max() < 2e-5
    env.close()


@pytest.mark.parametrize('task', ['slide'])
def test_speculative_double_repeat_is_bit_identical_to_the_serial_repeat(emu_library, emu_library_serial_repeat, task):
    """List 0 of slide: three wavefronts per workgroup -- env, float narrowphase, and the finger x puck pairs, which are repeated in
    double whenever they are in contact, computed beside it; the fingers pushing the puck.  States and outputs EQUAL to the build
    that repeats those pairs serially behind the float pass (-DPMG_CYL_SPEC=0, round 5's layout), and the double results are
    really taken (the emulator counts them)."""
    import ctypes as C
    N = 3
    kw = {} if task == 'slide' else {'num_block': 2}
    envs = [pmg.make_env(task=task, num_envs=N, seed=3, seed_stride=1, _library=lib, **kw) for lib in (emu_library, emu_library_serial_repeat)]
    for e in envs:
        e.reset()
    st = envs[0].get_state().copy()
    if task == 'slide':
        st[:, 64] = -0.52 + np.float32([0.0, 0.003, -0.002]); st[:, 65] = 0.045 + np.float32([0.0, -0.002, 0.003]); st[:, 66] = 0.170
        st[:, 67:71] = [0, 0, 0, 1]; st[:, 71:77] = 0
        acts = [[0, 1, 0], [0, 1, 0], [0.3, 1, 0]]
    else:
        acts = [[-1, 0.2 * k, 0.5] for k in (-1, 0, 1, 0, 1)]
    for e in envs:
        e.set_state(st)
    counter = C.CDLL(emu_library.path).pmge_cyl_spec_taken
    counter.restype = C.c_longlong
    before = counter()
    for t, a in enumerate(acts):
        a = np.tile(np.float32(a), (N, 1))
        if task != 'slide':
            a[:, 1] *= np.float32([1.0, 0.5, -1.0])
        outs = [e.step(a) for e in envs]
        assert all(np.array_equal(outs[0][0][k], outs[1][0][k]) for k in outs[0][0])
        assert np.array_equal(envs[0].get_state(), envs[1].get_state())
        if task == 'slide' or t >= 1:
            assert envs[0].handle.schedule()['prone'].size == N         # every env ran on list 0: the three-wavefront kernel
    assert counter() - before > 50                                        # fingers on the puck / gripper base on the door: double results taken
    if task == 'slide':
        assert (envs[0].get_state()[:, 65] > 0.06).all()
    for e in envs:
        e.close()


def test_emulated_gripper_base_contact_matches_oracle(emu_library):
    """gripper-base cylinder (link 7) x block pairs: a block wedged between the open fingers against the palm."""
    env, ora = _pair(emu_library, 'pick_and_place')
    st = ora.get_state().copy()
    st[0, 64:67] = [-0.52, 0.0, 0.25 + 0.0295]
    env.set_state(st), ora.set_state(st)
    so = _drive(env, ora, [[0, 0, 0, 1], [0, 0, -1, 1]])
    assert so[66] > 0.25                                         # held up by the contacts, not in free fall
    env.close()


def test_emulated_stacked_blocks_behind_the_table_run_match_oracle(emu_library):
    """The block x table run is solved in row space (table_run_*), the rows behind it (block x block, finger x block) as LDS
    rows that move the same blocks: a block dropped onto another one, then the closed gripper pressed onto the stack --
    the run's unclamped impulses must be re-derived from the velocity changes at every phase change."""
    env = _make_quiet('block_stack', emu_library, num_block=2, seed=3)
    ora = O.OracleEnv('block_stack', 1, num_block=2, seed_base=3, seed_stride=1)
    ora.reset()
    env.reset(), ora.reset()
    st = ora.get_state().copy()
    st[0, 64:77] = [-0.52, 0.0, 0.175, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]                     # block 0 on the table under the tip
    st[0, 77:90] = [-0.515, 0.004, 0.175 + 0.0305, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]         # block 1 half a millimetre above it, offset
    st[0, 18:21] = [-0.52, 0.0, 0.26]
    env.set_state(st), ora.set_state(st)
    for a in ([0, 0, -1, 1], [0, 0, -1, 1], [0, 0.3, -1, 1]):
        a = np.float32(a).reshape(1, -1)
        o, r, d, _ = env.step(a)
        oo, ro, do, _ = ora.step(a)
    se, so = env.get_state()[0], ora.get_state()[0]
    assert np.abs(se[:9] - so[:9]).max() < 5e-5
    assert np.abs(se[64:71] - so[64:71]).max() < 2e-4 and np.abs(se[77:84] - so[77:84]).max() < 2e-4
    assert so[79] > 0.19                                          # block 1 rests on block 0 (not fallen through, not thrown off)
    env.close()


def test_emulated_object_with_more_contacts_than_the_row_space_solve_holds(emu_library_small_rowspace):
    """One free object, one env per wavefront: up to 16 contacts are solved in row space; beyond that the object x table run
    goes to row space and the rest stays LDS rows built one per lane (object_run_*, build_rows_by_lane).  A build with the
    limit lowered to 4 contacts takes that path as soon as the fingers touch the table next to the object they squeeze."""
    env, ora = _pair(emu_library_small_rowspace, 'pick_and_place')
    st = ora.get_state().copy()
    st[0, 64:67] = [-0.52, 0.0, 0.175]
    st[0, 18:21] = [-0.52, 0.0, 0.176]
    env.set_state(st), ora.set_state(st)
    so = _drive(env, ora, [[0, 0, -1, 1], [0, 0, -1, -1]])             # (a third, sliding step decorrelates in float32 on the LDS-row path, old or new)
    assert abs(so[66] - 0.175) < 5e-3                                  # the object stays on the table between the fingers
    env.close()


def _golden(name):
    import json
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', name)))


@pytest.mark.parametrize('name', ['sampling_block_rearrange3_curriculum', 'sampling_block_stack4_curriculum', 'sampling_push',
                                  'sampling_chest_push2_curriculum'])
def test_emulated_reset_kernel_replays_reference_sampling(emu_library, name):
    """The device reset kernel (MT19937, numpy choice(p=) / choice(replace=False), shuffles, rejection loops, curriculum
    schedule) against what the REFERENCE's own _task_reset / _generate_goal / _generate_curriculum drew for several
    seeds (tests/golden/ref_sampling_*.json, tools/gen_reference_fixtures.py) -- no oracle in between."""
    import ref_replay as R
    fx = R.load(os.path.join(ROOT, 'tests', 'golden', 'ref_%s.json' % name))
    env = R.ProductAdapter(fx, library=emu_library)
    R.replay(fx, env, tol_static=2e-5)
    env.close()


def _make_quiet(task, lib, **kw):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return pmg.make_env(task=task, num_envs=1, seed_stride=1, _library=lib, **kw)


def test_emulated_sub_goals_and_dynamic_goal_match_oracle(emu_library):
    """task_decomposition: set_sub_goal(k) keeps the first k+1 blocks of the order at their targets and every other
    block 'at its goal' wherever it currently is (kuka_multi_step_base_env.py:154-177,309-312), re-derived after
    every step; reward follows the active sub-goal."""
    nb = 3
    env = _make_quiet('block_stack', emu_library, num_block=nb, seed=3, task_decomposition=True)
    ora = O.OracleEnv('block_stack', 1, num_block=nb, seed_base=3, seed_stride=1, task_decomposition=True)
    ora.reset()
    o, oo = env.reset(), ora.reset()
    assert np.array_equal(o['desired_goal'], oo['desired_goal'])          # sub_goal_ind = -1: the full stack
    st = ora.get_state()[0]
    order = st[40:40 + nb].astype(int)
    for k in range(nb):
        g = env.set_sub_goal(k)
        ora.set_sub_goal(k)
        ref = ora.reset(mask=np.zeros(1, bool))['desired_goal']          # re-observe without resetting
        assert np.array_equal(g, ref)
        assert np.array_equal(env.sub_goals[k], ref)
        for i in range(nb):
            b = order[i]
            want = st[48 + 3 * b:51 + 3 * b] if i <= k else st[64 + 13 * b:67 + 13 * b]
            assert np.array_equal(g[0, 3 * b:3 * b + 3], want)
    # with sub-goal 0 active and block order[0] teleported onto its target, the step reports success
    env.set_sub_goal(0), ora.set_sub_goal(0)
    b0 = order[0]
    st2 = ora.get_state().copy()
    st2[0, 64 + 13 * b0:67 + 13 * b0] = st2[0, 48 + 3 * b0:51 + 3 * b0]
    env.set_state(st2), ora.set_state(st2)
    a = np.zeros((1, 4), np.float32)
    o, r, d, info = env.step(a)
    oo, ro, do, oko = ora.step(a)
    assert np.abs(o['desired_goal'] - oo['desired_goal']).max() < 1e-5     # the other blocks' goals track their poses
    assert info['goal_achieved'][0] and oko[0] and r[0] == 0.0 and ro[0] == 0.0
    assert env.set_sub_goal(-1) is not None and not np.array_equal(env.set_sub_goal(-1), o['desired_goal'])
    with pytest.raises(Exception):
        env.set_sub_goal(nb)
    env.close()


def test_emulated_rearrange_step_matches_oracle(emu_library):
    env = _make_quiet('block_rearrange', emu_library, num_block=2, seed=3)
    ora = O.OracleEnv('block_rearrange', 1, num_block=2, seed_base=3, seed_stride=1)
    ora.reset()
    o, oo = env.reset(), ora.reset()
    assert np.array_equal(o['desired_goal'], oo['desired_goal'])
    assert np.abs(env.get_state() - ora.get_state()).max() < 1e-6
    a = np.float32([[0.5, -1.0, 0.3]])
    o, r, d, _ = env.step(a)
    oo, ro, do, _ = ora.step(a)
    assert o['observation'].shape == (1, 8 + 16 * 2) and env.dims.action_dim == 3
    assert np.abs(o['observation'] - oo['observation']).max() < 2e-3
    assert np.abs(o['observation'][0, 3]) == 0 and np.abs(o['observation'][0, 7]) == 0     # no gripper terms (kuka.py:245-246)
    assert np.array_equal(r, ro) and np.array_equal(d, do)
    env.close()


@pytest.mark.parametrize('kw', [dict(task_decomposition=True), dict(use_curriculum=True), dict()])
def test_emulated_grip_informed_goals_match_oracle(emu_library, kw):
    """grip_informed_goal (kuka_multi_step_envs.py:75-77,91-111,143-145): goals carry the gripper-tip target and the
    0.03 finger width; sub-goals come in (pick, place) pairs; the achieved goal appends tip xyz + finger closeness."""
    nb = 3
    env = _make_quiet('block_stack', emu_library, num_block=nb, seed=3, grip_informed_goal=True, **kw)
    ora = O.OracleEnv('block_stack', 1, num_block=nb, seed_base=3, seed_stride=1, grip_informed_goal=True, **kw)
    ora.reset()
    o, oo = env.reset(), ora.reset()
    assert env.dims.goal_dim == 3 * nb + 4 and o['desired_goal'].shape == (1, 13)
    assert np.array_equal(o['desired_goal'], oo['desired_goal'])
    assert np.abs(o['achieved_goal'] - oo['achieved_goal']).max() < 1e-6
    st = ora.get_state()[0]
    order = st[40:40 + nb].astype(int)
    tgt = lambda b: st[48 + 3 * b:51 + 3 * b]
    pos = lambda b: st[64 + 13 * b:67 + 13 * b]
    top = order[nb - 1]
    if kw.get('use_curriculum'):
        lvl = env.last_curriculum_level[0]
        assert np.array_equal(o['desired_goal'][0, 9:12], tgt(order[lvl]))                 # :143
    else:
        assert np.array_equal(o['desired_goal'][0, 9:12], tgt(top))                        # :76 (and sub_goals[-1])
    assert o['desired_goal'][0, 12] == np.float32(0.03)
    if kw.get('task_decomposition'):
        assert env.num_steps == 2 * nb
        subs = env.sub_goals
        for s in range(2 * nb):
            g = env.set_sub_goal(s)
            ora.set_sub_goal(s)
            assert np.array_equal(g, ora.reset(mask=np.zeros(1, bool))['desired_goal']) and np.array_equal(g, subs[s])
            j, pick = s // 2, s % 2 == 0
            for i in range(nb):
                b = order[i]
                assert np.array_equal(g[0, 3 * b:3 * b + 3], tgt(b) if (i < j if pick else i <= j) else pos(b))
            assert np.array_equal(g[0, 9:12], pos(order[j]) if pick else tgt(order[j]))
        with pytest.raises(Exception):
            env.set_sub_goal(2 * nb)
        env.set_sub_goal(0), ora.set_sub_goal(0)
    a = np.float32([[0.2, -0.4, -1.0, 1.0]])
    o, r, d, info = env.step(a)
    oo, ro, do, oko = ora.step(a)
    assert np.abs(o['desired_goal'] - oo['desired_goal']).max() < 1e-4
    assert np.abs(o['achieved_goal'] - oo['achieved_goal']).max() < 1e-4
    assert np.array_equal(r, ro) and np.array_equal(info['goal_achieved'], oko)
    r2, ok2 = env._compute_reward(o['achieved_goal'], o['desired_goal'])                   # HER path with goal_dim 13
    assert np.array_equal(r2, r) and np.array_equal(ok2, info['goal_achieved'])
    env.close()


def test_emulated_row_packed_reach_and_redo(emu_library):
    """Four envs per wavefront for the contact-free reach envs (pmg_packed.h): 6 envs = one full wave + one with
    two live rows; then a misprediction -- an env whose plan entry says 'away from the table' while its fingers
    are 7 mm inside it -- must be caught by the per-substep predicate and recomputed by pmg_k_redo."""
    N = 6
    env = pmg.make_env(task='reach', num_envs=N, seed=3, seed_stride=1, _library=emu_library)
    ora = O.OracleEnv('reach', N, seed_base=3, seed_stride=1)
    ora.reset()
    env.reset(), ora.reset()
    rs = np.random.RandomState(5)
    a = rs.uniform(-1, 1, (N, 3)).astype(np.float32)
    o, r, d, _ = env.step(a)
    oo, ro, do, _ = ora.step(a)
    sch = env.handle.schedule()
    assert len(sch['prone']) == 0 and sorted(sch['free']) == list(range(N)) and len(sch['redo']) == 0
    assert np.abs(o['observation'] - oo['observation']).max() < 2e-5 and np.array_equal(r, ro)
    assert np.abs(env.get_state() - ora.get_state()).max() < 2e-5
    st = ora.get_state().copy()
    q_low, _ = O.ik(st[1, :9].astype(float), [-0.52, 0.0, 0.168])
    st[1, :7] = q_low[:7]; st[1, 9:18] = 0; st[1, 18:21] = [-0.52, 0, 0.30]; st[1, 21:28] = q_low[:7]
    env.set_state(st), ora.set_state(st)
    o, r, d, _ = env.step(np.zeros((N, 3), np.float32))
    oo, ro, do, _ = ora.step(np.zeros((N, 3), np.float32))
    sch = env.handle.schedule()
    assert list(sch['redo']) == [1] and len(sch['prone']) == 0
    assert np.abs(o['observation'] - oo['observation']).max() < 2e-5
    assert np.abs(env.get_state() - ora.get_state()).max() < 5e-5
    assert oo['observation'][1, 2] > 0.17                      # the table pushed the fingers back out
    env.close()


def test_emulated_row_packed_object_tasks_and_overflow_redo(emu_library):
    """push with four envs per wavefront (each row its own 12-contact store): parity with the oracle, then an env the
    plan routes to the packed list (tip TARGET 10 cm from the block) although its closed fingers are touching the
    block on the table -- more than 12 contacts -- must be given up and recomputed by pmg_k_redo_env<1, 24, CYL>."""
    N = 5
    env = pmg.make_env(task='push', num_envs=N, seed=3, seed_stride=1, _library=emu_library)
    ora = O.OracleEnv('push', N, seed_base=3, seed_stride=1)
    ora.reset()
    env.reset(), ora.reset()
    a = np.random.RandomState(5).uniform(-1, 1, (N, 3)).astype(np.float32)
    env.step(a), ora.step(a)
    sch = env.handle.schedule()
    assert len(sch['free']) + len(sch['prone']) == N and len(sch['free']) >= 4 and len(sch['redo']) == 0
    se, so = env.get_state(), ora.get_state()
    assert np.abs(se[:, :9] - so[:, :9]).max() < 2e-5 and np.abs(se[:, 64:71] - so[:, 64:71]).max() < 5e-5
    st = so.copy()
    tipxy = ora.reset(mask=np.zeros(N, bool))['observation'][2, :2]
    st[2, 64:67] = [tipxy[0], tipxy[1] + 0.027, 0.175]          # block against the side of the closed fingers
    st[2, 67:71] = [0, 0, 0, 1]; st[2, 71:77] = 0
    st[2, 18:21] = [tipxy[0], tipxy[1] - 0.10, 0.176]           # ... while the tip target is 10+ cm away
    env.set_state(st), ora.set_state(st)
    z = np.zeros((N, 3), np.float32)
    o, r, d, _ = env.step(z)
    oo, ro, do, _ = ora.step(z)
    sch = env.handle.schedule()
    assert 2 in sch['free'] and list(sch['redo']) == [2]
    se, so = env.get_state(), ora.get_state()
    assert np.abs(se[:, :9] - so[:, :9]).max() < 5e-5 and np.abs(se[:, 64:67] - so[:, 64:67]).max() < 2e-4
    env.close()


@pytest.mark.parametrize('kind', ['box', 'cyl'])
def test_device_narrowphase_matches_oracle_on_random_pairs(emu_run, kind):
    """The HIP narrowphase functions (box_box_fast -> box_box, cyl_box), called directly in the emulator build, against
    the oracle's on randomly oriented pairs in the regime the simulation lives in (brought together until first touch,
    then a little deeper): same number of points, normals, depths and witness points."""
    D.check_random_pairs(kind, emu_run.narrowphase)


def test_device_cyl_box_corner_in_the_side_matches_oracle(emu_run):
    """The product's cyl_box on a box corner touching / inside the cylinder's side (a finger's edge against the puck): the
    planar corner-to-circle distance, as the oracle -- in float32 the coinciding closest points of penetrating shapes are
    1e-8 apart, not 0, so the switch to the radial axis sits at 1 um in both."""
    D.check_corner_in_side(emu_run.narrowphase)


def test_device_box_box_on_cubes_stacked_flush_matches_oracle(emu_run):
    """vertices of the incident face exactly ON the clip planes of the reference face (cubes stacked off-centre with flush
    sides, a cube in the table's corner): four points, the oracle's, from box_box_fast and from the general box_box"""
    assert D.check_flush_stacks(emu_run.narrowphase, D.NP_FAST) > 40
    D.check_flush_stacks(emu_run.narrowphase, D.NP_GENERAL)


def test_axis_aligned_partner_front_end_is_bit_identical(emu_run):
    """The reach kernel's narrowphase instantiation knows that box B (the table) is axis-aligned and leaves the sums with
    exact zeros out of the separating-axis front end: same contacts, same bits as the general routine on fingers in
    random poses over, in and beside a table-sized box."""
    n = D.check_two_routines_bit_identical(D.axis_aligned_cases(), emu_run.narrowphase, D.NP_FAST_ALIGNED, D.NP_GENERAL)
    hit = int((n > 0).sum())
    assert hit > 250, hit


def test_face_clip_is_bit_identical_to_the_general_box_box_routine(emu_run):
    """box_box_fast serves a face contact whose incident face is NOT inside the reference face (a finger on a cube, cubes
    stacked off-centre) with box_face_clip: clip passes over all vertices at once, batched LDS traffic.  It must return
    exactly what the general routine (box_box: vertex-by-vertex Sutherland-Hodgman through the workspace) returns -- same
    points, same order, same bits -- on fingers against cubes, cubes on cubes and cubes on a table-sized box, in random
    orientations, touching, deeper and with more than four clipped vertices inside the margin."""
    lib = emu_run.lib
    lib.pmge_face_clip_count.restype = C.c_longlong
    calls0 = lib.pmge_face_clip_count()
    n = D.check_two_routines_bit_identical(D.face_clip_cases(), emu_run.narrowphase, D.NP_FAST, D.NP_GENERAL)
    clipped, many = int((n > 0).sum()), int((n == 4).sum())
    assert clipped > 300 and many > 100, (clipped, many)
    assert lib.pmge_face_clip_count() - calls0 > 250          # the new path is what answered


@pytest.mark.parametrize('nb,frac_down', [(0, 0.3), (1, 0.05), (1, 0.4)])
def test_two_pass_plan_writes_the_same_lists_as_the_single_workgroup_plan(built, nb, frac_down):
    """Batches beyond 65 536 envs are planned by ceil(N / 1024) workgroups in two passes (pmg_k_plan_count /
    pmg_k_plan_scatter).  On a batch both plans can take (3 000 envs = three workgroups, the last one ragged) they must
    write identical launch lists and counts -- for reach, and for one free object with few / many envs down at the
    table (the promotion rule decided from the grand totals, on either side of its threshold)."""
    import ctypes as C
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'emu', 'libpmg_emu.so'))
    N, adim = 3000, 3
    rs = np.random.RandomState(nb * 7 + int(frac_down * 100))
    hot = np.zeros((N, 32), np.float32)
    hot[:, 18] = rs.uniform(-0.67, -0.37, N); hot[:, 19] = rs.uniform(-0.2, 0.2, N)
    hot[:, 20] = np.where(rs.uniform(0, 1, N) < frac_down, 0.175 + rs.uniform(0, 0.01, N), rs.uniform(0.19, 0.5, N))
    blocks = np.zeros((N, 13 * max(nb, 1)), np.float32)
    blocks[:, 0] = rs.uniform(-0.64, -0.40, N); blocks[:, 1] = rs.uniform(-0.15, 0.15, N); blocks[:, 2] = 0.175; blocks[:, 6] = 1
    near = rs.uniform(0, 1, N) < 0.1                       # some grippers right at their object: class 0
    hot[near, 18:21] = blocks[near, 0:3] + np.float32([0.0, 0.0, 0.02])
    actions = rs.uniform(-1, 1, (N, adim)).astype(np.float32)
    out, flags = [], []
    for two_pass in (0, 1):
        sc = np.full(3 + 3 * N, -7, np.int32)
        rc = lib.pmge_probe_plan(C.c_int(N), C.c_int(nb), hot.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p),
                                 actions.ctypes.data_as(C.c_void_p), C.c_int(adim), C.c_int(1536), C.c_int(two_pass),
                                 sc.ctypes.data_as(C.c_void_p))
        assert rc in (0, 1)
        out.append(sc)
        flags.append(rc)
    a, b = out
    # the promotion flag (list 0 takes issue priority when the fingers-down class was moved there): same in both plans,
    # set exactly for one object with few envs down at the table
    assert flags[0] == flags[1] == (1 if (nb == 1 and frac_down < 0.125) else 0)
    n0, n1 = int(a[0]), int(a[1])
    assert n0 + n1 == N and (n0, n1) == (int(b[0]), int(b[1])) and 0 < n0 < N
    assert np.array_equal(a[2:2 + n0], b[2:2 + n0]) and np.array_equal(a[2 + N:2 + N + n1], b[2 + N:2 + N + n1])
    assert a[2 + 2 * N] == 0 and b[2 + 2 * N] == 0
    assert sorted(np.concatenate([b[2:2 + n0], b[2 + N:2 + N + n1]]).tolist()) == list(range(N))    # a partition of the batch


@pytest.mark.parametrize('task', ['push', 'pick_and_place', 'slide'])
def test_emulated_sharded_batch_is_bit_identical_to_the_unsharded_batch(emu_library, task):
    """The product's kernels on the emulator: 24 envs in one batch against 3 shards of 8, half of the batch with its fingers
    driven onto the table (the class whose kernel depended on batch-wide counts until round 5) -- outputs and state rows EQUAL
    (tests/test_gpu_parity.py runs the same at 512 / 2 and 4096 / 8 on the device)."""
    from test_gpu_parity import _sharded_equals_unsharded
    _sharded_equals_unsharded(emu_library, task, 24, 3, 4)


def test_double_forward_kinematics_of_the_contact_links_matches_the_oracle(emu_run):
    """fk64_link (the double poses cyl_redo64 takes for the gripper base and the fingers, from float32 joint angles) against
    the float64 oracle's kinematics() through its Bullet-call-level world: link frames of Bullet links 12 / 13 / 15."""
    D.check_fk64(emu_run.fk64)


def test_double_repeat_of_a_cylinder_pair_is_the_float64_oracle(emu_run):
    """cyl_redo64 (cyl_box<double> on poses re-derived in double from the float32 state) against the float64 oracle's cyl_box on
    the same poses: the slide puck -- any small tilt, any yaw -- against the table and near its edge.  Same count, points and
    normals to 1e-6 (the outputs are float32), depths to 1e-8.  Beside it the float32 pass on float32 poses: its gross
    disagreements with the oracle are counted (the resting puck has none: the repeat is for vertex / edge contacts)."""
    D.check_cyl_redo64(emu_run.cyl_redo64, emu_run.narrowphase_amb)


@pytest.mark.parametrize('ck', [-1, 0, 1])
def test_double_repeat_matches_the_oracle_on_every_pair_it_serves(emu_run, ck):
    """cyl_redo64<ck> on all six kinds of pair collide() hands it -- gripper base x cube (state row 1), puck x finger 1 / 2, puck x
    floor and table side wall; per chest kind handle x finger 1 / 2, gripper base x door / lid and x EVERY wall, the door joint
    at 0, at its limit and between, the arm's pose through q9 from the oracle's IK -- against the float64 oracle's cyl_box on
    operands assembled from the oracle's link states and tests/golden/model.json: the oracle's count in every case, normals and
    points to 1e-6, depths to 1e-8 (the g++ build measures at most 3.1e-7 / 1.5e-9 / 1.2e-7 over its 1682 cases); coverage per row asserted.  The same
    cases with the robot body's pose handed in (spec_fk's way: sincos64 per joint, fk64_chain with the table): the same bars and
    the same bits"""
    D.check_redo_pairs(ck, emu_run.redo_pairs, handed_bits=True)
    if ck >= 0:
        D.check_mirror_walls_are_told_apart(ck)


def test_float_pass_matches_the_oracle_on_the_shapes_of_every_cylinder_pair(emu_run):
    """cyl_box<float> had met the puck against a cube and the table: here the gripper base (0.05 / 0.02) against a cube, the thin
    door, the lid and both wall boxes, the two handles (0.005 / 0.01 and 0.005 / 0.025, longer than wide) and the puck against
    the finger box -- 160 first-touch cases each, the strict narrowphase bars, pairs the oracle's own float32 mode cannot hold
    set aside and capped at 1 % (4 of 1280; the g++ build's largest errors on the rest: 2.0e-5 normal, 4.7e-7 depth, 4.5e-7 points)"""
    D.check_float_shapes(emu_run.narrowphase)


def test_double_sine_and_cosine_hold_their_error_on_every_joint_angle(emu_run):
    """sincos64 (shared code: what the device runs) against numpy on every float32 joint angle of the cases above -- limits,
    quadrant switch points, multiples of pi / 2, each one float32 step up and down -- and 4096 random angles in [-3.06, 3.06]:
    absolute error < 1e-15 (measured 1.1e-16).  Angles beyond 3.06 are not what the routine is for.  t_sqrt / t_div are the plain operations in
    this build, exact by IEEE: only the gfx950 build (-m gpu) tests the Newton sequences"""
    D.check_sincos64(emu_run.double_maths)
    es, ed = D.check_sqrt_div64(emu_run.double_maths)
    assert es <= 2.0 ** -52 and ed <= 2.0 ** -52
