"""Cases and checks of the ONE-SUBSTEP tests (tests/test_substep_emulated.py on the emulator, tests/test_gpu_substep.py on the
device) -- TEST INFRASTRUCTURE.

A one-substep build of the product (-DPMG_RUN_SIM_STEPS=1 -DPMG_RUN_SUBSTEPS=1) runs one substep() per env step.  After one
substep there is no contact chaos yet, so every kernel form of the contact solve can be held to the float64 oracle (run with
its `sim_steps` = `substeps` = 1 switches) case by case, at a bar that comes from the oracle alone: four times the worst distance
of the FLOAT32 build of the oracle from the float64 build on the same cases, per task and column group, never below 1e-6.

A case is a float32 state row plus an action row whose arm part is zero.  Every env runs joint_control=True: the motion sits
in the state's joint-target columns (21:28) and in the finger target, so the oracle and every build start from bit-equal motor
targets (under tip control the float32 and float64 IK results differ by ~1e-5 rad, which the stiff motor row turns into ~5e-3
rad/s).  The one exception to "zero action": the grasping tasks take the finger target from the action's last entry
(kuka.py:171), so that entry carries the finger command of the harvested scene (-1, 0 or 1: an exact float32 in every build).

The cases are harvested from the float64 oracle, deterministically: rollouts of tools/scripted_policies.py under tip control
(grasp, lift, carry, push, stack, open the door, drop in) are cut at chosen env steps, the next tip target is turned into joint
targets by the oracle's IK, and the scene is carried a few substeps INTO the next env step (SubstepOracle(substeps=k)) so that
the bodies move; the suite's constructed scenes are treated the same way.  Half of the cases get small random sliding and
spinning velocities on the free bodies so that the friction rows act.

Under joint control the launch plan keeps every env with several blocks on list 0.  The list-1 kernels of several blocks are
reached by the `<task>/away` sets instead: tip control, the gripper away from every free body, free-body and door columns
only (_away_cases).
"""
import functools
import os
import re
import sys
import warnings

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import scripted_policies as SP  # noqa: E402

FLOOR = 1e-6            # float32 rounding of the velocity increments: the bar of a group whose oracle spread is zero
FACTOR = 4.0            # 1-ulp rcp / sqrt, 2.5-ulp division, contracted multiply-adds against 0.5 ulp per operation (test_gpu_device_functions.py)
BATCH = 64              # envs per batch, at most
RESIDUAL_THRESHOLD = 1e-7
LEFT_OUT_CAP = 0.02     # share of a task's cases that may be left out (device / emulator)
LEFT_OUT_CAP_F32 = 0.01 # ... of the case set itself: what the float32 oracle may leave out

_MODEL = open(os.path.join(ROOT, 'include', 'pmg_model.h')).read()


def _model_list(name):
    return [float(x) for x in re.search(r'#define %s \{([^}]*)\}' % name, _MODEL).group(1).split(',')]


def _model_int(name):
    return int(re.search(r'#define %s (\d+)' % name, _MODEL).group(1))


JLO, JHI = np.array(_model_list('PMG_JLO')), np.array(_model_list('PMG_JHI'))
FINGERS = (100 + _model_int('PMG_BL_FINGER1'), 100 + _model_int('PMG_BL_FINGER2'))      # body ids of the oracle's contact list
GBASE = 100 + _model_int('PMG_BL_GBASE')
STATIC, DOOR = -1, 50

# name -> (task, its options).  nb = 2 ... 5 blocks: the four instantiations of the multi-block kernels
TASKS = {
    'reach': ('reach', {}),
    'push': ('push', {}),
    'slide': ('slide', {}),
    'pick_and_place': ('pick_and_place', {}),
    'block_stack2': ('block_stack', {'num_block': 2}),
    'block_stack3': ('block_stack', {'num_block': 3}),
    'block_stack4': ('block_stack', {'num_block': 4}),
    'block_rearrange5': ('block_rearrange', {'num_block': 5}),
    'chest_push2': ('chest_push', {'num_block': 2}),
    'chest_pick_and_place1': ('chest_pick_and_place', {'num_block': 1}),
}
# ... and the sets that run under TIP control with the gripper away from every free body (name + '/away', see away_cases)
EXTRA_TASKS = {'chest_push5': ('chest_push', {'num_block': 5})}
AWAY = ['push/away', 'slide/away', 'block_stack2/away', 'block_stack3/away', 'block_stack4/away', 'block_rearrange5/away', 'chest_push2/away', 'chest_push5/away']
GRASPING = ('pick_and_place', 'block_stack', 'chest_pick_and_place')


def _base(name):
    return name[:-5] if name.endswith('/away') else name


def _joint(name):
    return not name.endswith('/away')


def _task(name):
    return dict(TASKS, **EXTRA_TASKS)[_base(name)]


def num_blocks(name):
    task, kw = _task(name)
    return 0 if task == 'reach' else kw.get('num_block', 1)


def action_dim(name):
    return (7 if _joint(name) else 3) + (_task(name)[0] in GRASPING)


def groups(name):
    """column groups of the state row: velocities, then the positions they integrate to"""
    nb, chest = num_blocks(name), _task(name)[0].startswith('chest')
    blk = lambda lo, hi: np.concatenate([np.arange(64 + 13 * b + lo, 64 + 13 * b + hi) for b in range(nb)]) if nb else np.zeros(0, int)
    g = {'qd': np.arange(9, 18), 'q': np.arange(0, 9)}
    if nb:
        g.update({'lin vel': blk(7, 10), 'ang vel': blk(10, 13), 'pos': blk(0, 3), 'quat': blk(3, 7)})
    if chest:
        g.update({'door qd': np.array([49]), 'door q': np.array([48])})
    if not _joint(name):                    # tip control: the IK's float32 / float64 difference buries the arm's columns
        del g['qd'], g['q']
    return g


VELOCITY_GROUPS = ('qd', 'lin vel', 'ang vel', 'door qd')


# ----------------------------------------------------------------------------------------------------------------------
# harvesting
def _oracle(name, n, cls=O.OracleEnv, joint=False, **extra):
    joint = joint and _joint(name)
    task, kw = _task(name)
    ora = cls(task, n, seed_base=11, seed_stride=1, joint_control=joint, max_episode_steps=1000, **dict(kw, **extra))
    ora.reset(), ora.reset()
    return ora


def _joint_targets(st, act):
    """the next tip target of a tip-control scene as joint targets: the oracle's IK from the scene's own joint angles"""
    jt = np.zeros((len(st), 7), np.float32)
    for i in range(len(st)):
        tip = np.clip(st[i, 18:21].astype(float) + 0.01 * act[i, :3], SP.TIP_LOW, SP.TIP_HIGH)
        jt[i] = O.ik(st[i, :9].astype(float), tip)[0][:7]
    return jt


def _rollout(name, n, T, cuts, policy_kw=None):
    """the scripted policy of the task on the float64 oracle under tip control -> (states, tip-control actions) before the env
    steps `cuts`"""
    task, kw = _task(name)
    ora = _oracle(name, n, threads=O.usable_threads())
    pkw = dict(policy_kw or {})
    if task.startswith(('block', 'chest')):
        pkw.setdefault('num_block', kw['num_block'])
    pol = SP.make_policy(task, n, **pkw)
    obs = ora.reset(mask=np.zeros(n, bool))
    S, A = [], []
    for t in range(T):
        a = pol.act(obs)
        if t in cuts:
            S.append(ora.get_state().copy()), A.append(a.copy())
        obs = ora.step(a)[0]
    ora.close()
    return np.concatenate(S), np.concatenate(A)


def _as_joint_cases(name, st, act):
    """tip-control scenes (state, action) -> joint-control cases: joint targets from the IK, the finger command kept"""
    st = st.copy()
    st[:, 21:28] = _joint_targets(st, act)
    ja = np.zeros((len(st), action_dim(name)), np.float32)
    if _task(name)[0] in GRASPING:
        ja[:, -1] = np.sign(act[:, -1])
    return st, ja


def _advance(name, st, ja, ks):
    """carry case i `ks[i]` substeps into its env step on the float64 oracle (joint control, the case's own action)"""
    out = st.copy()
    for k in sorted(set(ks)):
        idx = np.nonzero(np.asarray(ks) == k)[0]
        if k == 0:
            continue
        for lo in range(0, len(idx), BATCH):
            sel = idx[lo:lo + BATCH]
            ora = _oracle(name, len(sel), cls=O.SubstepOracle, joint=True, substeps=int(k))
            ora.set_state(st[sel])
            ora.step(ja[sel])
            out[sel] = ora.get_state()
            ora.close()
    out[:, 29] = 0                                                      # (elapsed: episodes never end here)
    return out


def _stir(name, st, rs, share=0.5):
    """small random sliding and spinning velocities on the free bodies of a share of the cases: the friction rows act"""
    nb = num_blocks(name)
    for i in np.nonzero(rs.uniform(0, 1, len(st)) < share)[0]:
        for b in range(nb):
            o = 64 + 13 * b
            st[i, o + 7:o + 9] += rs.uniform(-0.03, 0.03, 2).astype(np.float32)
            st[i, o + 10:o + 13] += (rs.uniform(-1, 1, 3) * [0.2, 0.2, 1.0]).astype(np.float32)
    return st


def _scene_states(name, n, edit):
    """n reset states of the task, edited in place by `edit(st)`"""
    ora = _oracle(name, n)
    st = ora.get_state().copy()
    ora.close()
    edit(st)
    return st


def _lower(st, i, xyz, press=0.0):
    """env i's arm to the tip position xyz (the oracle's IK), at rest; joint targets `press` below it"""
    q = O.ik(st[i, :9].astype(float), list(xyz))[0]
    st[i, :7] = q[:7]
    st[i, 9:18] = 0
    st[i, 18:21] = xyz
    tgt = O.ik(q, [xyz[0], xyz[1], xyz[2] - press])[0] if press else q
    st[i, 21:28] = tgt[:7]


def _blocks_at(st, i, poses):
    for b, p in enumerate(poses):
        st[i, 64 + 13 * b:77 + 13 * b] = list(p) + [0, 0, 0, 1, 0, 0, 0, 0, 0, 0]


def _yaw(st, i, b, ang):
    st[i, 64 + 13 * b + 3:64 + 13 * b + 7] = [0, 0, np.sin(ang / 2), np.cos(ang / 2)]


def _constructed(name, rs):
    """the suite's constructed scenes of the task, as (states, joint-control actions) at rest"""
    task, kw = _task(name)
    nb = num_blocks(name)
    A = action_dim(name)
    n = 24
    grip = np.zeros(n, np.float32)

    def edit(st):
        if task == 'reach':
            for i in range(n):
                x, y = rs.uniform(-0.60, -0.44), rs.uniform(-0.15, 0.15)
                if i < 8:                   # both fingers on / in the table (3 mm inside ... 1.5 mm above: both branches of the rhs)
                    _lower(st, i, [x, y, 0.1715 + 0.0006 * i], press=0.01 * (i % 2))
                elif i < 16:                # wrist rolled: one finger lower than the other
                    _lower(st, i, [x, y, 0.1745 + 0.0004 * (i - 8)])
                    st[i, 5] += (-1) ** i * rs.uniform(0.05, 0.20)
                    st[i, 21:28] = st[i, :7]
                elif i < 20:                # a joint beyond its limit (lim_active), fingers included
                    st[i, 6] = JHI[6] + 0.003 if i % 2 else JLO[6] - 0.002
                    st[i, 7:9] = [0.0355, -0.0004]
                    st[i, 21:28] = st[i, :7]
                st[i, 9:16] += rs.uniform(-0.05, 0.05, 7).astype(np.float32) * (i % 4 != 3)       # (most of them moving: the fingers slide)
        elif nb == 1 and not task.startswith('chest'):
            z_obj = 0.170 if task == 'slide' else 0.175
            side = 0.045 if task == 'slide' else 0.027
            for i in range(n):
                x, y = rs.uniform(-0.58, -0.46), rs.uniform(-0.12, 0.12)
                if i < 8:                   # closed fingers down at the table beside the object: push contact (slide_push / the redo scene of push)
                    _lower(st, i, [x, y, 0.1745 + 0.0004 * (i % 4)], press=0.004 * (i % 2))
                    _blocks_at(st, i, [[x + rs.uniform(-0.003, 0.003), y + side + rs.uniform(-0.001, 0.002), z_obj]])
                    if task != 'slide':
                        _yaw(st, i, 0, rs.uniform(-0.3, 0.3) * (i % 2))
                    st[i, 21:28] = O.ik(st[i, :9].astype(float), [x, y + 0.01, st[i, 20]])[0][:7]      # pushing along +y
                elif i < 14:                # the object between the open fingers that come down on the table around it and close
                    _lower(st, i, [x, y, 0.1745 + 0.0004 * (i % 3)], press=0.003 * (i % 2))
                    st[i, 7:9] = 0.0145 + 0.0015 * (i % 4) if task != 'slide' else 0.034
                    _blocks_at(st, i, [[x, y + (0.0 if task != 'slide' else 0.055), z_obj]])
                    if task != 'slide':
                        _yaw(st, i, 0, rs.uniform(-0.05, 0.05))
                    grip[i] = 1.0
                    st[i, 28] = 0.0
                elif i < 17:                # palm_block: the object wedged between the open fingers against the gripper base
                    if task != 'pick_and_place':
                        continue
                    _blocks_at(st, i, [[st[i, 18] + 0.002 * (i - 14), st[i, 19], st[i, 20] + 0.0295]])
                    grip[i] = 1.0
                elif i < 20:                # off the table: on the floor plane of the robot's base
                    edge = (-0.70 if task == 'slide' else -0.52) + (0.5 if task == 'slide' else 0.25)
                    _blocks_at(st, i, [[edge + 0.04 + 0.01 * (i - 17), 0.02, (0.011 if task == 'slide' else 0.016) + 0.0003 * (i - 18)]])
                else:                       # gripper high and far: object x table only, tilted a little so that corners differ
                    _lower(st, i, [x, y, 0.36])
                    _blocks_at(st, i, [[x + 0.13 * (1 if x < -0.52 else -1), -y, z_obj + 0.0004 * (i - 21)]])
        elif not task.startswith('chest'):
            for i in range(n):
                x, y = rs.uniform(-0.56, -0.48), rs.uniform(-0.06, 0.06)
                if i < 6:                   # a stack: block 1 on block 0 (no table contact between two that have one), gripper pressing / near / far
                    poses = [[x, y, 0.175], [x + 0.005, y + 0.004, 0.2052 + 0.0003 * (i % 3)]]
                    poses += [[x + 0.09 * (b - 1) * (-1) ** b, y + 0.07 * (-1) ** b, 0.175] for b in range(2, nb)]
                    _blocks_at(st, i, poses)
                    _lower(st, i, [x, y, [0.2352, 0.26, 0.40][i % 3]], press=0.004 if i % 3 == 0 else 0.0)
                    grip[i] = 1.0
                elif i < 10:                # the blocks pushed together into a row (block x block rows behind the table runs)
                    _blocks_at(st, i, [[-0.45, -0.09 + (0.0302 + 0.0004 * (i - 6)) * b, 0.175] for b in range(nb)])
                    _lower(st, i, [-0.60, 0.1, 0.40] if i % 2 else [-0.45, -0.09 - 0.03, 0.1765])
                    if task == 'block_stack':
                        grip[i] = 1.0
                    if i % 2 == 0:
                        st[i, 21:28] = O.ik(st[i, :9].astype(float), [-0.45, -0.08, 0.1765])[0][:7]    # the closed fingers push the row's end
                elif i < 14:                # the gripper holds block 0 in the air above the others
                    if task != 'block_stack':
                        _blocks_at(st, i, [[-0.62 + 0.06 * b, 0.12 * (-1) ** b, 0.175] for b in range(nb)])
                        continue
                    _blocks_at(st, i, [[x, y, 0.24]] + [[-0.62 + 0.05 * b, 0.1 * (-1) ** b, 0.175] for b in range(1, nb)])
                    _lower(st, i, [x, y, 0.24])
                    st[i, 7:9] = 0.0148
                    grip[i] = 1.0
                # else: the reset scene, blocks apart on the table (table runs only)
        else:
            handle = task == 'chest_push'
            for i in range(n):
                if i < 4:                   # the door / lid beyond its lower limit, at rest and moving
                    st[i, 48] = -0.0005 * i
                    st[i, 49] = 0.0 if i % 2 else -0.01
                elif i < 8:                 # beyond its upper limit; latched motor on half of them
                    st[i, 48] = (0.12 if handle else 0.10) + 0.002 * (i - 4)
                    st[i, 49] = 0.02 * (i % 2)
                    st[i, 50] = float(i >= 6)
                elif i < 12:                # open and latched: the motor row alone
                    st[i, 48] = (0.115 if handle else 0.095) - 0.004 * (i - 8)
                    st[i, 49] = 0.01
                    st[i, 50] = 1.0
                elif i < 16 and handle:     # a block against the chest's front wall / the door box, on the table
                    _blocks_at(st, i, [[-0.592 + 0.0152 + 0.0004 * (i - 12), -0.03 + 0.02 * (i - 12), 0.175]] +
                               [[-0.45, 0.1 * (-1) ** b, 0.175] for b in range(1, nb)])
                    st[i, 64 + 7] = -0.02
        return st

    st = _scene_states(name, n, edit)
    for b in range(nb):                     # no two faces exactly parallel: a little yaw and a fraction of a millimetre on every free body
        o = 64 + 13 * b
        ang = rs.uniform(-0.02, 0.02, n)
        still = (st[:, o + 3:o + 6] == 0).all(1)
        st[still, o + 5], st[still, o + 6] = np.sin(ang / 2)[still], np.cos(ang / 2)[still]
        st[:, o:o + 2] += rs.uniform(-2e-4, 2e-4, (n, 2)).astype(np.float32)
    ja = np.zeros((n, A), np.float32)
    if task in GRASPING:
        ja[:, -1] = grip
    return st, ja


# what the rollouts are cut at: the phases of the scripted policies (tools/scripted_policies.py)
ROLLOUTS = {
    'reach': (8, 12, range(2, 12, 3)),
    'push': (12, 44, range(6, 44, 5)),
    'slide': (12, 44, range(6, 44, 5)),
    'pick_and_place': (12, 40, range(4, 40, 4)),
    'block_stack2': (8, 100, range(8, 100, 7)),
    'block_stack3': (8, 140, range(8, 140, 10)),
    'block_stack4': (8, 180, range(8, 180, 13)),
    'block_rearrange5': (8, 60, range(6, 60, 6)),
    'chest_push2': (8, 110, range(5, 110, 8)),
    'chest_pick_and_place1': (8, 90, list(range(3, 21, 2)) + list(range(24, 90, 11))),
}


@functools.lru_cache(maxsize=None)
def cases(name):
    """-> (states [M, state_dim] float32, actions [M, 7 or 8] float32), both read-only; deterministic"""
    rs = np.random.RandomState(sum(map(ord, name)))
    if not _joint(name):
        st, ja = _away_cases(name, rs)
        st.setflags(write=False), ja.setflags(write=False)
        return st, ja
    n, T, cuts = ROLLOUTS[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        st_r, ja_r = _as_joint_cases(name, *_rollout(name, n, T, set(cuts)))
        st_c, ja_c = _constructed(name, rs)
    st, ja = np.concatenate([st_r, st_c]), np.concatenate([ja_r, ja_c])
    ks = rs.choice([1, 2, 3, 5, 8, 13, 30], len(st))                    # (at least one: a scene exactly as built has bodies EXACTLY flush)
    st = _stir(name, _advance(name, st, ja, ks), rs)
    assert np.isfinite(st).all()
    # scenes no simulation reaches are dropped, by the float64 oracle alone: a penetration deeper than MAX_DEPTH (the ERP row
    # ejects it at depth x 0.9 / 0.002 s: 2 m/s and more) makes the substep violent, and the absolute float32 error with it
    depth, corner = _deepest(name, st, ja)
    st, ja = st[(depth <= MAX_DEPTH) & ~corner], ja[(depth <= MAX_DEPTH) & ~corner]
    st.setflags(write=False), ja.setflags(write=False)
    return st, ja


def _away_cases(name, rs):
    """Cases under TIP control, for the kernels the launch plan never picks under joint control (several blocks on list 1: the
    small contact store with its redo pass, the chest's ranked stage slots and their overflow).  Only cases in which no row
    joins the robot and a free body (no finger / gripper base on a block or on the door): the arm's motor targets then come
    from the IK, whose float32 / float64 difference reaches the arm's columns alone, and the free bodies and the door are held
    to the oracle at their own bars (groups() leaves `qd` and `q` out).  The joint-control cases of the task that qualify, and
    the blocks pushed together into rows with the gripper far away: rows of 28 ... 36 contacts, on either side of the 30 the
    small store holds (rows on a knife edge of the narrowphase are not taken: judged by the two oracle builds, so the float32
    oracle's left-out cap of check_case_set is not informative for those rows).  One object: see below."""
    base, nb, A = _base(name), num_blocks(name), action_dim(name)
    grasp = _task(name)[0] in GRASPING
    S, J = [], []
    if base in TASKS:
        st, ja = cases(base)
        keep = ~tags(base)['robot x free body']
        S.append(st[keep])
        J.append(np.concatenate([np.zeros((keep.sum(), 3), np.float32), ja[keep, -1:]], 1) if grasp else np.zeros((keep.sum(), 3), np.float32))
    if nb == 1:
        # One object, four envs per wavefront (pmgp::step_group_obj, 12 contacts per row).  (a) the closed fingers down on the table
        # away from the object: 4 + 8 = 12 contacts, the full store, kept on list 1;  (b) MISPREDICTED envs: the fingers at the
        # object (13 and more contacts) while the tip TARGET is far away, so the plan sends them to list 1 and the kernel must give
        # them up to pmg_k_redo_env<1, 24, CYL>.  In (b) the arm and the object share rows: those cases are `coupled` (reference()),
        # held to the oracle's contact count, the redo flag and the bits of the full-store kernel, not to the bars
        n = 24
        obj_z = 0.170 if base == 'slide' else 0.175

        def edit(st):
            for i in range(n):
                x, y = rs.uniform(-0.58, -0.46), rs.uniform(-0.12, 0.12)
                _lower(st, i, [x, y, 0.1738 + 0.0003 * (i % 8)], press=0.003 * (i % 2))
                _blocks_at(st, i, [[x + rs.uniform(-0.02, 0.02), y + (0.10 + 0.002 * i) * (1 if y < 0 else -1), obj_z]])
                st[i, 9:16] += rs.uniform(-0.05, 0.05, 7).astype(np.float32) * (i % 4 != 3)
        st1 = _scene_states(name, n, edit)
        S.append(_advance(name, st1, np.zeros((n, A), np.float32), rs.choice([1, 2, 3, 5], n))), J.append(np.zeros((n, A), np.float32))
        t = tags(base)
        hit = np.nonzero(t['finger x object'] & (reference(base)['info']['nc'] >= 13))[0][:16]
        st2 = st[hit].copy()
        side = np.where(st2[:, 65] < 0, 1.0, -1.0)
        st2[:, 18], st2[:, 19], st2[:, 20] = st2[:, 64], st2[:, 65] + np.float32(0.13) * side, np.float32(0.25)
        S.append(st2), J.append(np.zeros((len(hit), A), np.float32))
    if nb >= 4:
        n = 192

        def edit(st):
            for i in range(n):
                gap = 0.0300 + rs.uniform(0.0, 0.0022, nb)
                y = -0.09 + np.cumsum(gap) - gap[0]
                _blocks_at(st, i, [[-0.45 + rs.uniform(-3e-4, 3e-4), y[b], 0.175] for b in range(nb)])
                for b in range(nb):
                    _yaw(st, i, b, rs.uniform(-0.06, 0.06))
                if i % 2:                   # the first block tipped onto a corner: three of its corners inside the margin -> odd counts
                    tx, ty = rs.uniform(0.022, 0.036, 2)
                    q = np.array([tx / 2, ty / 2, 0.0, 1.0])
                    st[i, 67:71] = q / np.linalg.norm(q)
                    st[i, 66] += 0.02 * (tx + ty)
                _lower(st, i, [-0.60, 0.12, 0.40])
                if i % 3 == 0:              # the tip TARGET at the row while the arm is still away: list 0, and still no row joins arm and blocks
                    st[i, 18:21] = [-0.45, y[nb // 2], 0.21]
        st = _scene_states(name, n, edit)
        ja = np.zeros((n, A), np.float32)
        st = _advance(name, st, ja, rs.choice([1, 2, 3], n))
        # Not the rows on a knife edge of the narrowphase: the two oracle builds disagree on the count, or on a contact point by
        # 0.1 mm.  (Moving the blocks by micrometres on the float64 oracle alone does not find them all: the float32 build's own
        # error in a yawed box pair is larger.)  For these constructed rows check_case_set's cap on what the float32 oracle leaves
        # out is therefore met by construction and says nothing; it is informative for the harvested cases only.
        i64, i32 = _run_oracle(name, st, ja)[1], _run_oracle(name, st, ja, f32=True)[1]
        nc = np.where((i32['nc'] == i64['nc']) & (np.abs(i32['point_a'] - i64['point_a']).max((1, 2)) < 1e-4), i64['nc'], -1)
        pick = np.sort(np.concatenate([np.nonzero(nc == k)[0][:6] for k in range(26, 40)]).astype(int))   # up to six rows of every count
        S.append(st[pick]), J.append(ja[pick])
    st, ja = np.concatenate(S), np.concatenate(J)
    st = _stir(name, st, rs, share=0.7 if nb == 1 else 0.3)     # (one object alone on the table: at rest every solve agrees)
    return st, ja


# ----------------------------------------------------------------------------------------------------------------------
# the oracle's side: reference, spread, what a case reaches
MAX_DEPTH = 0.005


def _run_oracle(name, st, ja, f32=False, priors=None):
    out, info = np.zeros_like(st), []
    for lo in range(0, len(st), BATCH):
        m = min(BATCH, len(st) - lo)
        ora = _oracle(name, m, cls=O.SubstepOracle, joint=True, substeps=1, f32=f32, priors=priors)
        ora.set_state(st[lo:lo + m])
        ora.step(ja[lo:lo + m])
        out[lo:lo + m] = ora.get_state()
        info.append(ora.last_substep())
        ora.close()
    return out, {k: np.concatenate([d[k] for d in info]) for k in info[0]}


def _deepest(name, st, ja):
    """-> (deepest penetration per case, `corner` per case), float64 oracle.  corner: a finger stands on the chest with ONE point
    (a corner on a wall's or the lid's rim, well above the table).  Five iterations do not settle that single stiff row (its
    residual oscillates), so rounding is amplified tenfold against every other case and one such case would set its whole
    set's spread: it is no measure of a kernel, and is not taken"""
    info = _run_oracle(name, st, ja)[1]
    live = np.arange(info['distance'].shape[1])[None, :] < info['nc'][:, None]
    corner = np.zeros(len(st), bool)
    if _task(name)[0].startswith('chest'):
        for f in FINGERS:
            on_chest = live & (info['a'] == f) & (info['b'] == STATIC) & (info['point_a'][:, :, 2] > 0.2)
            corner |= on_chest.sum(1) == 1
    return np.where(live, -info['distance'], 0.0).max(1), corner


def run_oracle(name, f32=False, priors=None):
    """one substep of every case on the oracle -> (states after, last_substep() read-out)"""
    return _run_oracle(name, *cases(name), f32=f32, priors=priors)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict(s64, s32: states after one substep on the float64 / float32 oracle; info: the float64 read-out; near_exit [M]:
    a residual before the last iteration within a factor 4 of the early-exit threshold; bars: name of group -> bar)"""
    s64, info = run_oracle(name)
    s32, info32 = run_oracle(name, f32=True)
    res = info['residual'][:, :4]
    ran = np.arange(4)[None, :] < info['iterations'][:, None]
    near_exit = (ran & (res >= RESIDUAL_THRESHOLD / 4) & (res <= RESIDUAL_THRESHOLD * 4)).any(1)
    left32 = near_exit | (info32['nc'] != info['nc'])
    # away sets: cases in which a row joins the robot and a free body (the mispredicted envs) take no part in the bars
    live = np.arange(info['a'].shape[1])[None, :] < info['nc'][:, None]
    coupled = (live & (info['a'] >= 100) & (((info['b'] >= 0) & (info['b'] < 10)) | (info['b'] == DOOR))).any(1) & (not _joint(name))
    bars = {}
    for g, cols in groups(name).items():
        use = ~left32 & ~coupled
        d = np.abs(s32[use][:, cols].astype(np.float64) - s64[use][:, cols]).max() if use.any() else 0.0
        bars[g] = max(FLOOR, FACTOR * float(d))
    for a in (s64, s32, near_exit, left32, coupled):
        a.setflags(write=False)
    return dict(s64=s64, s32=s32, info=info, nc32=info32['nc'], near_exit=near_exit, left32=left32, coupled=coupled, bars=bars)


def tags(name):
    """what each case reaches, from its state and the float64 oracle's contact list: dict(tag -> bool [M])"""
    st, _ = cases(name)
    info = reference(name)['info']
    a, b, nc = info['a'], info['b'], info['nc']
    live = np.arange(a.shape[1])[None, :] < nc[:, None]
    pair = lambda pa, pb: (live & pa(a) & pb(b))
    is_blk = lambda x: (x >= 0) & (x < 10)
    is_fng = lambda x: (x == FINGERS[0]) | (x == FINGERS[1])
    t = {}
    t['no contact'] = nc == 0
    f_tab = pair(is_fng, lambda x: x == STATIC)
    t['both fingers on a static box'] = (pair(lambda x: x == FINGERS[0], lambda x: x == STATIC).any(1) &
                                         pair(lambda x: x == FINGERS[1], lambda x: x == STATIC).any(1))
    t['one finger only'] = f_tab.any(1) & ~t['both fingers on a static box']
    o_tab = pair(is_blk, lambda x: x == STATIC)
    t['object x static only'] = (nc > 0) & (o_tab.sum(1) == nc)
    t['finger x object'] = pair(is_fng, is_blk).any(1)
    t['gripper base x object'] = pair(lambda x: x == GBASE, is_blk).any(1)
    t['block x block'] = pair(is_blk, is_blk).any(1)
    t['finger x door'] = pair(is_fng, lambda x: x == DOOR).any(1)
    t['gripper base x chest'] = pair(lambda x: x == GBASE, lambda x: (x == DOOR) | (x == STATIC)).any(1)
    t['block x door'] = pair(is_blk, lambda x: x == DOOR).any(1)
    t['robot x free body'] = pair(lambda x: x >= 100, lambda x: is_blk(x) | (x == DOOR)).any(1)
    nbk = num_blocks(name)
    if nbk >= 2:                            # a block without a static contact while a lower- and a higher-numbered one have one
        has = np.stack([(o_tab & (a == k)).any(1) for k in range(nbk)], 1)
        t['a block without a table contact between two that have one'] = np.array(
            [any(not h[k] and h[:k].any() and h[k + 1:].any() for k in range(nbk)) for h in has])
        t['a block without a table contact'] = (~has).any(1)
        t['table runs only'] = (nc > 0) & (o_tab.sum(1) == nc) & has.all(1)
    q = st[:, :9].astype(np.float64)
    t['a joint at its limit'] = ((q <= JLO) | (q >= JHI)).any(1)
    t['a finger at its limit'] = ((q[:, 7:] <= JLO[7:]) | (q[:, 7:] >= JHI[7:])).any(1)
    t['an arm joint at its limit'] = ((q[:, :7] <= JLO[:7]) | (q[:, :7] >= JHI[:7])).any(1)
    dist = np.where(live, info['distance'] + 1e-5, np.nan)              # (+ LINEAR_SLOP, as the row's right-hand side has it)
    with np.errstate(invalid='ignore'):
        t['a contact inside the margin (dist > 0)'] = (dist > 0).any(1)
        t['a contact with penetration (ERP)'] = (dist <= 0).any(1)
    if _task(name)[0].startswith('chest'):
        upper = 0.12 if _task(name)[0] == 'chest_push' else 0.10
        t['door at its lower limit'] = st[:, 48] <= 0
        t['door at its upper limit'] = st[:, 48] >= upper
        t['door motor latched'] = st[:, 50] != 0
    for k in (8, 12, 13, 16, 30, 31):
        t['nc = %d' % k] = nc == k
    t['nc >= 17'] = nc >= 17
    t['nc >= 31'] = nc >= 31
    t['early exit of the solver'] = info['iterations'] < 5
    return t


# ----------------------------------------------------------------------------------------------------------------------
# the product's side
def run_product(pmg, library, name, packed, order=None):
    """one substep of every case on a one-substep build of the product (PMG_PACKED = packed, PMG_ENV_CYCLES=1), in batches
    of 64 -> (states after, contact count per case, list per case: 0 / 1, redone per case)"""
    st, ja = cases(name)
    task, kw = _task(name)
    order = np.arange(len(st)) if order is None else np.asarray(order)
    out = np.zeros((len(order), st.shape[1]), np.float32)
    nc, lst, redo = np.zeros(len(order), np.int64), np.zeros(len(order), np.int64), np.zeros(len(order), bool)
    saved = {k: os.environ.get(k) for k in ('PMG_PACKED', 'PMG_ENV_CYCLES')}
    os.environ['PMG_PACKED'], os.environ['PMG_ENV_CYCLES'] = str(int(packed)), '1'
    try:
        for lo in range(0, len(order), BATCH):
            sel = order[lo:lo + BATCH]
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                env = pmg.make_env(task=task, num_envs=len(sel), seed=11, seed_stride=1, joint_control=_joint(name), max_episode_steps=1000,
                                   _library=library, **kw)
            try:
                env.reset()
                env.set_state(st[sel])
                env.handle.step(np.ascontiguousarray(ja[sel]))
                out[lo:lo + len(sel)] = env.get_state()
                sch = env.handle.schedule()
                cyc = env.handle.env_cycles()[:, 1]
                on1 = np.zeros(len(sel), bool)
                on1[sch['free']] = True
                rd = np.zeros(len(sel), bool)
                rd[sch['redo']] = True
                assert len(sch['free']) + len(sch['prone']) == len(sel)
                # (the four-per-wavefront reach kernel has no contacts and counts none: its envs either finish there or are redone)
                counted = ~on1 | rd | (num_blocks(name) > 0)
                nc[lo:lo + len(sel)] = np.where(counted, cyc, 0)
                lst[lo:lo + len(sel)], redo[lo:lo + len(sel)] = on1, rd
            finally:
                env.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out, nc, lst, redo


def judge(name, got, got_nc, label, out=print):
    """Hold one run of the product (or a mutant of the oracle) to the float64 oracle.  -> dict(left_out [M], worst: group ->
    largest distance over the kept cases, failing [M]: kept cases beyond a VELOCITY bar, beyond: group -> kept cases beyond its bar)"""
    ref = reference(name)
    left = (ref['near_exit'] | (got_nc != ref['info']['nc'])) & ~ref['coupled']
    keep = ~left & ~ref['coupled']
    worst, beyond = {}, {}
    failing = np.zeros(len(got), bool)
    for g, cols in groups(name).items():
        d = np.abs(got[:, cols].astype(np.float64) - ref['s64'][:, cols]).max(1)
        d32 = np.abs(ref['s32'][:, cols].astype(np.float64) - ref['s64'][:, cols]).max(1)
        worst[g] = float(d[keep].max()) if keep.any() else 0.0
        beyond[g] = np.nonzero(keep & (d > ref['bars'][g]))[0]
        if g in VELOCITY_GROUPS:
            failing |= keep & (d > ref['bars'][g])
        out('%-22s %-28s %-8s worst %.3g  bar %.3g  (float32 oracle: %.3g)  ratio to the oracle spread %.2f  beyond: %s' % (
            name, label, g, worst[g], ref['bars'][g], float(d32[~ref['left32'] & ~ref['coupled']].max()) if (~ref['left32'] & ~ref['coupled']).any() else 0.0,
            worst[g] / max(ref['bars'][g] / FACTOR, 1e-30), list(beyond[g][:8])))
    for i in np.nonzero(left)[0]:
        out('%-22s %-28s left out: case %d, contacts %d (oracle %d), oracle residuals %s' % (
            name, label, i, got_nc[i], ref['info']['nc'][i], ref['info']['residual'][i, :5]))
    return dict(left_out=left, worst=worst, failing=failing, beyond=beyond)


# ----------------------------------------------------------------------------------------------------------------------
# what the case set must reach (asserted, CPU tier and device tier alike).  Tags come from the float64 oracle's contact list
# and the case's state; `lists` from the product's schedule().  Under joint control the launch plan (contact_prone,
# csrc/pmg_kernels.h) keeps EVERY env with several blocks on list 0 and sends a one-object env to list 1 only while its
# fingers are 4.7 cm above the table and its tip 11 cm from the object -- so a list-1 env has object x table contacts only.
# What the plan cannot produce under joint control is reached by the `<task>/away` sets under tip control instead
# (check_reach_away): 12 contacts kept and 13+ redone on the packed one-object list, 30 kept and 31+ redone on the multi-block
# and chest list 1, several blocks on list 1.
# Not reached, with the reason:
#  - slide, 17 and more contacts: a finger against the puck's SIDE gives two points (a line), so closed or open fingers at the
#    table give at most 4 + 8 + 2 + 2 = 16; four points per finger need a finger ON the puck's flat face, which lifts the
#    fingers off the table (4 + 4 + 4 = 12) -- or a penetration of centimetres, which MAX_DEPTH drops.
#  - the chest's stage-slot overflow on list 1 (ContactLds<6, 30>: more than NSTAGE = 32 pairs survive the culls,
#    csrc/pmg_contact_body.inc) with 30 contacts or fewer: gripper away, the survivors are the block x table pairs (5), block x
#    block pairs inside the 6 cm cull (five blocks that do not touch: at most 6 of the 10, a pentagon's diagonals are 1.6 sides)
#    and block x chest-box pairs inside 2.8 cm of a box; a pair that touches brings 2 ... 4 contacts and passes the 30 of the
#    store first.  Rings and grids of five blocks at the door under hovering fingers (a mispredicted env) reached 32 survivors
#    at most; check_reach_away therefore asserts the opposite, exactly: on list 1 an env is redone if and only if it has more
#    contacts than the store holds.
REQUIRED = {
    'reach': ['no contact', 'both fingers on a static box', 'one finger only', 'nc = 8', 'a finger at its limit', 'an arm joint at its limit',
              'a contact inside the margin (dist > 0)', 'a contact with penetration (ERP)'],
    'push': ['object x static only', 'finger x object', 'both fingers on a static box', 'nc = 12', 'nc = 13', 'nc = 16', 'nc >= 17',
             'a contact inside the margin (dist > 0)', 'a contact with penetration (ERP)', 'a joint at its limit'],
    'slide': ['object x static only', 'finger x object', 'both fingers on a static box', 'nc = 12', 'nc = 16'],
    'pick_and_place': ['object x static only', 'finger x object', 'gripper base x object', 'both fingers on a static box', 'nc = 12', 'nc = 16',
                       'nc >= 17'],
    'block_stack2': ['table runs only', 'block x block', 'a block without a table contact', 'finger x object', 'nc >= 17'],
    'block_stack3': ['table runs only', 'block x block', 'a block without a table contact between two that have one', 'finger x object', 'nc >= 17'],
    'block_stack4': ['table runs only', 'block x block', 'a block without a table contact between two that have one', 'finger x object', 'nc >= 31'],
    'block_rearrange5': ['table runs only', 'block x block', 'finger x object', 'both fingers on a static box', 'nc >= 31'],
    'chest_push2': ['door at its lower limit', 'door at its upper limit', 'door motor latched', 'finger x door', 'gripper base x chest',
                    'block x door', 'finger x object', 'table runs only'],
    'chest_pick_and_place1': ['door at its lower limit', 'door at its upper limit', 'door motor latched', 'finger x door', 'finger x object',
                              'object x static only'],
}
BOTH_LISTS = ('reach', 'push', 'slide', 'pick_and_place', 'chest_pick_and_place1')


SMALL_STORE = 30        # MULTI_SMALL_MAXC: contacts the multi-block / chest list 1 holds; beyond it the env is redone on the full store


PACKED_STORE = 12       # PACKED_MAXC: contacts a row of the packed one-object list holds; beyond it: pmg_k_redo_env<1, 24, CYL>


def check_reach_away(name, lst, nc, redo, packed):
    """... of a tip-control set: both lists, block x block rows on list 1, and a full store kept on list 1 (12 contacts for one
    object, 30 for several blocks and the chest), one contact more given up and redone -- exactly those"""
    t = tags(name)
    ref = reference(name)
    coupled, store = ref['coupled'], PACKED_STORE if num_blocks(name) == 1 else SMALL_STORE
    assert np.array_equal(t['robot x free body'], coupled)
    assert np.array_equal(nc[coupled], ref['info']['nc'][coupled]), (name, 'contact count of a mispredicted env', nc[coupled], ref['info']['nc'][coupled])
    assert (lst == 0).sum() >= 4 and (lst == 1).sum() >= 4, (name, (lst == 0).sum(), (lst == 1).sum())
    if num_blocks(name) == 1:
        want = (lst == 1) & (nc > store) & bool(packed)
        assert np.array_equal(redo, want), (name, np.nonzero(redo != want)[0])
        on1 = lst == 1
        assert coupled.sum() >= 8 and (on1 & coupled & (nc == store + 1)).any() and (on1 & coupled & (nc > store + 1)).any(), nc[coupled]
        assert (on1 & ~coupled & (nc == store) & t['both fingers on a static box']).sum() >= 8       # the full store: 4 + 8, fingers down
        assert (on1 & ~coupled & (nc == 4)).any() and ((lst == 0) & ~coupled & (nc == store)).any()
        return
    assert not coupled.any()
    if name == 'chest_push2/away':            # (its two blocks are pushed into the chest one after the other: they never meet)
        assert t['block x door'].any() and (t['door motor latched'] & (lst == 0)).any()
    else:
        assert (t['block x block'] & (lst == 1)).any() and (t['block x block'] & (lst == 0)).any()
    want = (lst == 1) & (nc > SMALL_STORE) & bool(packed)       # (PMG_PACKED=0: list 1 runs on the full store, nothing to redo)
    assert np.array_equal(redo, want), (name, np.nonzero(redo != want)[0])
    if num_blocks(name) == 5:
        on1 = lst == 1
        assert (on1 & (nc == SMALL_STORE)).any() and (on1 & (nc == SMALL_STORE + 1)).any() and (on1 & (nc > SMALL_STORE + 1)).any(), np.bincount(nc[on1])
    if num_blocks(name) == 3 or _base(name) == 'block_stack4':
        assert t['a block without a table contact between two that have one'].any()
    if _task(name)[0].startswith('chest'):
        assert (t['door at its lower limit'] & (lst == 1)).any() and (name != 'chest_push2/away' or (t['door motor latched'] & (lst == 1)).any())


def check_reach(name, lst, nc, redo=None, packed=1):
    """the paths the case set must reach: tags of the oracle, lists of the product's schedule"""
    if not _joint(name):
        return check_reach_away(name, lst, nc, redo, packed)
    t = tags(name)
    missing = [k for k in REQUIRED[name] if not t[k].any()]
    assert not missing, (name, 'no case reaches', missing)
    if name in BOTH_LISTS:
        assert (lst == 0).sum() >= 4 and (lst == 1).sum() >= 4, (name, 'cases on list 0 / list 1', (lst == 0).sum(), (lst == 1).sum())
    else:
        assert (lst == 0).all(), (name, 'several blocks under joint control: list 0')
    if name in ('push', 'slide', 'pick_and_place'):
        assert (t['both fingers on a static box'] & (lst == 0)).any(), 'fingers down at the table, on list 0'
        assert (t['object x static only'] & (lst == 1)).any(), 'object x table only, on list 1'
    if name == 'chest_pick_and_place1':       # list 1 of the chest: stage slots by rank among the surviving pairs, none given up
        assert ((lst == 1) & (nc > 4)).any() and ((lst == 1) & (nc == 4)).any()
    assert redo is None or not redo.any(), (name, 'redone under joint control', np.nonzero(redo)[0])


def check_task(pmg, library, name, packed, out=print):
    """every case of `name` on the one-substep build `library` with PMG_PACKED=packed, against the float64 oracle"""
    got, nc, lst, redo = run_product(pmg, library, name, packed)
    check_reach(name, lst, nc, redo, packed)
    j = judge(name, got, nc, 'PMG_PACKED=%d' % packed, out)
    share = j['left_out'].mean()
    out('%-22s PMG_PACKED=%d: %d cases, %d on list 1, %d redone, %d left out' % (name, packed, len(got), lst.sum(), redo.sum(), j['left_out'].sum()))
    assert share <= LEFT_OUT_CAP, (name, 'left out', np.nonzero(j['left_out'])[0])
    bad = {g: list(v) for g, v in j['beyond'].items() if len(v)}
    assert not bad, (name, 'PMG_PACKED=%d' % packed, 'cases beyond the bar, per group', bad, j['worst'], reference(name)['bars'])
    return got, nc, lst


def check_case_set(name, out=print):
    """the case set by itself: what the float32 oracle leaves out"""
    ref = reference(name)
    for i in np.nonzero(ref['left32'])[0]:
        out('%-22s float32 oracle leaves out case %d: contacts %d (float64 %d), residuals %s' % (
            name, i, ref['nc32'][i], ref['info']['nc'][i], ref['info']['residual'][i, :5]))
    assert ref['left32'].mean() <= LEFT_OUT_CAP_F32, (name, np.nonzero(ref['left32'])[0])
    assert len(ref['s64']) >= (48 if _joint(name) else 24) and len(ref['s64']) <= 4 * BATCH


MUTANTS = {'one friction direction': {'friction_dirs': 1.0}, 'four solver iterations': {'solver_iterations': 4.0}}


def check_mutant(name, mutant, out=print):
    """the float64 oracle with one switch changed, in place of the kernel: at least half of the cases with a contact must fail"""
    got, info = run_oracle(name, priors=MUTANTS[mutant])
    j = judge(name, got, info['nc'], mutant, out=lambda *a: None)
    touched = (reference(name)['info']['nc'] > 0) & ~j['left_out'] & ~reference(name)['coupled']     # (coupled cases are not held to the bars)
    share = j['failing'][touched].mean()
    out('%-22s %-24s fails the velocity check on %d of %d cases with a contact (%.0f %%)' % (name, mutant, j['failing'][touched].sum(), touched.sum(), 100 * share))
    assert touched.sum() >= 8 and share >= 0.5, (name, mutant, share)


def check_row_independence(pmg, library, name, out=print):
    """a case gives the same bits wherever it stands in its batch: the list-1 cases of `name` (four rows per packed wavefront)
    and as many list-0 cases, rotated through the four rows and with other neighbours"""
    got, nc, lst, _ = run_product(pmg, library, name, 1)
    pick = np.concatenate([np.nonzero(lst == 1)[0][:10], np.nonzero(lst == 0)[0][:6]])
    assert (lst[pick] == 1).sum() >= 4
    for turn, order in enumerate([pick, np.roll(pick, 1), np.roll(pick, 2), np.roll(pick, 3), pick[::-1]]):
        g2, n2, l2, _ = run_product(pmg, library, name, 1, order=order)
        assert np.array_equal(l2, lst[order]), (name, turn)
        same = (g2.view(np.uint32) == got[order].view(np.uint32)).all(1)
        assert same.all(), (name, 'order %d: cases %s differ from their run in the full batch' % (turn, list(order[~same])))
    out('%-22s %d cases bit-equal in five batch orders' % (name, len(pick)))



def check_redo_equals_full_store(pmg, library, name, out=print):
    """an env the small store of list 1 gives up is recomputed by pmg_k_redo_env on the full store: the same bits as under
    PMG_PACKED=0, where list 1 runs on the full store from the start"""
    g1, n1, l1, r1 = run_product(pmg, library, name, 1)
    g0, n0, l0, r0 = run_product(pmg, library, name, 0)
    assert r1.sum() >= 8 and not r0.any() and np.array_equal(l1, l0) and np.array_equal(n1, n0)
    same = (g1.view(np.uint32) == g0.view(np.uint32)).all(1)
    assert same[r1].all(), (name, 'redone cases that differ from the full-store kernel', np.nonzero(r1 & ~same)[0])
    out('%-22s %d redone cases bit-equal to the full-store kernel' % (name, r1.sum()))


def _handle_banner(make):
    """make() with the process's stderr captured -> (what make() returned, the text): the library names the switches a handle
    was created under on stderr"""
    import tempfile
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            got = make()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return got, f.read().decode(errors='replace')


def check_two_wavefront_reach(pmg, library, out=print):
    """pmg_k_step_reach2 (tip control only) against pmg_k_step_reach (PMG_REACH_TWO_WAVES=0) on the one-substep build: bit for
    bit, on the reach cases whose fingers are at the table, under tip control with a downward action"""
    st, _ = cases('reach')
    t = tags('reach')
    pick = np.nonzero(t['both fingers on a static box'] | t['one finger only'])[0]
    pick = np.concatenate([pick, np.nonzero(t['no contact'])[0][:len(pick)]])
    rs = np.random.RandomState(4)
    act = rs.uniform(-1, 1, (len(pick), 3)).astype(np.float32)
    act[:, 2] = -np.abs(act[:, 2])
    res = []
    for two in ('1', '0'):
        # the two-wavefront kernel runs only with the packed lists on (pmg_step_device: mode 2): pinned, whatever the caller's
        # environment says -- and the handle's own banner must name both switches with these values
        saved = {k: os.environ.get(k) for k in ('PMG_REACH_TWO_WAVES', 'PMG_ENV_CYCLES', 'PMG_PACKED')}
        os.environ['PMG_REACH_TWO_WAVES'], os.environ['PMG_ENV_CYCLES'], os.environ['PMG_PACKED'] = two, '1', '1'
        try:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                env, banner = _handle_banner(lambda: pmg.make_env(task='reach', num_envs=len(pick), seed=11, seed_stride=1, max_episode_steps=1000,
                                                                  _library=library))
            assert 'PMG_REACH_TWO_WAVES=%s' % two in banner and 'PMG_PACKED=1' in banner, banner
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        env.reset()
        s0 = st[pick].copy()
        s0[:, 18:21] = [O.fk_tip(q.astype(float))[0] for q in s0[:, :9]]          # the tip target where the tip is
        env.set_state(s0)
        o = env.handle.step(act)
        sch = env.handle.schedule()
        res.append((env.get_state(), o, env.handle.env_cycles()[:, 1].copy(), sch))
        env.close()
    (s2, o2, n2, sch2), (s1, o1, n1, sch1) = res
    assert len(sch2['prone']) >= 8 and (n2[sch2['prone']] > 0).sum() >= 4, (sch2, n2)       # contact-prone, and in contact
    assert np.array_equal(np.sort(sch2['prone']), np.sort(sch1['prone']))
    assert np.array_equal(s2.view(np.uint32), s1.view(np.uint32))
    for a, b in zip(o2, o1):
        assert np.array_equal(a, b)
    assert np.array_equal(n2[sch2['prone']], n1[sch1['prone']])
    out('two-wavefront reach kernel: %d envs on list 0, %d of them in contact, bit-equal to the one-wavefront kernel' % (
        len(sch2['prone']), (n2[sch2['prone']] > 0).sum()))
