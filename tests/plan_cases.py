"""The launch plan of a batched step held to a model: what pmg_k_plan / pmg_k_plan_reach / pmg_k_plan_count + pmg_k_plan_scatter
(plan_class, plan_promote, plan_place, plan_commit of csrc/pmg_kernels.h) must leave in the schedule buffer (csrc/pmg_sched.h), stated
once more in numpy float64 from the rule as DESIGN.md section 3.2 and the header's comments give it, the cases it is asked on, and the
check that both tiers run: tests/test_plan_emulated.py (pmge_plan, the CPU emulator) and tests/test_gpu_plan.py (pmgd_plan, gfx950).

THE RULE.  An env is *contact-prone* (class 0, list 0: one env per wavefront, full contact store) when
  * reach, tip control: the tip target's height now, or after this action (target + 0.01 * action, clipped to the tip box), is
    under the lower clip plane + 12 mm;
  * free objects, tip control: the clipped next tip target lies within `near_r` of a block centre, or -- chest tasks -- inside the
    box around the chest that the finger boxes can touch (five faces: the back at x0 - 0.064, the front at x1 + chest_reach, the
    sides at -0.134 and y1 + 0.064, the top at 0.287; all strict);
  * joint control: the lowest point of either finger box is under table top + 4.5 cm + the contact margin, or several blocks are
    in the scene, or the tip is within 11 cm of the one block.
Every other env is on the fast path: class 1 for reach; with free objects class 1 when the fingers are down at the table (the
height test above) and class 2 when they are up -- or, several blocks and longest-first on, class 1 when the env's wavefront took
more than the threshold in the previous step (strict).  List 0 = class 0 in env order, then class 1 if it is promoted; list 1 = an
unpromoted class 1, then class 2.  Promotion is one decision per batch from the grand totals: one block, tip control, and fd_div < 0,
or fd_div > 0 with n1 * fd_div <= N and n0 + n1 + ceil(n2 / 4) <= wave_budget.

WHY THE CASES KEEP CLEAR OF THE THRESHOLDS.  The kernels compute in float32 and the compiler may contract `ee + a * 0.01f` into one
fused operation, so no float32 restatement is bit-true AT a threshold and a float64 one is not either.  Every generator therefore
draws again any env whose deciding quantity is closer to its threshold than a margin: 1e-5 m under tip control (about 40 times the
few float32 roundings of O(1) m values: 3 x 6e-8 x 1.4), 1e-4 m under joint control (the float32 chain of nine joints of plan_fk:
nine rotations and translations of O(1) m at 6e-8 each, times the same factor).  `band_share` is the share of envs left inside a band
and must be zero.  The band is dropped only where float32 arithmetic is exact whatever the contraction (`exact` envs: a zero action,
so target + 0 * 0.01 is the target itself, compared with the float32 sum 0.175f + 0.012f that the device forms too).
"""
import ast
import ctypes as C
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODEL = open(os.path.join(ROOT, 'include', 'pmg_model.h')).read()


def _model_value(name):
    text = re.search(r'^#define %s (.*)$' % name, _MODEL, re.M).group(1).split('/*')[0]
    return np.array(ast.literal_eval(text.strip().replace('{', '[').replace('}', ']')), np.float64)


JPARENT, JTYPE = _model_value('PMG_JPARENT').astype(int), _model_value('PMG_JTYPE').astype(int)
JXYZ, JROT, JAXIS = _model_value('PMG_JXYZ'), _model_value('PMG_JROT'), _model_value('PMG_JAXIS')
FINGER_HALF, TIP_OFF, TABLE_HALF = _model_value('PMG_FINGER_HALF'), _model_value('PMG_TIP_OFF'), _model_value('PMG_TABLE_HALF')
NJ = 9
HOT_DIM, BLOCK_DIM = 32, 13
# the tip box and the table of every task but slide, as the probes set them (float32 values, held in float64)
EE_LO, EE_HI = np.float32([-0.67, -0.2, 0.175]).astype(np.float64), np.float32([-0.37, 0.2, 0.55]).astype(np.float64)
Z_DOWN32 = np.float32(0.175) + np.float32(0.012)          # the float32 sum the device compares with
Z_DOWN = float(Z_DOWN32)
TABLE_TOP = 0.08 + float(TABLE_HALF[2])
FINGER_CLEAR = TABLE_TOP + 0.045 + 0.002                   # + CONTACT_MARGIN (pmg_contact_body.inc)
JOINT_NEAR = 0.11
TIP_MARGIN, JOINT_MARGIN = 1e-5, 1e-4
PLAN_WG, PLAN_SINGLE_MAX = 1024, 16384
LPT_BINS, LPT_BIN_SHIFT = 128, 11
SENTINEL, GUARD = -7, 64
BIG_BUDGET = 1 << 30


def sched_words(n):
    return 4 + 3 * n + 3 * ((n + PLAN_WG - 1) // PLAN_WG)


# ---- float64 forward kinematics of the model constants: lowest point of the finger boxes, tip -------------------------------------
def fk(q):
    """q [n, 9] -> (lowest z of either finger box [n], tip [n, 3]): every joint's frame from its parent's, finger 2 off link 7 too."""
    q = np.asarray(q, np.float64)
    n = len(q)
    R, p = [None] * NJ, [None] * NJ
    for j in range(NJ):
        Rp = np.broadcast_to(np.eye(3), (n, 3, 3)) if JPARENT[j] < 0 else R[JPARENT[j]]
        pp = np.zeros((n, 3)) if JPARENT[j] < 0 else p[JPARENT[j]]
        if JTYPE[j]:                                       # prismatic along the joint axis
            L = np.broadcast_to(JROT[j], (n, 3, 3))
            o = JXYZ[j] + (JROT[j] @ JAXIS[j]) * q[:, j, None]
        else:                                              # revolute about the joint frame's z
            c, s = np.cos(q[:, j]), np.sin(q[:, j])
            Rz = np.zeros((n, 3, 3))
            Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
            L = JROT[j] @ Rz
            o = np.broadcast_to(JXYZ[j], (n, 3))
        p[j] = pp + np.einsum('nab,nb->na', Rp, o)
        R[j] = Rp @ L
    fz = np.minimum(*[p[j][:, 2] - np.abs(R[j][:, 2, :]) @ FINGER_HALF for j in (7, 8)])
    return fz, p[6] + R[6] @ TIP_OFF


# ---- the model -------------------------------------------------------------------------------------------------------------------
def lpt_on(case):
    return case['nb'] > 1 and case['env_cycles'] is not None and (case['lpt_thresh'] > 0 or case['lpt_permille'] > 0)


def lpt_threshold(case):
    if case['lpt_thresh'] > 0:
        return int(case['lpt_thresh'])
    return int(case['lpt_state'][case['lpt_parity']]) if case['lpt_permille'] > 0 else 0


def decide(case, mutant=None):
    """-> (class of every env, gap of the height test, smallest gap of every other deciding quantity), gaps in units of the margin."""
    hot, act = case['hot'].astype(np.float64), case['actions'].astype(np.float64)
    blocks = case['blocks'].astype(np.float64)
    N, nb = len(hot), case['nb']
    target = hot[:, 18:21]
    nxt = np.clip(target + 0.01 * act[:, :3], EE_LO, EE_HI)
    height = np.minimum(target[:, 2], nxt[:, 2])
    down = height <= Z_DOWN if mutant == 'le_height' else height < Z_DOWN
    gap_h = np.abs(height - Z_DOWN) / TIP_MARGIN
    gap = np.full(N, np.inf)
    if case['joint_control']:
        fz, tip = fk(hot[:, :NJ])
        prone = fz < FINGER_CLEAR
        gap = np.abs(fz - FINGER_CLEAR) / JOINT_MARGIN
        if nb > 1:
            prone, gap = np.ones(N, bool), np.full(N, np.inf)
        elif nb == 1:
            d = np.linalg.norm(tip - blocks[:, :3], axis=1)
            prone = prone | (d < JOINT_NEAR)
            gap = np.minimum(gap, np.abs(d - JOINT_NEAR) / JOINT_MARGIN)
        if nb != 1:
            gap_h = np.full(N, np.inf)                     # the height decides nothing here
    elif nb == 0:
        prone = down
    else:
        near_r = float(np.float32(case['near_r']))
        prone = np.zeros(N, bool)
        for b in range(nb):
            d = np.linalg.norm(nxt - blocks[:, BLOCK_DIM * b:BLOCK_DIM * b + 3], axis=1)
            prone |= d < near_r
            gap = np.minimum(gap, np.abs(d - near_r) / TIP_MARGIN)
        if case['chest'] >= 0:
            door = case['chest'] == 0
            x0, x1, y1 = (-0.705, -0.592, 0.19) if door else (-0.805, -0.555, 0.07)
            faces = [(nxt[:, 0], x0 - 0.064, 1), (nxt[:, 0], x1 + float(np.float32(case['chest_reach'])), -1), (nxt[:, 1], -0.07 - 0.064, 1),
                     (nxt[:, 1], y1 + 0.064, -1), (nxt[:, 2], 0.272 + 0.015, -1)]
            inside = np.ones(N, bool)
            for v, f, sign in faces:
                inside &= sign * (v - f) > 0
                gap = np.minimum(gap, np.abs(v - f) / TIP_MARGIN)
            prone |= inside
    cls = np.where(prone, 0, 1)
    if nb >= 1:
        thr = lpt_threshold(case) if lpt_on(case) else 0
        if thr > 0:
            fast = np.where(case['env_cycles'][:, 0].astype(np.int64) > thr, 1, 2)
            gap_h = np.full(N, np.inf)
        else:
            fast = np.where(down, 1, 2)
        cls = np.where(prone, 0, fast)
    return cls, gap_h, gap


def _promote(case, n_envs, n0, n1, n2):
    fd = case['fd_div']
    return bool(case['nb'] == 1 and not case['joint_control'] and
                (fd < 0 or (fd > 0 and n1 * fd <= n_envs and n0 + n1 + (n2 + 3) // 4 <= case['wave_budget'])))


def model(case, mutant=None):
    """What the plan must leave behind.  mutant (tests/test_plan_model.py: the case set must tell each from the rule): 'le_height' (<=
    for < at the height test), 'class2_first' (class 2 in front of an unpromoted class 1), 'per_workgroup' (promotion decided by
    every 1024-env workgroup from its own counts)."""
    cls = decide(case, mutant)[0]
    N = len(cls)
    idx = np.arange(N, dtype=np.int32)
    nwg = (N + PLAN_WG - 1) // PLAN_WG
    wg_counts = np.array([[np.count_nonzero(cls[w * PLAN_WG:(w + 1) * PLAN_WG] == c) for c in range(3)] for w in range(nwg)], np.int32)
    n0, n1, n2 = (int(x) for x in wg_counts.sum(0))
    if mutant == 'per_workgroup':
        moved = np.repeat([_promote(case, N, *(int(x) for x in wg_counts[w])) for w in range(nwg)], PLAN_WG)[:N]
        promote = bool(moved[0])
    else:
        promote = _promote(case, N, n0, n1, n2)
        moved = np.full(N, promote)
    e1_up, e1_stay = idx[(cls == 1) & moved], idx[(cls == 1) & ~moved]
    list0 = np.concatenate([idx[cls == 0], e1_up])
    list1 = np.concatenate([idx[cls == 2], e1_stay] if mutant == 'class2_first' else [e1_stay, idx[cls == 2]])
    out = {'cls': cls, 'list0': list0, 'list1': list1, 'promoted': int(promote), 'wg_counts': wg_counts, 'lpt_state': None}
    if case['lpt_state'] is not None:
        st = np.array(case['lpt_state'], np.int32)
        if case['nb'] > 1 and case['lpt_permille'] > 0 and case['env_cycles'] is not None and case['lpt_thresh'] <= 0:
            # two-pass plan only: this step's fast-path envs into the histogram, the share's bin into the OTHER parity's word, histogram emptied
            bins = np.minimum(case['env_cycles'][cls > 0, 0].astype(np.int64) >> LPT_BIN_SHIFT, LPT_BINS - 1)
            hist = st[2:].astype(np.int64) + np.bincount(bins, minlength=LPT_BINS)
            total = int(hist.sum())
            tail = np.cumsum(hist[::-1])[::-1]             # envs in bin b or above
            named = [b for b in range(1, LPT_BINS) if tail[b] * 1000 >= total * case['lpt_permille']]
            st[case['lpt_parity'] ^ 1] = 0 if hist[0] == total else (max(named) if named else 0) << LPT_BIN_SHIFT
            st[2:] = 0
        out['lpt_state'] = st
    return out


# ---- case generators ---------------------------------------------------------------------------------------------------------------
def _new_case(N, nb, adim=3, **kw):
    case = dict(N=N, nb=nb, adim=adim, chest=-1, joint_control=0, near_r=0.065 if nb <= 1 else 0.045, chest_reach=0.02, fd_div=0,
                wave_budget=BIG_BUDGET, lpt_thresh=0, lpt_permille=0, lpt_parity=0, env_cycles=None, lpt_state=None,
                hot=np.zeros((N, HOT_DIM), np.float32), blocks=np.zeros((N, BLOCK_DIM * max(nb, 1)), np.float32),
                actions=np.zeros((N, adim), np.float32), exact=np.zeros(N, bool))
    case.update(kw)
    return case


@functools.lru_cache(maxsize=None)
def _base_poses():
    """Arm poses with the gripper pointing down at a grid of tip positions, fingers low over the table to well clear of it."""
    import oracle_lib as O
    env = O.OracleEnv('reach', 1, seed_base=0, seed_stride=1)
    env.reset()
    q0 = env.get_state()[0, :NJ].astype(np.float64)
    env.close()
    out = []
    for z in (0.18, 0.20, 0.215, 0.23, 0.25, 0.30, 0.40):
        for x in (-0.62, -0.52, -0.42):
            for y in (-0.15, 0.0, 0.15):
                out.append(O.ik(q0, [x, y, z])[0])
    return np.array(out)


def _rows(rs, case, n, mix):
    """n fresh env rows of `case`'s family: (hot, blocks, actions).  mix = (share aimed at an object / the chest, share with the fingers down)."""
    nb, adim = case['nb'], case['adim']
    hot, blocks = np.zeros((n, HOT_DIM)), np.zeros((n, BLOCK_DIM * max(nb, 1)))
    act = rs.uniform(-1, 1, (n, adim))
    for b in range(nb):
        blocks[:, BLOCK_DIM * b] = rs.uniform(-0.64, -0.40, n)
        blocks[:, BLOCK_DIM * b + 1] = rs.uniform(-0.18, 0.18, n)
        blocks[:, BLOCK_DIM * b + 2] = 0.175 + 0.03 * (rs.uniform(0, 1, n) < 0.2) * (b > 0)      # some stacked a level up
        blocks[:, BLOCK_DIM * b + 6] = 1.0
    kind = rs.choice(3, n, p=[mix[0], mix[1], 1.0 - mix[0] - mix[1]])
    hot[:, 18], hot[:, 19] = rs.uniform(-0.67, -0.37, n), rs.uniform(-0.2, 0.2, n)
    hot[:, 20] = np.where(kind == 1, 0.175 + rs.uniform(0, 0.011, n), rs.uniform(0.2, 0.5, n))
    if case['joint_control']:
        base = _base_poses()
        q = base[rs.randint(len(base), size=n)].copy()
        q[:, :7] += rs.uniform(-0.03, 0.03, (n, 7))
        q[:, 7:] = rs.uniform(0, 0.035, (n, 2))
        hot[:, :NJ] = q
        if nb == 1:
            tip = fk(q.astype(np.float32))[1]
            d = rs.normal(size=(n, 3))
            d *= (rs.uniform(0.02, 0.10, n) / np.linalg.norm(d, axis=1))[:, None]
            at = kind == 0
            blocks[at, :3] = (tip + d)[at]
    elif nb >= 1:
        at = kind == 0                                      # aimed at one of the blocks
        which = rs.randint(nb, size=n)
        centre = np.stack([blocks[np.arange(n), BLOCK_DIM * which + a] for a in range(3)], 1)
        aim = centre + rs.uniform(-0.03, 0.03, (n, 3))
        aim[:, 2] = np.maximum(aim[:, 2], 0.175)
        hot[at, 18:21] = aim[at]
        if case['chest'] >= 0:
            # a third of those at the chest instead: inside the box, and just inside / outside one of its five faces (either side by
            # 1e-4 or 1e-3 m); the action is zero so that the target itself is what the faces see; the blocks are put out of reach
            door = case['chest'] == 0
            x0, x1, y1 = (-0.705, -0.592, 0.19) if door else (-0.805, -0.555, 0.07)
            lo = (np.array([x0 - 0.064, -0.134, 0.0]), np.array([x1 + case['chest_reach'], y1 + 0.064, 0.287]))      # the box: low and high corner
            ch = at & (rs.uniform(0, 1, n) < 0.5)
            m = int(ch.sum())
            p = np.stack([rs.uniform(max(lo[0][0], -0.67) + 0.005, lo[1][0] - 0.005, m), rs.uniform(-0.12, min(lo[1][1], 0.2) - 0.01, m),
                          np.where(rs.uniform(0, 1, m) < 0.5, rs.uniform(0.176, 0.186, m), rs.uniform(0.20, 0.28, m))], 1)
            face = rs.randint(6, size=m)                   # 5: none, well inside
            off = rs.choice([1e-4, 1e-3], m) * rs.choice([-1.0, 1.0], m)
            for f, (axis, value) in enumerate([(0, lo[0][0]), (0, lo[1][0]), (1, lo[0][1]), (1, lo[1][1]), (2, lo[1][2])]):
                p[face == f, axis] = value + off[face == f]
            hot[ch, 18:21] = p
            act[ch] = 0.0
            for b in range(nb):
                blocks[ch, BLOCK_DIM * b] = -0.40
                blocks[ch, BLOCK_DIM * b + 1] = 0.19 - 0.04 * b
                blocks[ch, BLOCK_DIM * b + 2] = 0.35
    return hot.astype(np.float32), blocks.astype(np.float32), act.astype(np.float32)


def in_band(case):
    _, gap_h, gap = decide(case)
    return (gap < 1.0) | (~case['exact'] & (gap_h < 1.0))


def band_share(case):
    return float(in_band(case).mean())


def _fill(rs, case, mix):
    N = case['N']
    case['hot'], case['blocks'], case['actions'] = _rows(rs, case, N, mix)
    if case['env_cycles'] is not None:
        case['env_cycles'] = np.stack([rs.randint(0, 12000, N), rs.randint(0, 30, N)], 1).astype(np.int32)
    for _ in range(100):
        bad = np.nonzero(in_band(case))[0]
        if len(bad) == 0:
            break
        case['hot'][bad], case['blocks'][bad], case['actions'][bad] = _rows(rs, case, len(bad), mix)
    return case


def _tiny(case, shift):
    """1 or 2 envs: the classes in turn (env i of variant `shift` is class (i + shift) % 3); a free block, tip control."""
    for i in range(case['N']):
        k = (i + shift) % 3
        for b in range(case['nb']):
            case['blocks'][i, BLOCK_DIM * b:BLOCK_DIM * b + 3] = [-0.45, 0.1 - 0.04 * b, 0.175]
            case['blocks'][i, BLOCK_DIM * b + 6] = 1
        case['hot'][i, 18:21] = [[-0.45, 0.1, 0.19], [-0.6, -0.1, 0.18], [-0.6, -0.1, 0.3]][k]
        case['actions'][i] = 0
    return case


def _edges(case):
    """The exact edges on the last envs of the batch (a zero action: no rounding whatever the contraction), and the two clip cases."""
    N, nb = case['N'], case['nb']
    rows = []
    # (target height, action z, block 0 height or None)
    rows.append((Z_DOWN32, 0.0, None))                                   # on the plane: strict <, fingers up
    rows.append((np.nextafter(Z_DOWN32, np.float32(0)), 0.0, None))      # one ulp under it: down
    rows.append((np.float32(0.18), 1.0, None))                           # low now, going up: still down (the lower of now and next)
    if nb >= 1:
        rows.append((np.float32(0.60), 1.0, np.float32(0.52)))           # above the box: clipped to 0.55, 3 cm over a block held at 0.52
    if N < 2 * len(rows):
        return case
    for k, (z, az, bz) in enumerate(rows):
        i = N - 1 - k
        case['hot'][i, 18:21] = [-0.65, -0.18, z]
        case['actions'][i] = 0
        case['actions'][i, 2] = az
        for b in range(nb):
            case['blocks'][i, BLOCK_DIM * b:BLOCK_DIM * b + 3] = [-0.40, 0.18 - 0.04 * b, 0.175]
        if bz is not None:
            case['blocks'][i, 0:3] = [-0.65, -0.18, bz]
        case['exact'][i] = az == 0.0
    return case


def _force_n1(case, want):
    """Move envs between the fingers-down and the fingers-up class until exactly `want` are down (one block, tip control)."""
    cls = decide(case)[0]
    free = ~case['exact'] & (np.linalg.norm(case['hot'][:, 18:20] - case['blocks'][:, 0:2], axis=1) > 0.09)
    free[-4:] = False                                      # (the edge rows stay as they are)
    for i in np.nonzero(free & (cls == 1))[0][:max(0, int((cls == 1).sum()) - want)]:
        case['hot'][i, 20], case['actions'][i, 2] = 0.3, 0.0
    for i in np.nonzero(free & (cls == 2))[0][:max(0, want - int((cls == 1).sum()))]:
        case['hot'][i, 20], case['actions'][i, 2] = 0.18, 0.0
    assert int((decide(case)[0] == 1).sum()) == want
    return case


FAMILIES = ('obj_pick', 'obj_push', 'obj_fd8_few', 'obj_fd8_many', 'obj_fd8_fits', 'obj_fd8_over', 'multi2', 'multi3', 'multi4', 'multi5',
            'chest_door', 'chest_lid', 'lpt_const', 'reach_joint', 'obj_joint', 'multi_joint', 'lpt_a', 'lpt_b', 'lpt_c', 'lpt_empty')
SIZES_SINGLE = (1, 2, 63, 64, 65, 1023, 1024, 1025, 3000, 4095, 4096, 4097, 16383, 16384)
SIZES = SIZES_SINGLE + (16385, 65536 + 256)
EMULATED_MAX = 4097


def _spread_cycles(rs, N):
    c = rs.randint(0, 200000, N)
    c[rs.uniform(0, 1, N) < 0.05] = LPT_BINS << LPT_BIN_SHIFT           # past the histogram: the last bin
    c[rs.uniform(0, 1, N) < 0.05] += 10 << 20
    return c


def build(family, N, seed=0):
    rs = np.random.RandomState((hash_name(family) + 7919 * N + seed) % (1 << 31))
    shift = FAMILIES.index(family) if family in FAMILIES else 0
    if family == 'reach':
        return _edges(_fill(rs, _new_case(N, 0), (0.0, 0.3)))
    if family == 'reach_joint':
        return _fill(rs, _new_case(N, 0, adim=7, joint_control=1), (0.0, 0.3))
    if family.startswith('obj_'):
        joint = family == 'obj_joint'
        fd = {'obj_pick': -1, 'obj_push': 0, 'obj_joint': 0}.get(family, 8)
        case = _new_case(N, 1, adim=7 if joint else 4, joint_control=int(joint), fd_div=fd)
        if N < 3 and not joint:
            case = _tiny(case, shift)
        else:
            case = _fill(rs, case, (0.3, 0.3) if joint else (0.15, 0.06 if family in ('obj_fd8_fits', 'obj_fd8_over') else 0.2))
            if not joint:
                case = _edges(case)
        if N >= 63 and family in ('obj_fd8_few', 'obj_fd8_many'):       # either side of n1 * fd_div <= N, to the env
            case = _force_n1(case, N // 8 + (family == 'obj_fd8_many'))
        if N >= 63 and family in ('obj_fd8_fits', 'obj_fd8_over'):      # (few enough down for the first condition to hold)
            case = _force_n1(case, N // 16)
        if family in ('obj_fd8_fits', 'obj_fd8_over'):                   # either side of the wavefront budget, to the wavefront
            n = np.bincount(decide(case)[0], minlength=3)
            case['wave_budget'] = int(n[0] + n[1] + (n[2] + 3) // 4) - (family == 'obj_fd8_over')
        return case
    if family.startswith('multi'):
        joint = family == 'multi_joint'
        nb = 3 if joint else int(family[5:])
        case = _new_case(N, nb, adim=7 if joint else 4, joint_control=int(joint))
        return _tiny(case, shift) if N < 3 and not joint else (_fill(rs, case, (0.2, 0.3)) if joint else _edges(_fill(rs, case, (0.2, 0.3))))
    if family.startswith('chest_'):
        case = _new_case(N, 2, adim=3 if family == 'chest_door' else 4, chest=0 if family == 'chest_door' else 1, near_r=0.05)
        return _tiny(case, shift) if N < 3 else _edges(_fill(rs, case, (0.35, 0.25)))
    if family == 'lpt_const':
        # class 1 iff the env's cycle count is ABOVE the constant: some envs on it, some one over it
        case = _fill(rs, _new_case(N, 3, adim=4, lpt_thresh=6000, env_cycles=True), (0.2, 0.3))
        case['env_cycles'][::5, 0] = 6000
        case['env_cycles'][1::5, 0] = 6001
        return _tiny(case, shift) if N < 3 else case
    if family in ('lpt_a', 'lpt_b', 'lpt_c', 'lpt_empty'):
        # the derived threshold over three consecutive plans, the parity flipping: (a) nothing measured -- every cycle count in bin 0,
        # or no fast-path env at all -- leaves 0; (b) a spread histogram leaves the bin the share names; (c) the next plan orders by it
        case = _new_case(N, 4, adim=4, lpt_permille=400, env_cycles=True, lpt_state=np.zeros(2 + LPT_BINS, np.int32))
        case = _tiny(case, shift) if N < 3 else _fill(rs, case, (0.2, 0.3))
        if family == 'lpt_empty':                          # every env aimed at its first block: no fast-path env, an empty histogram
            for _ in range(100):
                case['hot'][:, 18:21] = case['blocks'][:, 0:3]
                case['actions'][:] = 0
                bad = np.nonzero(in_band(case))[0]         # (another block's distance may have come to lie on the radius)
                if len(bad) == 0:
                    break
                case['hot'][bad], case['blocks'][bad], case['actions'][bad] = _rows(rs, case, len(bad), (0.2, 0.3))
        if family in ('lpt_a', 'lpt_empty'):
            case['env_cycles'] = np.stack([rs.randint(0, 1 << LPT_BIN_SHIFT, N), rs.randint(0, 30, N)], 1).astype(np.int32)
            case['lpt_state'] = np.zeros(2 + LPT_BINS, np.int32)
            return case
        case['env_cycles'] = np.stack([_spread_cycles(rs, N), rs.randint(0, 30, N)], 1).astype(np.int32)
        case['lpt_parity'] = 1 if family == 'lpt_b' else 0
        before = build('lpt_a' if family == 'lpt_b' else 'lpt_b', N, seed)
        case['lpt_state'] = model(before)['lpt_state']
        return case
    raise KeyError(family)


def hash_name(s):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(s))


def _case_table():
    """The families distributed over the sizes (not their product): reach at every size, three more per size in rotation, so that every
    family meets small, ragged and multi-workgroup batches."""
    out = []
    for i, N in enumerate(SIZES):
        out.append(('reach', N))
        for k in range(3):
            out.append((FAMILIES[(3 * i + k) % len(FAMILIES)], N))
    # what the rotation leaves out: the promotion boundaries at a ragged multi-workgroup size, each chest at
    # the single-workgroup limit, the derived threshold where several workgroups add to one histogram
    out += [('obj_fd8_few', 3000), ('obj_fd8_many', 3000), ('obj_fd8_fits', 1025), ('obj_fd8_over', 1025), ('chest_door', 16384), ('chest_lid', 1025),
            ('lpt_a', 65), ('lpt_b', 65), ('lpt_c', 65), ('lpt_a', 4097), ('lpt_b', 4097), ('lpt_c', 4097), ('lpt_a', 16385), ('lpt_b', 16385), ('lpt_c', 16385), ('multi5', 65), ('obj_joint', 1025),
            ('lpt_empty', 4097)]
    return list(dict.fromkeys(out))


CASES = _case_table()


def case_id(fn):
    return '%s-%d' % fn


@functools.lru_cache(maxsize=None)
def case(family, N):
    return build(family, N)


def modes(family, N):
    """The plans that serve the case: 0 the single-workgroup plan, 1 its reach instantiation, 2 the two-pass plan."""
    single = [] if N > PLAN_SINGLE_MAX else ([0, 1] if family == 'reach' else [0])
    return single + [2]


def has_free_objects(family):
    return family not in ('reach', 'reach_joint', 'multi_joint', 'lpt_empty')


def check_case_set(out=print):
    """On the CPU: no env of any case within a band, and all three classes present in every case with free objects (1 and 2 envs: in
    the cases of that size together; several blocks under joint control are class 0 by rule)."""
    tiny = {1: set(), 2: set()}
    for family, N in CASES:
        c = case(family, N)
        share = band_share(c)
        present = set(np.unique(decide(c)[0]).tolist())
        assert share == 0.0, (family, N, share)
        if has_free_objects(family):
            if N < 3:
                tiny[N] |= present
            else:
                assert present == {0, 1, 2}, (family, N, present)
        elif family not in ('multi_joint', 'lpt_empty'):
            assert present == ({0, 1} if N > 2 else present), (family, N, present)
    assert tiny[1] == {0, 1, 2} and tiny[2] == {0, 1, 2}, tiny
    out('%d plan cases, no env within a band, every class present' % len(CASES))


def check_fk_against_oracle(fk_tip, out=print):
    """The model's float64 kinematics against the oracle's on the poses the joint-control cases use (both float64 over nine joints of
    O(1) m: 1e-13 is a hundred times their rounding)."""
    worst = 0.0
    for family, N in CASES:
        c = case(family, N)
        if c['joint_control']:
            q = c['hot'][:256, :NJ].astype(np.float64)
            tip = fk(q)[1]
            worst = max(worst, max(float(np.abs(fk_tip(q[i])[0] - tip[i]).max()) for i in range(len(q))))
    out('model tip against the oracle: %.2e' % worst)
    assert worst < 1e-13, worst
    return worst


# ---- running a probe -----------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def run(fn, c, mode, lpt_state=None):
    """One call of pmge_plan / pmgd_plan -> (return code, the whole buffer with its guards, lpt_state after)."""
    N = c['N']
    buf = np.full(2 * GUARD + sched_words(N), SENTINEL, np.int32)
    st = None if c['lpt_state'] is None else np.array(c['lpt_state'] if lpt_state is None else lpt_state, np.int32)
    fn.restype = C.c_int
    rc = fn(C.c_int(mode), C.c_int(N), C.c_int(c['nb']), C.c_int(c['chest']), C.c_int(c['joint_control']), C.c_float(c['near_r']), C.c_float(c['chest_reach']),
            C.c_int(c['fd_div']), C.c_int(c['wave_budget']), C.c_int(c['lpt_thresh']), C.c_int(c['lpt_permille']), C.c_int(c['lpt_parity']), _ptr(c['env_cycles']),
            _ptr(st), _ptr(c['hot']), _ptr(c['blocks']), _ptr(c['actions']), C.c_int(c['adim']), C.c_int(GUARD), _ptr(buf))
    return rc, buf, st


def compare(c, mode, buf, st, want, label):
    """Every word of the buffer against the model: counts, lists, redo count, promoted word, per-workgroup counts (two-pass plan) -- and
    the sentinel wherever the plan has no business: behind either list's count, the whole redo list, the guards."""
    N = c['N']
    nwg = (N + PLAN_WG - 1) // PLAN_WG
    assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), '%s: guard words written' % label
    w = buf[GUARD:-GUARD]
    n0, n1 = len(want['list0']), len(want['list1'])
    assert (int(w[0]), int(w[1])) == (n0, n1), '%s: counts %s, model %s' % (label, (int(w[0]), int(w[1])), (n0, n1))
    assert np.array_equal(w[2:2 + n0], want['list0']), '%s: list 0' % label
    assert np.array_equal(w[2 + N:2 + N + n1], want['list1']), '%s: list 1' % label
    assert (w[2 + n0:2 + N] == SENTINEL).all() and (w[2 + N + n1:2 + 2 * N] == SENTINEL).all(), '%s: a list word behind its count written' % label
    assert w[2 + 2 * N] == 0, '%s: redo count' % label
    assert (w[3 + 2 * N:3 + 3 * N] == SENTINEL).all(), '%s: redo list written' % label
    wg = w[3 + 3 * N:3 + 3 * N + 3 * nwg]
    if mode == 2:
        assert np.array_equal(wg.reshape(nwg, 3), want['wg_counts']), '%s: per-workgroup class counts' % label
    else:
        assert (wg == SENTINEL).all(), '%s: the single-workgroup plan wrote per-workgroup counts' % label
    assert w[3 + 3 * N + 3 * nwg] == want['promoted'] and len(w) == 4 + 3 * N + 3 * nwg, '%s: promoted word' % label
    if st is not None:
        # the single-workgroup plan keeps no histogram and derives no threshold (a known gap, pmg_kernels.h: plan_commit's comment): it
        # leaves lpt_state as it found it.  Stated as it is
        assert np.array_equal(st, want['lpt_state'] if mode == 2 else c['lpt_state']), '%s: lpt_state' % label


def check(fn, family, N, tier):
    """The case through every plan that serves it; the plans agree word for word where both ran (but for the workgroup counts)."""
    c = case(family, N)
    want = model(c)
    got = {}
    for mode in modes(family, N):
        label = '%s %s-%d mode %d' % (tier, family, N, mode)
        rc, buf, st = run(fn, c, mode)
        assert rc == 0, '%s: return code %d' % (label, rc)
        compare(c, mode, buf, st, want, label)
        got[mode] = buf
    wgc = slice(GUARD + 3 + 3 * N, GUARD + 3 + 3 * N + 3 * ((N + PLAN_WG - 1) // PLAN_WG))
    for mode, buf in got.items():
        a, b = buf.copy(), got[2].copy()
        a[wgc] = b[wgc] = 0
        assert np.array_equal(a, b), '%s %s-%d: plans %d and 2 differ' % (tier, family, N, mode)
    return want


def check_lpt_sequence(fn, N, tier):
    """Three consecutive two-pass plans through the probe, each from the lpt_state the probe itself left: (a) every cycle count in
    bin 0 -> threshold 0, (b) spread, a twentieth beyond the 128 bins -> the bin the share names, (c) ordered by that threshold."""
    st = None
    for family in ('lpt_a', 'lpt_b', 'lpt_c'):
        c = case(family, N)
        want = model(c)
        rc, buf, st = run(fn, c, 2, lpt_state=st)
        assert rc == 0
        compare(c, 2, buf, st, want, '%s %s-%d from the probe\'s own state' % (tier, family, N))
    b, cc = model(case('lpt_b', N))['lpt_state'], case('lpt_c', N)
    assert b[0] > 0 and lpt_threshold(cc) == b[0] and (b[0] >> LPT_BIN_SHIFT) < LPT_BINS
    return st


def check_refusals(fn):
    """Arguments outside the probe's range return < 0 and leave the buffer alone (the arrays are those of 64 envs: a refusal comes
    before anything is read)."""
    c = case('reach', 64)
    for patch, mode in ((dict(N=0), 0), (dict(N=131073), 2), (dict(nb=6), 0), (dict(N=PLAN_SINGLE_MAX + 1), 0), (dict(nb=1), 1), (dict(lpt_parity=2), 0),
                        (dict(chest=2), 0), (dict(env_cycles=np.full((64, 2), -1, np.int32)), 0)):
        rc, buf, _ = run(fn, dict(c, **patch), mode)
        assert rc < 0 and (buf == SENTINEL).all(), patch
