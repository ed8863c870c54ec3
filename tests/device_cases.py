"""The cases -- and the checks against the float64 oracle -- of the device-function tests, shared by their two tiers:
tests/test_emulated_kernels.py runs the product's device functions as g++ code on the fiber emulator, one call per case;
tests/test_gpu_device_functions.py runs them as gfx950 code through the device probe library, one lane per pair and many
cases per launch.  Both hand a RUNNER to the same check, so both see the same inputs, the same oracle_lib probes and the
same bars.

Runners:
    dynamics(q, qd, tau [n][9])      -> qdd [n][9], minv [n][81], tip [n][12]
    ik(q [n][9], target [n][3])      -> q_out [n][9]
    narrowphase(kind, pairs [n][30]) -> n [n], out [n][40], amb [n]      (kind: NP_* below; a pair: ca3 Ra9 ha3 cb3 Rb9 hb3)
    fk64(q9 [n][9], body [n])        -> p [n][3], R [n][9]  (float64)
    cyl_redo64(blk [n][13], kc [24]) -> n [n], out [n][40]   (the puck, free body 0, against the table)
    redo_pairs(ck, ids [n][4], q9 [n][9], blk [n][2][13], doorq [n], kc [24], lanes=None) -> n [n], out [n][40]
        (cyl_redo64<ck> on any of its pairs; an id row: cyl_body, box_body, wall, handed -- REDO_* below)
    double_maths(op, x [n], y [n])   -> o0 [n], o1 [n]  (float64; op: DM_SQRT t_sqrt(x), DM_DIV t_div(x, y), DM_SINCOS sincos64(x))"""
import ctypes as C
import functools
import itertools
import json
import os

import numpy as np

import oracle_lib as O

NP_FAST, NP_CYL, NP_GENERAL, NP_FAST_ALIGNED = 0, 1, 2, 3
JLO = np.array([-2.96705972839, -2.09439510239, -2.96705972839, -2.09439510239, -2.96705972839, -2.09439510239, -3.05432619099, 0.0, 0.0])
JHI = -JLO + np.r_[np.zeros(7), 0.035, 0.035]
Q_START = np.float32([0, -0.5592432, 0, 1.733180, 0, -0.8501557, 0, 0.035, 0.035])
EE_LO, EE_HI = np.array([-0.67, -0.2, 0.175]), np.array([-0.37, 0.2, 0.55])       # the workspace box of the tip target


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_pair(ca, Ra, ha, cb, Rb, hb):
    return np.concatenate([np.float32(x).ravel() for x in (ca, Ra, ha, cb, Rb, hb)])


def unpack_pair(p):
    return [p[0:3], p[3:12], p[12:15], p[15:18], p[18:27], p[27:30]]


# ----------------------------------------------------------------------------------------------------------------------
# dynamics
def dynamics_cases_basic():
    """the three poses around the start pose of the emulated test"""
    rs = np.random.RandomState(0)
    out = []
    for _ in range(3):
        q = np.float32(np.r_[rs.uniform(-1, 1, 7) + [0, -0.5, 0, 1.7, 0, -0.8, 0], rs.uniform(0, 0.035, 2)])
        qd = np.float32(np.r_[rs.uniform(-2, 2, 7), rs.uniform(-0.1, 0.1, 2)])
        tau = np.float32(rs.uniform(-1, 1, 9))
        out.append((q, qd, tau))
    return out


def dynamics_cases_wide():
    """... plus 256 poses across the joint ranges, the start pose (at rest and moving), and poses AT the joint limits: all
    joints low, all high, alternating, and every arm joint alone at either limit"""
    out = dynamics_cases_basic()
    rs = np.random.RandomState(21)
    for _ in range(256):
        q = np.float32(rs.uniform(JLO, JHI))
        out.append((q, np.float32(np.r_[rs.uniform(-2, 2, 7), rs.uniform(-0.1, 0.1, 2)]), np.float32(rs.uniform(-1, 1, 9))))
    out.append((Q_START.copy(), np.zeros(9, np.float32), np.zeros(9, np.float32)))
    out.append((Q_START.copy(), np.float32(np.r_[rs.uniform(-2, 2, 7), rs.uniform(-0.1, 0.1, 2)]), np.float32(rs.uniform(-1, 1, 9))))
    alt = np.where(np.arange(9) % 2 == 0, JLO, JHI)
    limits = [JLO, JHI, alt, JLO + JHI - alt]
    for j in range(7):
        for lim in (JLO, JHI):
            q = Q_START.astype(float)
            q[j] = lim[j]
            limits.append(q)
    for q in limits:
        out.append((np.float32(q), np.float32(np.r_[rs.uniform(-2, 2, 7), rs.uniform(-0.1, 0.1, 2)]), np.float32(rs.uniform(-1, 1, 9))))
    return out


def dynamics_errors(cases, run, f32=False):
    """relative errors against the float64 oracle, per case: qdd / max(1, |qdd_ref|), minv / |minv_ref|, tip position, tip
    rotation.  f32: the oracle's own float32 mode in place of the runner (its spread: how much float32 arithmetic costs)"""
    if not f32:
        q, qd, tau = [np.ascontiguousarray(np.stack([c[k] for c in cases]), np.float32) for k in range(3)]
        qdd, mi, tip = run(q, qd, tau)
    err = np.zeros((len(cases), 4))
    for i, (q1, qd1, tau1) in enumerate(cases):
        a64 = [x.astype(float) for x in (q1, qd1, tau1)]
        ref = O.fdyn(*a64)
        mref = O.minv(a64[0])
        p, R = O.fk_tip(a64[0])
        if f32:
            g_qdd, g_mi = O.fdyn(*a64, f32=True), O.minv(a64[0], f32=True)
            gp, gR = O.fk_tip(a64[0], f32=True)
        else:
            g_qdd, g_mi, gp, gR = qdd[i], mi[i].reshape(9, 9), tip[i, :3], tip[i, 3:].reshape(3, 3)
        err[i] = [np.abs(g_qdd - ref).max() / max(1.0, np.abs(ref).max()), np.abs(g_mi - mref).max() / np.abs(mref).max(),
                  np.abs(gp - p).max(), np.abs(gR - R).max()]
    return err


DYN_BARS = (2e-5, 1e-5, 1e-6, 1e-6)      # qdd, minv (float32 Gauss-Jordan, cond(M) ~ 1e3), tip position, tip rotation


def check_dynamics(cases, run, bars=DYN_BARS):
    err = dynamics_errors(cases, run)
    worst = err.max(0)
    for k, name in enumerate(('qdd', 'minv', 'tip position', 'tip rotation')):
        assert worst[k] < bars[k], '%s: %.3g >= %.3g (case %d of %d)' % (name, worst[k], bars[k], int(err[:, k].argmax()), len(cases))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# inverse kinematics
def ik_cases_basic():
    return [(Q_START.copy(), np.float32(t)) for t in ([-0.52, 0.0, 0.25], [-0.45, 0.1, 0.30])]


def ik_cases_wide():
    """... plus 256 targets inside the workspace box, its eight corners, and targets outside it (beyond every face, and out
    of the arm's reach altogether), from the start pose and from poses the IK itself reached"""
    out = ik_cases_basic()
    rs = np.random.RandomState(31)
    starts = [Q_START]
    for t in ([-0.6, -0.15, 0.2], [-0.4, 0.15, 0.5], [-0.52, 0.0, 0.4]):
        q, _ = O.ik(Q_START.astype(float), t)
        starts.append(np.float32(q))
    for i in range(256):
        out.append((starts[i % 4].copy(), np.float32(rs.uniform(EE_LO, EE_HI))))
    for cx in (EE_LO[0], EE_HI[0]):
        for cy in (EE_LO[1], EE_HI[1]):
            for cz in (EE_LO[2], EE_HI[2]):
                out.append((Q_START.copy(), np.float32([cx, cy, cz])))
    mid = 0.5 * (EE_LO + EE_HI)
    for a in range(3):
        for s in (-1, 1):
            t = mid.copy()
            t[a] += s * (0.5 * (EE_HI[a] - EE_LO[a]) + 0.1)
            out.append((Q_START.copy(), np.float32(t)))
    out.append((Q_START.copy(), np.float32([-1.5, 0.0, 0.3])))          # out of reach
    out.append((Q_START.copy(), np.float32([-0.3, 0.9, 1.2])))
    return out


def ik_errors(cases, run, f32=False):
    if not f32:
        got = run(np.ascontiguousarray(np.stack([c[0] for c in cases]), np.float32), np.ascontiguousarray(np.stack([c[1] for c in cases]), np.float32))
    err = np.zeros(len(cases))
    for i, (q0, tgt) in enumerate(cases):
        ref, _ = O.ik(q0.astype(float), tgt.astype(float))
        g = O.ik(q0.astype(float), tgt.astype(float), f32=True)[0] if f32 else got[i]
        err[i] = np.abs(g - ref).max()
    return err


IK_BAR = 5e-5


def check_ik(cases, run, bar=IK_BAR):
    err = ik_errors(cases, run)
    assert err.max() < bar, 'ik: %.3g >= %.3g (case %d of %d)' % (err.max(), bar, int(err.argmax()), len(cases))
    return err.max()


# ----------------------------------------------------------------------------------------------------------------------
# narrowphase
def _quat_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_pairs_at_first_touch(kind):
    """randomly oriented pairs in the regime the simulation lives in: brought together until the oracle reports the first
    touch, then a little deeper.  -> [(trial, pair [30])], two per trial"""
    from test_oracle_physics import _rot_axis
    rs = np.random.RandomState(4)

    def rot():
        q = rs.normal(size=4); q /= np.linalg.norm(q)
        return _quat_rot(q)
    hb = np.float32([0.015, 0.015, 0.015])
    ha = np.float32([0.0125, 0.005, 0.04]) if kind == 'box' else np.float32([0.03, 0.03, 0.01])
    out = []
    for trial in range(100):
        Ra, Rb = (np.eye(3), np.eye(3)) if trial % 4 == 0 else (rot(), rot())
        if trial % 4 == 1:
            # bodies tilted by <= 3 degrees out of the table plane, any yaw: rim x edge crossings, the extrapolated closest
            # pair and the edge refinement of cyl_box (round 4) are taken here
            Ra = _rot_axis(rs.normal(size=3), rs.uniform(0, 0.05))
            Rb = _rot_axis(rs.normal(size=3), rs.uniform(0, 0.05)) @ _rot_axis(np.array([0.0, 0.0, 1.0]), rs.uniform(0, 2 * np.pi))
        cb = rs.uniform(-0.1, 0.1, 3)
        u = rs.normal(size=3); u /= np.linalg.norm(u)
        for step in range(0, 200):
            ca = cb + u * (0.09 - 0.0005 * step)
            ref = (O.box_box(ca, Ra.ravel(), ha, cb, Rb.ravel(), hb) if kind == 'box'
                   else O.cyl_box(ca, Ra.ravel(), 0.03, 0.01, cb, Rb.ravel(), hb))
            if len(ref):
                break
        for extra in (0.0, 0.0007):                       # at first touch and slightly deeper
            ca2 = np.float32(ca - u * extra)
            out.append((trial, pack_pair(ca2, Ra.ravel(), ha, cb, Rb.ravel(), hb)))
    return out


def oracle_pair(kind, pair, f32=False):
    a = [x.astype(float) for x in unpack_pair(pair)]
    if kind == 'box':
        return O.box_box(*a, f32=f32)
    return O.cyl_box(a[0], a[1], 0.03, 0.01, a[3], a[4], np.float32([0.015, 0.015, 0.015]), f32=f32)


# strict bars (normal, depth, points) and the loose ones of an ill-conditioned closest pair
NP_STRICT = (2e-4, 2e-5, 5e-5)
NP_LOOSE = (2e-2, 1e-4, 1e-2)


def check_random_pairs(kind, run, strict=NP_STRICT, results=None):
    """same number of points, normals, depths and witness points as the oracle; -> the largest errors of the strictly
    checked pairs (normal, depth, points).  results: [(n, out [40])] per case from another source instead of the runner"""
    cases = random_pairs_at_first_touch(kind)
    if results is None:
        ns, outs, _ = run(NP_FAST if kind == 'box' else NP_CYL, np.stack([p for _, p in cases]))
        results = list(zip(ns, outs))
    checked = tilted = loose = general_loose = 0
    worst = np.zeros(3)
    for (trial, pair), (n, out) in zip(cases, results):
        ref = oracle_pair(kind, pair)
        n = int(n)
        got = np.asarray(out).reshape(4, 10)[:n]
        if n != len(ref):
            # a point sitting exactly on the margin / a tie between axes may flip between float32 and float64
            assert abs(n - len(ref)) <= 1 and (len(ref) == 0 or np.abs(ref[:, 9]).max() < 0.0021)
            continue
        if n == 0:
            continue
        checked += 1
        order_g, order_r = np.lexsort(got[:, :3].round(4).T), np.lexsort(ref[:, :3].round(4).T)
        en = np.abs(got[order_g][:, 6:9] - ref[order_r][:, 6:9]).max()
        ed = np.abs(got[order_g][:, 9] - ref[order_r][:, 9]).max()
        ep = np.abs(got[order_g][:, 0:6] - ref[order_r][:, 0:6]).max()
        if trial % 4 == 1:
            # two almost parallel features: the closest pair's position along them, and with it the last third of a degree
            # of the normal, is ill-conditioned -- float32 and float64 settle on different points of a flat minimum.
            # The depth is not: strict bar on it, loose bars on the rest, and a count of the strict misses
            tilted += 1
            assert ed < NP_LOOSE[1] and en < NP_LOOSE[0] and ep < NP_LOOSE[2], (en, ed, ep)
            loose += int(en >= strict[0] or ed >= strict[1] or ep >= strict[2])
            continue
        if not (en < strict[0] and ed < strict[1] and ep < strict[2]):
            # (cyl, any orientation) the closest-feature direction of two features that are nearly parallel by chance
            general_loose += 1
            assert kind == 'cyl' and ed < NP_LOOSE[1] and en < NP_LOOSE[0] and ep < NP_LOOSE[2], (en, ed, ep)
            continue
        worst = np.maximum(worst, [en, ed, ep])
    print('tilted pairs %d, beyond the strict bars %d; other pairs %d, beyond the strict bars %d; largest strict errors %s'
          % (tilted, loose, checked - tilted, general_loose, worst))
    assert loose <= 0.25 * max(tilted, 1) and general_loose <= 0.03 * checked
    assert checked > 130
    return worst


def corner_in_side_cases():
    """a box corner touching / inside the cylinder's side (a finger's edge against the puck) -> [(yoff, gap, pair)]"""
    I = np.eye(3, dtype=np.float32).ravel()
    cc, ha, hb = np.float32([-0.495, 0.0979, 0.17]), np.float32([0.03, 0.03, 0.01]), np.float32([0.0125, 0.005, 0.04])
    out = []
    for yoff in (0.0157, 0.0257):
        for gap in np.arange(0.042, 0.028, -0.001):
            cb = np.float32([cc[0] + gap, cc[1] + yoff, 0.207])
            out.append((yoff, gap, pack_pair(cc, I, ha, cb, I, hb)))
    return out


def check_corner_in_side(run):
    cases = corner_in_side_cases()
    ns, outs, _ = run(NP_CYL, np.stack([c[2] for c in cases]))
    checked = 0
    for (yoff, gap, pair), n, out in zip(cases, ns, outs):
        a = [x.astype(float) for x in unpack_pair(pair)]
        ref = O.cyl_box(a[0], a[1], 0.03, 0.01, a[3], a[4], a[5])
        n = int(n)
        assert n == len(ref), (yoff, gap, n, len(ref))
        if n:
            got = out.reshape(4, 10)[:n]
            assert abs(got[:, 9].min() - ref[:, 9].min()) < 2e-6 and np.abs(got[0, 6:9] - ref[0, 6:9]).max() < 1e-4, (yoff, gap, got[:, 9], ref[:, 9])
            checked += 1
    assert checked > 10


def axis_aligned_cases():
    """fingers in random poses over, in and beside a table-sized axis-aligned box"""
    rs = np.random.RandomState(3)
    ha, hb = np.float32([0.0125, 0.005, 0.04]), np.float32([0.5, 0.4, 0.1])
    Rb = np.eye(3, dtype=np.float32)
    out = []
    for trial in range(600):
        q = rs.normal(size=4) * ([1, 1, 1, 1] if trial % 3 == 0 else [0.02, 0.02, 1, 1]); q /= np.linalg.norm(q)
        Ra = _quat_rot(q)
        ext = np.abs(Ra[2]) @ ha                                     # the finger's half extent along z
        cb = np.float32([0, 0, 0])
        ca = np.float32([rs.uniform(-0.52, 0.52), rs.uniform(-0.42, 0.42), 0.1 + ext + rs.uniform(-0.002, 0.003)])
        out.append(pack_pair(ca, Ra.ravel(), ha, cb, Rb.ravel(), hb))
    return np.stack(out)


def check_two_routines_bit_identical(pairs, run, kind_new, kind_old):
    """same contacts, same bits from the two routines on every pair -> (n of the new routine, per pair)"""
    n1, o1, _ = run(kind_new, pairs)
    n2, o2, _ = run(kind_old, pairs)
    for t in range(len(pairs)):
        assert n1[t] == n2[t], (t, n1[t], n2[t])
        k = 10 * int(n1[t])
        assert np.array_equal(o1[t][:k].view(np.uint32), o2[t][:k].view(np.uint32)), (t, o1[t][:k], o2[t][:k])
    return np.asarray(n1)


def check_two_routines_agree(pairs, run, kind_new, kind_old, bars=NP_STRICT):
    """what holds of the two routines where their bits may differ (another compiler contracts the multiply-adds of the two
    instantiations differently): the same number of contacts on every pair, the points in the same order, and normals /
    depths / points within the strict narrowphase bars of each other.  -> (n of the new routine per pair, pairs whose bits
    differ, largest differences (normal, depth, points))"""
    n1, o1, _ = run(kind_new, pairs)
    n2, o2, _ = run(kind_old, pairs)
    differ = np.nonzero(n1 != n2)[0]
    assert len(differ) == 0, 'contact counts differ on %d of %d pairs, first %s: %s vs %s' % (len(differ), len(pairs), differ[:8], n1[differ[:8]], n2[differ[:8]])
    worst, bits = np.zeros(3), 0
    for t in range(len(pairs)):
        k = int(n1[t])
        if k == 0:
            continue
        a, b = o1[t].reshape(4, 10)[:k].astype(np.float64), o2[t].reshape(4, 10)[:k].astype(np.float64)
        bits += int(not np.array_equal(o1[t][:10 * k].view(np.uint32), o2[t][:10 * k].view(np.uint32)))
        worst = np.maximum(worst, [np.abs(a[:, 6:9] - b[:, 6:9]).max(), np.abs(a[:, 9] - b[:, 9]).max(), np.abs(a[:, 0:6] - b[:, 0:6]).max()])
    print('pairs in contact %d, with different bits %d; largest differences (normal, depth, points) %s' % (int((n1 > 0).sum()), bits, worst))
    assert worst[0] < bars[0] and worst[1] < bars[1] and worst[2] < bars[2], worst
    return np.asarray(n1), bits, worst


def flush_stack_cases():
    """cubes stacked off-centre with their side faces FLUSH, a cube flush with the edge of a table-sized box, a finger flush with
    a cube's side: vertices of the incident face lie exactly ON the clip planes of the reference face (every number here is
    the same float32 on both sides of the comparison).  What block_stack builds.  -> [(pair, points expected)]"""
    I = np.eye(3).ravel()
    cube, table, finger = [0.015] * 3, [0.5, 0.5, 0.1], [0.0125, 0.005, 0.04]
    out = []
    for dx in (0.005, 0.01, 0.02, -0.01):
        for dz in (0.03, 0.0295, 0.031):
            out.append((pack_pair([dx, 0.0, dz], I, cube, [0, 0, 0], I, cube), 4))              # flush in y, shifted in x
            out.append((pack_pair([0.0, dx, dz], I, cube, [0, 0, 0], I, cube), 4))              # flush in x, shifted in y
            out.append((pack_pair([dx, dx, dz], I, cube, [0, 0, 0], I, cube), 4))               # shifted in both (no vertex on a plane)
    for dz in (0.115, 0.1145, 0.116):
        out.append((pack_pair([0.5, 0.0, dz], I, cube, [0, 0, 0], I, table), 4))                 # half over the table's edge, flush in nothing
        out.append((pack_pair([0.485, 0.485, dz], I, cube, [0, 0, 0], I, table), 4))             # in the table's corner, flush with two sides
    out.append((pack_pair([0.0025, 0.0, 0.055], I, finger, [0, 0, 0], I, cube), 4))              # finger on a cube, its side flush with the cube's
    return out


def check_flush_stacks(run, kind=NP_FAST):
    """the oracle's count and contacts on every flush pair, to the strict bars"""
    cases = flush_stack_cases()
    ns, outs, _ = run(kind, np.stack([p for p, _ in cases]))
    for t, (pair, want) in enumerate(cases):
        a = [x.astype(float) for x in unpack_pair(pair)]
        ref = O.box_box(*a)
        assert len(ref) == want, (t, len(ref), want)
        n = int(ns[t])
        assert n == len(ref), (t, n, len(ref), pair[:3])
        got = outs[t].reshape(4, 10)[:n]
        order_g, order_r = np.lexsort(got[:, :3].round(4).T), np.lexsort(ref[:, :3].round(4).T)
        en = np.abs(got[order_g][:, 6:9] - ref[order_r][:, 6:9]).max()
        ed = np.abs(got[order_g][:, 9] - ref[order_r][:, 9]).max()
        ep = np.abs(got[order_g][:, 0:6] - ref[order_r][:, 0:6]).max()
        assert en < NP_STRICT[0] and ed < NP_STRICT[1] and ep < NP_STRICT[2], (t, en, ed, ep)
    return len(cases)


def face_clip_cases():
    """fingers against cubes, cubes on cubes and cubes on a table-sized box, in random orientations, touching, deeper and with
    more than four clipped vertices inside the margin"""
    rs = np.random.RandomState(11)

    def rot(small):
        q = rs.normal(size=4) * ([small, small, 1.0, 1.0] if small else 1.0); q /= np.linalg.norm(q)
        return _quat_rot(q)
    shapes = [(np.float32([0.0125, 0.005, 0.04]), np.float32([0.015] * 3)),      # finger x cube
              (np.float32([0.015] * 3), np.float32([0.015] * 3)),                # cube x cube
              (np.float32([0.015] * 3), np.float32([0.5, 0.5, 0.1]))]            # cube x table-sized box
    out = []
    for trial in range(900):
        ha, hb = shapes[trial % 3]
        small = 0.0 if trial % 2 else rs.choice([0.003, 0.03, 0.3])               # nearly face-parallel poses clip most
        Ra, Rb = rot(small), (np.eye(3) if trial % 5 else rot(small))
        n_ax = Rb[:, rs.randint(3)] * rs.choice([-1, 1])
        reach = np.abs(Ra.T @ n_ax) @ ha + np.abs(Rb.T @ n_ax) @ hb
        lateral = rs.normal(size=3); lateral -= n_ax * (lateral @ n_ax)
        lateral *= rs.uniform(0, 1) * float(min(hb.min(), 0.03)) / max(np.linalg.norm(lateral), 1e-9)
        cb = rs.uniform(-0.1, 0.1, 3)
        ca = cb + n_ax * (reach - rs.uniform(-0.001, 0.003)) + lateral
        out.append(pack_pair(ca, Ra.ravel(), ha, cb, Rb.ravel(), hb))
    return np.stack(out)


# ----------------------------------------------------------------------------------------------------------------------
# the double-precision helpers of the cylinder repeat
def quat_R64(q):
    x, y, z, w = [float(v) for v in q]
    s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz, xx, xy, xz, yy, yz, zz = w * xs, w * ys, w * zs, x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
    return np.array([[1 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1 - (xx + yy)]])


FK64_BODIES = ((7, 12), (5, 13), (6, 15))                 # (contact body, Bullet link): BODY_GBASE, BODY_FINGER1, BODY_FINGER2


def fk64_edge_poses():
    """where sincos64 changes its path: all joints at JLO, at JHI, alternating; each arm joint alone at either limit (the
    quadrant becomes +-2 there) and, where inside its range, at the quadrant switch points +-pi/4 and +-3 pi/4, at +-pi/2, 0,
    1e-8 and -1e-30; every one of these also one float32 step above and below (clipped to nothing: the routine takes any
    float32 angle of |q| <= 3.06).  -> [float32 q9]"""
    alt = np.where(np.arange(9) % 2 == 0, JLO, JHI)
    out = [np.float32(q) for q in (JLO, JHI, alt, JLO + JHI - alt)]
    for j in range(7):
        for v in (JLO[j], JHI[j], np.pi / 4, -np.pi / 4, 3 * np.pi / 4, -3 * np.pi / 4, np.pi / 2, -np.pi / 2, 0.0, 1e-8, -1e-30):
            if not JLO[j] <= v <= JHI[j]:
                continue
            v32 = np.float32(v)
            for w in (v32, np.nextafter(v32, np.float32(4)), np.nextafter(v32, np.float32(-4))):
                q = Q_START.copy()
                q[j] = w
                out.append(q)
    return out


def check_fk64(run):
    """fk64_link against the float64 oracle's kinematics() through its Bullet-call-level world: link frames of Bullet links
    12 / 13 / 15 at 20 random poses and at the edge poses of fk64_edge_poses(), to 1e-12.  -> the largest error"""
    ora = O.OracleEnv('reach', 1, seed_base=0)
    ora.reset()
    ol = ora.lib
    rs = np.random.RandomState(3)
    qs = [np.float32(np.concatenate([rs.uniform(-2, 2, 7), rs.uniform(0, 0.035, 2)])) for _ in range(20)]
    edges = fk64_edge_poses()
    assert len(edges) >= 4 + 3 * 7 * 6
    qs += edges
    q9 = np.ascontiguousarray(np.repeat(np.stack(qs), 3, axis=0), np.float32)
    body = np.ascontiguousarray(np.tile([b for b, _ in FK64_BODIES], len(qs)), np.int32)
    p, R = run(q9, body)
    worst = 0.0
    for trial, q in enumerate(qs):
        for d in range(9):
            ol.pmgo_bw_reset_joint(ora.h, 0, d, C.c_double(float(q[d])), C.c_double(0.0))
        for k, (b, link) in enumerate(FK64_BODIES):
            ref = np.zeros(13)
            ol.pmgo_bw_link_state(ora.h, link, _fp(ref))
            i = 3 * trial + k
            ep, eR = np.abs(p[i] - ref[:3]).max(), np.abs(R[i].reshape(3, 3) - quat_R64(ref[3:7])).max()
            assert ep < 1e-12 and eR < 1e-12, (trial, b, q, ep, eR)
            worst = max(worst, ep, eR)
    ora.close()
    print('fk64_link: %d poses, largest error %.3g' % (len(qs), worst))
    return worst


def cyl_redo64_cases():
    """the slide puck -- any small tilt, any yaw -- against the table and near its edge -> state rows [300][13], kc [24]"""
    rs = np.random.RandomState(5)
    blks = []
    for trial in range(300):
        tilt = 10.0 ** rs.uniform(-8, -1.5) * rs.normal(size=2)
        yaw = rs.uniform(0, 2 * np.pi)
        quat = np.array([tilt[0] / 2, tilt[1] / 2, np.sin(yaw / 2), np.cos(yaw / 2)])
        quat /= np.linalg.norm(quat)
        edge = trial % 3 == 0
        blk = np.zeros(13, np.float32)
        blk[0:3] = [-0.70 + (0.5 - rs.uniform(0, 0.04) if edge else rs.uniform(-0.3, 0.3)), rs.uniform(-0.3, 0.3), 0.16 + 0.01 + rs.uniform(-2e-4, 1.5e-3)]
        blk[3:7] = quat
        blks.append(blk)
    tc, th = np.float32([-0.70, 0.0, 0.08]), np.float32([0.5, 0.45, 0.08])
    kc = np.zeros(24, np.float32); kc[0:3] = tc; kc[3:6] = th
    return np.stack(blks), kc


def check_cyl_redo64(run_redo, run_pairs):
    """cyl_redo64 against the float64 oracle's cyl_box on the same poses: same count, points and normals to 1e-6 (the outputs
    are float32), depths to 1e-8.  Beside it the float32 pass on float32 poses: its gross disagreements with the oracle are
    counted (the resting puck has none: the repeat is for vertex / edge contacts)"""
    blks, kc = cyl_redo64_cases()
    tc, th = kc[0:3], kc[3:6]
    I3 = np.eye(3)
    ns, outs = run_redo(blks, kc)
    fpairs = np.stack([pack_pair(b[0:3], np.float32(quat_R64(b[3:7])).ravel(), np.float32([0.03, 0.03, 0.01]), tc, np.float32(I3).ravel(), th) for b in blks])
    nfs, outfs, ambs = run_pairs(NP_CYL, fpairs)
    checked = flagged = gross_unflagged = 0
    for trial, blk in enumerate(blks):
        n = int(ns[trial])
        R = quat_R64(blk[3:7])
        ref = O.cyl_box(blk[0:3].astype(float), R.ravel(), 0.03, 0.01, tc.astype(float), I3.ravel(), th.astype(float))
        assert n == len(ref), (trial, n, len(ref))
        if n == 0:
            continue
        got = outs[trial].reshape(4, 10)[:n]
        assert np.abs(got[:, 6:9] - ref[:, 6:9]).max() < 1e-6 and np.abs(got[:, 9] - ref[:, 9]).max() < 1e-8 and np.abs(got[:, 0:6] - ref[:, 0:6]).max() < 1e-6, (trial, got, ref)
        checked += 1
        nf, amb = int(nfs[trial]), float(ambs[trial])          # the float pass: float32 poses
        gf = outfs[trial].reshape(4, 10)[:nf]
        # gross: another number of points, another normal, a point 3 mm from the oracle's or 20 um deeper (two candidates of the
        # same depth 1 mm apart on the rim may swap in the reduction to four points: not a different contact)
        gross = nf != n or np.abs(np.sort(gf[:, 0:3], axis=0) - np.sort(ref[:, 0:3], axis=0)).max() > 3e-3 or np.abs(gf[0, 6:9] - ref[0, 6:9]).max() > 1e-2 \
            or np.abs(np.sort(gf[:, 9]) - np.sort(ref[:, 9])).max() > 2e-5
        flagged += int(amb < 1.0)
        gross_unflagged += int(gross and not amb < 1.0)
    print('cylinder pairs in contact %d, float pass flagged ambiguous %d, gross float32 answers not flagged %d' % (checked, flagged, gross_unflagged))
    assert checked > 150 and gross_unflagged <= 0.02 * checked and flagged < 0.2 * checked


# ----------------------------------------------------------------------------------------------------------------------
# cyl_redo64 on EVERY pair collide() hands it.  Every reference value below comes from the float64 oracle and from
# tests/golden/model.json; nothing from include/pmg_model.h, nothing from the device
REDO_STATIC, REDO_FINGER1, REDO_FINGER2, REDO_GBASE, REDO_DOOR, REDO_HANDLE = -1, 5, 6, 7, 8, 100      # the ids of the call
DM_SQRT, DM_DIV, DM_SINCOS = 0, 1, 2
MODEL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'model.json')))
FINGER_H = np.array(MODEL['finger_half'])
CUBE_H = np.array(MODEL['block']['ext']) / 2
PUCK_R, PUCK_HL = MODEL['puck']['ext'][0] / 2, MODEL['puck']['ext'][2] / 2
GBASE_R, GBASE_HL = MODEL['gbase_radius'], MODEL['gbase_halflen']
PLANE_H = np.array(MODEL['plane']['ext']) / 2
SLIDE_TABLE_C, SLIDE_TABLE_H = np.array([-0.70, 0.0, 0.08]), np.array(MODEL['long_table']['ext']) / 2
PLANE_SWITCH_Z = 0.04                  # (oracle/pmg_oracle.c) a free body below it meets the floor, above it the table
REDO_BARS = (1e-6, 1e-8, 1e-6)         # normal, depth, points: the bars of check_cyl_redo64
_LINK = {REDO_GBASE: 12, REDO_FINGER1: 13, REDO_FINGER2: 15}
FAR_ROW = np.float32([3.0, 3.0, 3.0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])       # the other free-body row: identity, far away


def redo_kc():
    """the env's constant table as far as cyl_redo64 reads it: table centre / half at 0 / 3, cube half at 18, floor half at 21"""
    kc = np.zeros(24, np.float32)
    kc[0:3], kc[3:6], kc[18:21], kc[21:24] = SLIDE_TABLE_C, SLIDE_TABLE_H, CUBE_H, PLANE_H
    kc[6:15] = np.eye(3).ravel()
    return kc


class _Arm:
    """double poses of the contact links from float32 joint angles: the oracle's Bullet-call-level world, as check_fk64"""

    def __init__(self):
        self.ora = O.OracleEnv('reach', 1, seed_base=0)
        self.ora.reset()

    def pose(self, q9, body):
        ol, ref = self.ora.lib, np.zeros(13)
        for d in range(9):
            ol.pmgo_bw_reset_joint(self.ora.h, 0, d, C.c_double(float(np.float32(q9[d]))), C.c_double(0.0))
        ol.pmgo_bw_link_state(self.ora.h, _LINK[body], _fp(ref))
        return ref[:3].copy(), quat_R64(ref[3:7])


@functools.lru_cache(None)
def chest_base(ck):
    """where the chest stands, from the oracle's reset observation of a chest env (the door's first key point, float32, less the
    door's and the key point's offsets of model.json), rounded to the micrometre the layout is written in"""
    ch = MODEL['chest'][ck]
    ora = O.OracleEnv(('chest_push', 'chest_pick_and_place')[ck], 1, num_block=1, seed_base=5, seed_stride=1)
    ora.reset()
    obs = ora.reset()['observation'][0]
    ora.close()
    kp = obs[8 + 16:][2:].reshape(3, 6)[:, :3].astype(float)
    base = [np.round(kp[k] - ch['door_c'] - ch['keypoints'][k], 6) for k in range(3)]
    assert np.array_equal(base[0], base[1]) and np.array_equal(base[0], base[2]), base
    return base[0] + 0.0


def redo_geometry(arm, ck, cyl, box, wall, q9, blk, doorq, kc):
    """the operands cyl_redo64 is to assemble for this call, from the oracle and model.json: -> cc, Rc, rad, hl, cb, Rb, hb"""
    I3 = np.eye(3)
    if ck >= 0:
        ch = MODEL['chest'][ck]
        dc = chest_base(ck) + np.array(ch['door_c']) + np.array(ch['axis']) * float(np.float32(doorq))
    if cyl == REDO_GBASE:
        (cc, Rc), rad, hl = arm.pose(q9, REDO_GBASE), GBASE_R, GBASE_HL
    elif cyl == REDO_HANDLE:
        cc, Rc, rad, hl = dc + np.array(ch['handle_c']), np.array(ch['handle_R']), ch['handle_radius'], ch['handle_halflen']
    else:
        cc, Rc, rad, hl = blk[cyl, 0:3].astype(float), quat_R64(blk[cyl, 3:7]), PUCK_R, PUCK_HL
    if box in (REDO_FINGER1, REDO_FINGER2):
        (cb, Rb), hb = arm.pose(q9, box), FINGER_H
    elif box == REDO_DOOR:
        cb, Rb, hb = dc, I3, np.array(ch['door_half'])
    elif box == REDO_STATIC and wall >= 0:
        w = ch['walls'][wall]
        cb, Rb, hb = chest_base(ck) + np.array(w['c']), I3, np.array(w['half'])
    elif box == REDO_STATIC:
        if blk[cyl, 2] < np.float32(PLANE_SWITCH_Z):
            cb, Rb, hb = np.zeros(3), I3, kc[21:24].astype(float)
        else:
            cb, Rb, hb = kc[0:3].astype(float), I3, kc[3:6].astype(float)
    else:
        cb, Rb, hb = blk[box, 0:3].astype(float), quat_R64(blk[box, 3:7]), kc[18:21].astype(float)
    return cc, Rc, rad, hl, cb, Rb, hb


def _oracle_cyl(g, margin=0.002, f32=False):
    return O.cyl_box(g[0], np.asarray(g[1]).ravel(), g[2], g[3], g[4], np.asarray(g[5]).ravel(), g[6], margin=margin, f32=f32)


def _unit(rs):
    u = rs.normal(size=3)
    return u / np.linalg.norm(u)


def _rand_quat(rs):
    q = rs.normal(size=4)
    return np.float32(q / np.linalg.norm(q))


def _support_box(R, h, u):
    return float(np.abs(np.asarray(R).T @ u) @ h)


def _support_cyl(R, rad, hl, u):
    a = float(np.asarray(R)[:, 2] @ u)
    return abs(a) * hl + rad * np.sqrt(max(0.0, 1.0 - a * a))


def _first_touch(count_at, d0, coarse=0.002, fine=0.0003):
    """d walked down from d0 (out of contact by a separating axis) in 0.3 mm steps until the oracle reports the first touch; the
    first 2 mm strides only skip the empty part of the way.  -> d, or None (never touched within 25 cm / touched at the start)"""
    d = d0
    if count_at(d):
        return None
    while not count_at(d - coarse):
        d -= coarse
        if d < d0 - 0.25:
            return None
    while not count_at(d):
        d -= fine
    return d


class _Cases:
    def __init__(self, ck):
        self.ck, self.rows, self.ids, self.q9, self.blk, self.door, self.geo, self.ref = ck, [], [], [], [], [], [], []
        self.dropped = 0

    def add(self, arm, row, cyl, box, wall, q9, blk, doorq, kc):
        q9, blk, doorq = np.float32(q9), np.float32(blk).reshape(2, 13), np.float32(doorq)
        g = redo_geometry(arm, self.ck, cyl, box, wall, q9, blk, doorq, kc)
        ref = _oracle_cyl(g)
        # a count that hinges on the margin: a candidate within 1e-7 of the 2 mm -- the oracle itself answers differently there
        if len(_oracle_cyl(g, 0.002 + 1e-7)) != len(ref) or len(_oracle_cyl(g, 0.002 - 1e-7)) != len(ref):
            self.dropped += 1
            return
        self.rows.append(row); self.ids.append([cyl, box, wall, 0]); self.q9.append(q9); self.blk.append(blk); self.door.append(doorq)
        self.geo.append(g); self.ref.append(ref)

    def done(self, kc):
        n = len(self.rows)
        assert self.dropped <= 0.02 * (n + self.dropped), (self.dropped, n)
        return dict(ck=self.ck, kc=kc, rows=np.array(self.rows), ids=np.array(self.ids, np.int32), q9=np.stack(self.q9), blk=np.stack(self.blk),
                    doorq=np.array(self.door, np.float32), geo=self.geo, ref=self.ref, nref=np.array([len(r) for r in self.ref]), dropped=self.dropped)


def _free_body_walks(cs, arm, rs, row, kc, n_walks, robot_body, free_is_cyl, rows_of_state, aligned_third):
    """a free body (the cube against the gripper base / the puck against a finger) walked in towards a robot link held at a pose
    anywhere in the joint ranges; at first touch one case 0 - 1.5 mm deeper, and from every fourth walk one 0.3 - 2.5 mm back out"""
    made = 0
    while made < n_walks:
        q9 = np.float32(np.r_[rs.uniform(JLO[:7], JHI[:7]), rs.uniform(0, 0.035, 2)])
        pr, Rr = arm.pose(q9, robot_body)
        quat = np.float32([0, 0, 0, 1]) if aligned_third and made % 3 == 0 else _rand_quat(rs)
        Rf, u = quat_R64(quat), _unit(rs)
        lateral = rs.uniform(-0.5, 0.5, 3) * (0.03 if free_is_cyl else 0.04)
        lateral -= u * (lateral @ u)
        sr = _support_cyl(Rr, GBASE_R, GBASE_HL, u) if robot_body == REDO_GBASE else _support_box(Rr, FINGER_H, u)
        sf = _support_cyl(Rf, PUCK_R, PUCK_HL, u) if free_is_cyl else _support_box(Rf, CUBE_H, u)
        slot = rows_of_state[made % len(rows_of_state)]

        def state(d):
            blk = np.stack([FAR_ROW, FAR_ROW])
            blk[slot, 0:3] = pr + lateral + u * d
            blk[slot, 3:7] = quat
            return blk
        ids = (slot, robot_body, -1) if free_is_cyl else (REDO_GBASE, slot, -1)

        def count(d):
            return len(_oracle_cyl(redo_geometry(arm, cs.ck, ids[0], ids[1], -1, q9, state(d), 0.0, kc)))
        d = _first_touch(count, sr + sf + 0.0025)
        if d is None:
            continue
        cs.add(arm, row, ids[0], ids[1], -1, q9, state(d - rs.uniform(0, 0.0015)), rs.uniform(0, 0.1), kc)
        if made % 4 == 0:
            cs.add(arm, row, ids[0], ids[1], -1, q9, state(d + rs.uniform(0.0003, 0.0025)), rs.uniform(0, 0.1), kc)
        made += 1


def _puck_static_cases(cs, arm, rs, kc):
    q9 = Q_START

    def blk_of(pos, quat):
        blk = np.stack([FAR_ROW, FAR_ROW])
        blk[0, 0:3], blk[0, 3:7] = pos, quat
        return blk

    def tilted():
        tilt = 10.0 ** rs.uniform(-8, -1) * _unit(rs)[:2]
        yaw = rs.uniform(0, 2 * np.pi)
        quat = np.array([tilt[0] / 2, tilt[1] / 2, np.sin(yaw / 2), np.cos(yaw / 2)])
        return np.float32(quat / np.linalg.norm(quat))
    for trial in range(90):                             # the floor: anywhere on the 5 x 5 m plane, a third of them at its edge
        xy = rs.uniform(-2.45, 2.45, 2)
        if trial % 3 == 0:
            xy[rs.randint(2)] = rs.choice([-1, 1]) * (PLANE_H[0] - rs.uniform(0, 0.04))
        cs.add(arm, 'puck x floor', 0, REDO_STATIC, -1, q9, blk_of([xy[0], xy[1], PLANE_H[2] + PUCK_HL + rs.uniform(-2e-4, 1.5e-3)], tilted()), 0.0, kc)
    made = 0
    while made < 60:                                    # the table's side walls: the puck beside the table, above the switch
        ax, sg = rs.randint(2), rs.choice([-1, 1])
        quat = tilted() if made % 2 else _rand_quat(rs)
        Rf = quat_R64(quat)
        u = np.zeros(3); u[ax] = sg
        base = SLIDE_TABLE_C.copy()
        base[1 - ax] += rs.uniform(-0.9, 0.9) * SLIDE_TABLE_H[1 - ax]
        base[2] = rs.uniform(0.075, 0.15)
        base[ax] += sg * SLIDE_TABLE_H[ax]

        def count(d):
            return len(_oracle_cyl(redo_geometry(arm, cs.ck, 0, REDO_STATIC, -1, q9, blk_of(base + u * d, quat), 0.0, kc)))
        d = _first_touch(count, _support_cyl(Rf, PUCK_R, PUCK_HL, u) + 0.0025)
        if d is None:
            continue
        cs.add(arm, 'puck x table side', 0, REDO_STATIC, -1, q9, blk_of(base + u * (d - rs.uniform(0, 0.0015)), quat), 0.0, kc)
        if made % 3 == 0:
            cs.add(arm, 'puck x table side', 0, REDO_STATIC, -1, q9, blk_of(base + u * (d + rs.uniform(0.0003, 0.0025)), quat), 0.0, kc)
        made += 1


def _arm_walks(cs, arm, rs, row, kc, n_walks, cyl, box, wall):
    """a chest pair: the robot link (a finger against the handle, the gripper base against the door / lid / a wall) brought to
    its partner BY THE ARM -- oracle_lib.ik on targets around the partner, the pose goes through q9 -- along a random direction
    until the oracle reports the first touch; from every walk one case 0 - 1.5 mm deeper and one 0.3 - 2.5 mm back out (out of
    contact, within 5 mm of it).  The door joint: 0, its upper limit, anywhere between"""
    ck = cs.ck
    ch = MODEL['chest'][ck]
    body = REDO_GBASE if cyl == REDO_GBASE else box
    blk = np.stack([FAR_ROW, FAR_ROW])
    made = tries = 0
    while made < n_walks:
        tries += 1
        assert tries < 20 * n_walks, (row, made, tries)
        doorq = np.float32((0.0, ch['upper'], rs.uniform(0, ch['upper']))[made % 3])
        fingers = rs.uniform(0, 0.035, 2)
        g0 = redo_geometry(arm, ck, cyl, box, wall, Q_START, blk, doorq, kc)
        # the partner: where it is and how far it reaches along u (the link's own reach from its pose once the arm is there)
        if cyl == REDO_HANDLE:
            pc, reach = g0[0], lambda u: _support_cyl(g0[1], g0[2], g0[3], u)
            inside = g0[1] @ (rs.uniform(-0.8, 0.8, 3) * [g0[2], g0[2], g0[3]])
        else:
            pc, reach = g0[4], lambda u: _support_box(g0[5], g0[6], u)
            inside = rs.uniform(-0.9, 0.9, 3) * g0[6]
        u = _unit(rs)
        u[2] = abs(u[2])                                  # from above or from the side: the arm reaches these
        state = dict(q=Q_START.astype(float), off=None)

        def q_at(d):
            want = pc + inside + u * d                    # where the link's centre is to be
            for _ in range(2 if state['off'] is None else 1):
                off = np.zeros(3) if state['off'] is None else state['off']
                q, _ = O.ik(state['q'], want - off, max_iter=120)
                q[7:9] = fingers
                state['q'] = q
                state['off'] = arm.pose(q, body)[0] - O.fk_tip(np.float32(q).astype(float))[0]
            return np.float32(state['q'])

        def count(d):
            return len(_oracle_cyl(redo_geometry(arm, ck, cyl, box, wall, q_at(d), blk, doorq, kc)))
        q_far = q_at(0.12)
        pl, Rl = arm.pose(q_far, body)
        own = _support_cyl(Rl, GBASE_R, GBASE_HL, u) if body == REDO_GBASE else _support_box(Rl, FINGER_H, u)
        d = _first_touch(count, reach(u) - float(inside @ u) + own + 0.004)
        if d is None:
            continue
        q_touch = state['q'].copy()
        n0 = len(cs.rows)
        cs.add(arm, row, cyl, box, wall, q_at(d - rs.uniform(0, 0.0015)), blk, doorq, kc)
        state['q'] = q_touch
        cs.add(arm, row, cyl, box, wall, q_at(d + rs.uniform(0.0003, 0.0025)), blk, doorq, kc)
        made += 1


@functools.lru_cache(None)
def redo_pair_cases(ck):
    """every pair cyl_redo64<ck> serves -> dict(ck, kc, rows [n] (names), ids [n][4], q9 [n][9], blk [n][2][13], doorq [n], geo (the
    oracle-side operands), ref (the oracle's contacts), nref [n], dropped).
    ck -1 (slide and the cube tasks): gripper base x cube, puck x finger 1 / 2, puck x floor, puck x table side wall.
    ck 0 / 1 (the chests): gripper base x cube again, handle x finger 1 / 2, gripper base x door / lid, gripper base x every wall"""
    arm, rs, kc = _Arm(), np.random.RandomState(100 + ck), redo_kc()
    cs = _Cases(ck)
    if ck <= 0:
        _free_body_walks(cs, arm, rs, 'gripper base x cube', kc, 150, REDO_GBASE, False, (1,), True)
    if ck < 0:
        for f, body in enumerate((REDO_FINGER1, REDO_FINGER2)):
            _free_body_walks(cs, arm, rs, 'puck x finger %d' % (f + 1), kc, 80, body, True, (0, 1), False)
        _puck_static_cases(cs, arm, rs, kc)
    else:
        for f, body in enumerate((REDO_FINGER1, REDO_FINGER2)):
            _arm_walks(cs, arm, rs, 'handle x finger %d' % (f + 1), kc, 36, REDO_HANDLE, body, -1)
        _arm_walks(cs, arm, rs, 'gripper base x door', kc, 36, REDO_GBASE, REDO_DOOR, -1)
        for w in range(len(MODEL['chest'][ck]['walls'])):
            _arm_walks(cs, arm, rs, 'gripper base x wall %d' % w, kc, 36, REDO_GBASE, REDO_STATIC, w)
    arm.ora.close()
    return cs.done(kc)


def redo_rows_expected(ck):
    if ck < 0:
        return {'gripper base x cube': 150, 'puck x finger 1': 75, 'puck x finger 2': 75, 'puck x floor': 80, 'puck x table side': 50}
    out = {'handle x finger 1': 30, 'handle x finger 2': 30, 'gripper base x door': 30}
    out.update({'gripper base x wall %d' % w: 30 for w in range(len(MODEL['chest'][ck]['walls']))})
    if ck == 0:
        out['gripper base x cube'] = 150
    return out


def _match_errors(got, ref):
    """largest differences (normal, depth, points) with the points matched by lexsort of their positions as elsewhere; where two
    points tie within the rounding of the sort key, by the best of the <= 24 orders"""
    order_g, order_r = np.lexsort(got[:, :3].round(4).T), np.lexsort(ref[:, :3].round(4).T)
    best = None
    for perm in [order_g] + [np.array(p) for p in itertools.permutations(range(len(got)))]:
        a, b = got[perm].astype(float), ref[order_r]
        e = (np.abs(a[:, 6:9] - b[:, 6:9]).max(), np.abs(a[:, 9] - b[:, 9]).max(), np.abs(a[:, 0:6] - b[:, 0:6]).max())
        if best is None or max(e[0] / REDO_BARS[0], e[1] / REDO_BARS[1], e[2] / REDO_BARS[2]) < max(best[0] / REDO_BARS[0], best[1] / REDO_BARS[1], best[2] / REDO_BARS[2]):
            best = e
        if max(e[0] / REDO_BARS[0], e[1] / REDO_BARS[1], e[2] / REDO_BARS[2]) < 1.0:
            break
    return np.array(best)


def check_redo_pairs(ck, run, handed_bits=True):
    """cyl_redo64<ck> on every pair it serves against the float64 oracle's cyl_box on operands assembled from the oracle and
    model.json: the oracle's count in every case, normals and points to 1e-6, depths to 1e-8; the coverage of every row
    (cases in contact; for the chest rows also cases out of contact) asserted.  Then the same cases with the robot body's pose
    handed in: the same bars, and (handed_bits) the bits of the fetch-inside mode.
    -> (largest errors (normal, depth, points), handed cases whose bits differ, per-row worst errors)"""
    cs = redo_pair_cases(ck)
    need = redo_rows_expected(ck)
    ids = cs['ids'].copy()
    mix = np.random.RandomState(3).permutation(len(ids))      # a launch that takes many cases at once gets every row in it
    back = np.argsort(mix)

    def run_mixed(ids):
        ns, outs = run(ck, ids[mix], cs['q9'][mix], cs['blk'][mix], cs['doorq'][mix], cs['kc'])
        return ns[back], outs[back]
    n0, out0 = run_mixed(ids)
    ids[:, 3] = 1
    n1, out1 = run_mixed(ids)
    worst, per_row, differ = np.zeros(3), {}, 0
    for mode, (ns, outs) in enumerate(((n0, out0), (n1, out1))):
        for i, ref in enumerate(cs['ref']):
            row = cs['rows'][i] + (' (pose handed in)' if mode else '')
            assert int(ns[i]) == len(ref), 'chest kind %d, %s, case %d: %d contacts, the oracle %d' % (ck, row, i, ns[i], len(ref))
            if len(ref) == 0:
                continue
            e = _match_errors(outs[i].reshape(4, 10)[:len(ref)], ref)
            assert (e < REDO_BARS).all(), 'chest kind %d, %s, case %d: normal / depth / points off by %s (bars %s)' % (ck, row, i, e, REDO_BARS)
            worst = np.maximum(worst, e)
            per_row[cs['rows'][i]] = np.maximum(per_row.get(cs['rows'][i], 0), e)
    for i in range(len(ids)):
        k = 10 * int(n0[i])
        same = n0[i] == n1[i] and np.array_equal(out0[i][:k].view(np.uint32), out1[i][:k].view(np.uint32))
        differ += int(not same)
        assert same or not handed_bits, 'chest kind %d, %s, case %d: handed-in pose and fetched pose give different bits' % (ck, cs['rows'][i], i)
        if not same:                                          # what holds where the bits may differ: the same count, the two within the bars
            a, b = out0[i][:k].reshape(-1, 10).astype(float), out1[i][:k].reshape(-1, 10).astype(float)
            e = np.array([np.abs(a[:, 6:9] - b[:, 6:9]).max(), np.abs(a[:, 9] - b[:, 9]).max(), np.abs(a[:, 0:6] - b[:, 0:6]).max()])
            assert n0[i] == n1[i] and (e < REDO_BARS).all(), (ck, cs['rows'][i], i, e)
    for row, want in need.items():
        sel = cs['rows'] == row
        hit, miss = int((cs['nref'][sel] > 0).sum()), int((cs['nref'][sel] == 0).sum())
        print('chest kind %2d, %-22s in contact %3d, out of contact %3d, worst %s' % (ck, row, hit, miss, per_row.get(row)))
        assert hit >= want, (ck, row, hit, want)
        assert miss >= (30 if ck >= 0 and 'cube' not in row else 0 if 'floor' in row else 15), (ck, row, miss)      # (a puck on the floor is in contact)
    assert set(cs['rows']) == set(need), set(cs['rows']) ^ set(need)
    print('chest kind %d: %d cases, %d dropped on the margin; largest errors (normal, depth, points) %s; handed-in cases with other bits %d'
          % (ck, len(ids), cs['dropped'], worst, differ))
    return worst, differ, per_row


def check_mirror_walls_are_told_apart(ck):
    """the walls that are mirror images of each other (same half extents) get cases that another wall index cannot answer: the
    oracle on the same pose against the other wall gives another count or contacts a millimetre away"""
    cs = redo_pair_cases(ck)
    walls = MODEL['chest'][ck]['walls']
    for w, wall in enumerate(walls):
        for v, other in enumerate(walls):
            if v == w or other['half'] != wall['half']:
                continue
            told = total = 0
            for i in np.nonzero((cs['rows'] == 'gripper base x wall %d' % w) & (cs['nref'] > 0))[0]:
                g = list(cs['geo'][i])
                g[4] = chest_base(ck) + np.array(other['c'])
                alt = _oracle_cyl(g)
                total += 1
                told += int(len(alt) != len(cs['ref'][i]) or np.abs(alt[:, 0:3] - cs['ref'][i][:, 0:3]).max() > 1e-3)
            assert total >= 30 and told == total, (ck, w, v, told, total)


def check_redo_lanes(ck, run, lanes=(64, 37, 16)):
    """a shuffled mix of all rows of one chest kind, fetched and handed-in poses alternating: with 64, 37 and 16 lanes per launch
    every case gives, bit for bit, what it gives in a launch of its own"""
    cs = redo_pair_cases(ck)
    rs = np.random.RandomState(7)
    hit, miss = np.nonzero(cs['nref'] > 0)[0], np.nonzero(cs['nref'] == 0)[0]
    pick = np.concatenate([rs.permutation(hit)[:150], rs.permutation(miss)[:50]])
    pick = pick[rs.permutation(len(pick))]
    assert (cs['nref'][pick] > 0).sum() >= 100 and (cs['nref'][pick] == 0).sum() >= 30 and len(set(cs['rows'][pick])) == len(redo_rows_expected(ck))
    ids = cs['ids'][pick].copy()
    ids[:, 3] = np.arange(len(pick)) % 2
    args = (ck, ids, cs['q9'][pick], cs['blk'][pick], cs['doorq'][pick], cs['kc'])
    n1, o1 = run(*args, lanes=1)
    assert np.array_equal(n1, cs['nref'][pick])
    for ln in lanes:
        n, o = run(*args, lanes=ln)
        assert np.array_equal(n, n1), (ln, np.nonzero(n != n1)[0][:8])
        for t in range(len(pick)):
            k = 10 * int(n[t])
            assert np.array_equal(o[t][:k].view(np.uint32), o1[t][:k].view(np.uint32)), (ln, t, cs['rows'][pick[t]])
    return len(pick)


# ---- the float pass on the shapes of those pairs
def float_shape_pairs():
    """(name, radius, half length, box half extents) of the cylinder x box pairs the float pass meets beyond puck x cube / table"""
    c0, c1 = MODEL['chest']
    out = [('gripper base x cube', GBASE_R, GBASE_HL, CUBE_H),
           ('gripper base x door', GBASE_R, GBASE_HL, np.array(c0['door_half'])),
           ('gripper base x lid', GBASE_R, GBASE_HL, np.array(c1['door_half'])),
           ('gripper base x back wall', GBASE_R, GBASE_HL, np.array(c0['walls'][0]['half'])),
           ('gripper base x side wall', GBASE_R, GBASE_HL, np.array(c0['walls'][1]['half'])),
           ('door handle x finger', c0['handle_radius'], c0['handle_halflen'], FINGER_H),
           ('lid handle x finger', c1['handle_radius'], c1['handle_halflen'], FINGER_H),
           ('puck x finger', PUCK_R, PUCK_HL, FINGER_H)]
    assert c0['walls'][1]['half'] == c0['walls'][2]['half'] == c1['walls'][2]['half'] and c0['walls'][0]['half'] == c1['walls'][0]['half'] == c1['walls'][1]['half']
    return out


@functools.lru_cache(None)
def float_shape_cases():
    """per shape pair 80 walks to the first touch (explicit poses, no arm; every fourth pair axis-aligned, every fourth tilted by
    <= 3 degrees, the rest randomly oriented; the cylinder brought in towards a random point of the box, not only its centre),
    each at first touch and 0.7 mm deeper -> [(name, pair [30])], float32 poses.  The pairs lie within 0.1 m of the origin, as those
    of random_pairs_at_first_touch: 0.65 m out, where the chest stands, the oracle's own float32 mode (world coordinates
    throughout) already strays beyond NP_STRICT from its float64 mode on 3.4 % of these pairs (43 of 1280; here 4), more than
    check_float_shapes may set aside"""
    from test_oracle_physics import _rot_axis
    rs = np.random.RandomState(41)
    out = []
    for name, rad, hl, hb in float_shape_pairs():
        made = 0
        while made < 80:
            if made % 4 == 0:
                Ra, Rb = np.eye(3), np.eye(3)
            elif made % 4 == 1:
                Ra = _rot_axis(rs.normal(size=3), rs.uniform(0, 0.05))
                Rb = _rot_axis(rs.normal(size=3), rs.uniform(0, 0.05)) @ _rot_axis(np.array([0.0, 0.0, 1.0]), rs.uniform(0, 2 * np.pi))
            else:
                Ra, Rb = quat_R64(_rand_quat(rs)), quat_R64(_rand_quat(rs))
            cb, u = rs.uniform(-0.1, 0.1, 3), _unit(rs)
            inside = Rb @ (rs.uniform(-0.9, 0.9, 3) * hb)
            inside -= u * (inside @ u)

            def count(d):
                return len(O.cyl_box(cb + inside + u * d, Ra.ravel(), rad, hl, cb, Rb.ravel(), hb))
            d = _first_touch(count, _support_cyl(Ra, rad, hl, u) + _support_box(Rb, hb, u) + 0.0025)
            if d is None:
                continue
            for extra in (0.0, 0.0007):
                out.append((name, pack_pair(cb + inside + u * (d - extra), Ra.ravel(), [rad, rad, hl], cb, Rb.ravel(), hb)))
            made += 1
    return out


def oracle_shape_pair(pair, f32=False):
    a = [x.astype(float) for x in unpack_pair(pair)]
    return O.cyl_box(a[0], a[1], float(a[2][0]), float(a[2][2]), a[3], a[4], a[5], f32=f32)


def _np_errors(got, ref):
    order_g, order_r = np.lexsort(got[:, :3].round(4).T), np.lexsort(ref[:, :3].round(4).T)
    g, r = got[order_g].astype(float), ref[order_r].astype(float)
    return np.array([np.abs(g[:, 6:9] - r[:, 6:9]).max(), np.abs(g[:, 9] - r[:, 9]).max(), np.abs(g[:, 0:6] - r[:, 0:6]).max()])


def check_float_shapes(run):
    """cyl_box<float> on the float32 poses of the new shape pairs against the float64 oracle on the same float32 poses: the same
    count (one more or less only where check_random_pairs accepts it: every oracle depth short of 2.1 mm), normals, depths and
    points within NP_STRICT.  A pair on which the oracle's OWN float32 mode misses that against its float64 mode is
    ill-conditioned by the reference's measure alone: set aside and counted, at most 1 % of the cases.
    -> (largest errors of the checked pairs, pairs set aside, cases)"""
    cases = float_shape_cases()
    ns, outs, _ = run(NP_CYL, np.stack([p for _, p in cases]))
    worst, aside, per = np.zeros(3), 0, {}
    for i, (name, pair) in enumerate(cases):
        ref, r32 = oracle_shape_pair(pair), oracle_shape_pair(pair, f32=True)
        if len(r32) != len(ref) or (len(ref) and not (_np_errors(r32, ref) < NP_STRICT).all()):
            aside += 1
            continue
        n = int(ns[i])
        hit, checked = per.get(name, (0, 0))
        if n != len(ref):
            assert abs(n - len(ref)) <= 1 and (len(ref) == 0 or np.abs(ref[:, 9]).max() < 0.0021), '%s, case %d: %d contacts, the oracle %d' % (name, i, n, len(ref))
            per[name] = (hit, checked)
            continue
        per[name] = (hit + int(n > 0), checked + 1)
        if n == 0:
            continue
        e = _np_errors(outs[i].reshape(4, 10)[:n], ref)
        assert (e < NP_STRICT).all(), '%s, case %d: normal / depth / points off by %s (bars %s)' % (name, i, e, NP_STRICT)
        worst = np.maximum(worst, e)
    print('float pass on %d cases of %d shape pairs: set aside %d; in contact / checked per pair %s; largest errors %s' % (len(cases), len(per), aside, per, worst))
    assert aside <= 0.01 * len(cases), (aside, len(cases))
    for name, _, _, _ in float_shape_pairs():
        assert per[name][1] >= 150 and per[name][0] >= 100, (name, per[name])
    return worst, aside, len(cases)


# ---- the double arithmetic of the repeat
def double_maths_inputs():
    """squared lengths: exact 0, 4096 log-spaced and 4096 random over 1e-40 .. 1e4, exact squares, powers of two; dividends and
    divisors of both signs over 1e-20 .. 1e4 likewise; angles: every float32 joint angle of the cases above and 4096 random in
    [-3.06, 3.06].  Outside these ranges the routines are not meant to be used"""
    rs = np.random.RandomState(9)
    pw = 2.0 ** np.arange(-130, 14)
    sq = np.concatenate([[0.0], np.logspace(-40, 4, 4096), 10.0 ** rs.uniform(-40, 4, 4096), np.arange(1, 100.0) ** 2, pw[pw >= 1e-40]])
    mag = np.concatenate([np.logspace(-20, 4, 4096), 10.0 ** rs.uniform(-20, 4, 4096), pw[pw >= 1e-20], np.arange(1, 100.0)])
    den = mag * rs.choice([-1.0, 1.0], len(mag))
    num = rs.permutation(mag) * rs.choice([-1.0, 1.0], len(mag))
    ang = [np.stack(fk64_edge_poses())[:, :7].ravel().astype(float), rs.uniform(-3.06, 3.06, 4096)]
    ang += [redo_pair_cases(ck)['q9'][:, :7].ravel().astype(float) for ck in (-1, 0, 1)]
    ang = np.concatenate(ang)
    assert np.abs(ang).max() <= 3.06
    return sq, num, den, ang


def check_sincos64(run):
    """sincos64 against numpy: absolute error < 1e-15 = the kernel polynomials' < 1 ulp of a result <= 1 (1.1e-16 .. 2.2e-16) +
    the two-term reduction's half ulp of |r| <= 0.79 (5.6e-17) + numpy's own ulp (1.1e-16), ~4.5e-16, with margin"""
    ang = double_maths_inputs()[3]
    sn, cs = run(DM_SINCOS, ang, ang)
    err = max(np.abs(sn - np.sin(ang)).max(), np.abs(cs - np.cos(ang)).max())
    print('sincos64: %d angles, largest error %.3g' % (len(ang), err))
    assert len(ang) >= 4096 + 1000 and err < 1e-15, err
    return err


def check_sqrt_div64(run):
    """t_sqrt / t_div against numpy float64: relative error < 1e-15, the figure pmg_contact_body.inc states; t_sqrt(0) = 0"""
    sq, num, den, _ = double_maths_inputs()
    got = run(DM_SQRT, sq, sq)[0]
    assert got[0] == 0.0 and sq[0] == 0.0
    es = np.abs(got[1:] / np.sqrt(sq[1:]) - 1.0).max()
    q = run(DM_DIV, num, den)[0]
    ed = np.abs(q / (num / den) - 1.0).max()
    ulp = 2.0 ** -52
    print('t_sqrt: %d values, largest relative error %.3g (%.2f ulp); t_div: %d quotients, %.3g (%.2f ulp)' % (len(sq), es, es / ulp, len(num), ed, ed / ulp))
    assert len(sq) > 8192 and len(num) > 8192 and es < 1e-15 and ed < 1e-15, (es, ed)
    return es, ed
