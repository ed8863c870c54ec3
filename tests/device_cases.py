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
    cyl_redo64(blk [n][13], kc [24]) -> n [n], out [n][40]   (the puck, free body 0, against the table)"""
import ctypes as C

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


def check_fk64(run):
    """fk64_link against the float64 oracle's kinematics() through its Bullet-call-level world: link frames of Bullet links
    12 / 13 / 15 at 20 random poses"""
    ora = O.OracleEnv('reach', 1, seed_base=0)
    ora.reset()
    ol = ora.lib
    rs = np.random.RandomState(3)
    qs = [np.float32(np.concatenate([rs.uniform(-2, 2, 7), rs.uniform(0, 0.035, 2)])) for _ in range(20)]
    q9 = np.ascontiguousarray(np.repeat(np.stack(qs), 3, axis=0), np.float32)
    body = np.ascontiguousarray(np.tile([b for b, _ in FK64_BODIES], 20), np.int32)
    p, R = run(q9, body)
    for trial, q in enumerate(qs):
        for d in range(9):
            ol.pmgo_bw_reset_joint(ora.h, 0, d, C.c_double(float(q[d])), C.c_double(0.0))
        for k, (b, link) in enumerate(FK64_BODIES):
            ref = np.zeros(13)
            ol.pmgo_bw_link_state(ora.h, link, _fp(ref))
            i = 3 * trial + k
            assert np.abs(p[i] - ref[:3]).max() < 1e-12, (trial, b, p[i], ref[:3])
            assert np.abs(R[i].reshape(3, 3) - quat_R64(ref[3:7])).max() < 1e-12
    ora.close()


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
