"""Cases, float64 reference and bounds of the reach row set-up at function level (pmg::reach_rowspace_setup<0, 8>,
csrc/pmg_step_body.inc) -- TEST INFRASTRUCTURE, shared by tests/test_rowsetup_emulated.py and tests/test_gpu_rowsetup.py.  The probe
(prim::rowsetup_cases, gpu_probe/pmg_prim_probe.inc) runs the set-up for one env per case and returns, per lane, the coefficient
table c24, the response Rm = M^-1 J^T, the diagonal den and the right-hand side rhs, plus the float32 joint subspaces S and
M^-1 it worked from.

Cases.  Joint poses and velocities are pressed states the float64 oracle produces (reach, the tip driven down for twelve env
steps, four lateral directions); the contact list of each is the oracle's own for that state (both fingers flat on the table:
four corners each), and a case keeps a subset of it: one corner of finger 1 (1 contact), finger 1 flat (4), finger 1 flat and
one corner of finger 2 (5), both flat (8), finger 2 only (4) -- every tile edge of the 24 x 24 table: one row triple, half the
table, one triple past the half, the full table, and a list whose rows all carry the finger-2 column.  One more case tilts the
normals of a five-contact list so that both branches of plane_space and all three directions of a row are generic.

Reference: the same quantities in float64 from the SAME float32 contact list, S and M^-1.

Bounds (u = 2^-24; none of them comes from a run of the code under test).  With A(j, s) = sum_d sum_e |J_j[d]| |M^-1[d][e]| |J_s[e]|:
  Rm_j[d]   32 u sum_e |M^-1[d][e]| |J_j[e]|                                   + sum_e |M^-1[d][e]| dJ_j[e]
  den_j     32 u A(j, j)                                                        + 2 sum_de dJ_j[d] |M^-1[d][e]| |J_j[e]|        =: dden_j
  c(j, s)   32 u A(j, s) / den_j     (the bound the issue states)               + [sum dJ_j |M^-1| |J_s| + sum |J_j| |M^-1| dJ_s] / den_j + |c64| (dden_j / den_j + 4 u)
  rhs_j     [16 u sum_d |J_j[d]| |qd[d]| + sum_d dJ_j[d] |qd[d]| + 4 u (|rel| + |dist| / dt)] / den_j                           + |rhs64| (dden_j / den_j + 4 u)
The second column is the float32 rounding of the inputs themselves: the kernel builds J in float32, J_j[d] = ((w_d x p) + v_d) . dir
-- products, a difference, a sum, a three-term dot product with a direction that plane_space itself derived in float32 (a 2.5-ulp
1 / sqrt, two products): at most 16 roundings deep, dJ_j[d] = 16 u sum_k (|w_d x p|_k + |v_d|_k) |dir_k| with the cross product's
terms taken by absolute value.  32 u covers the nine-term sums of products in either association (pairwise on the VALU, the
(d, d + 4) chain on the matrix pipe: at most 10 roundings each, two products deep) with a factor of 1.6 in hand, so BOTH builds
of the set-up must meet it.  Rows that do not exist are exact zeros."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
import substep_cases as SC

U = 2.0 ** -24
DT, LINEAR_SLOP, CONTACT_ERP, SIMD_EPS = np.float32(0.002), np.float32(1e-5), np.float32(0.9), 1.1920929e-07
BODY_FINGER1, BODY_FINGER2, BODY_STATIC = 5, 6, -1          # the product's contact body ids (csrc/pmg_contact_body.inc)
MU = 0.5
SCENES = ['one corner of finger 1', 'finger 1 flat', 'finger 1 flat and one corner of finger 2', 'both flat', 'finger 2 only',
          'tilted normals, five contacts']


@functools.lru_cache(maxsize=None)
def pressed_states():
    """-> (states [4, D] float32 after twelve env steps of pressing down, per state the oracle's contact list of the next substep:
    (finger index 0 / 1, point [3], distance) in solve order)"""
    n = 4
    ora = O.OracleEnv('reach', n, seed_base=11, seed_stride=1, max_episode_steps=1000)
    ora.reset(), ora.reset()
    act = np.float32([[0.3, 0.2, -1], [-0.3, 0.1, -1], [0.1, -0.4, -1], [-0.2, -0.2, -1]])
    for _ in range(12):
        ora.step(act)
    st = ora.get_state().copy()
    ora.close()
    sub = O.SubstepOracle('reach', n, substeps=1, seed_base=11, seed_stride=1, max_episode_steps=1000)
    sub.reset(), sub.reset()
    sub.set_state(st)
    sub.step(np.zeros((n, 3), np.float32))
    info = sub.last_substep()
    sub.close()
    lists = []
    for i in range(n):
        nc = int(info['nc'][i])
        assert nc == 8 and (info['b'][i, :nc] == SC.STATIC).all(), (i, nc, info['a'][i, :nc], info['b'][i, :nc])
        lists.append([(SC.FINGERS.index(int(info['a'][i, c])), info['point_a'][i, c].copy(), float(info['distance'][i, c])) for c in range(nc)])
        assert sorted(f for f, _, _ in lists[-1]) == [0] * 4 + [1] * 4
    st.setflags(write=False)
    return st, lists


@functools.lru_cache(maxsize=None)
def cases():
    """-> dict(name [n], q, qd [n, 9], con [n, 8, 12], mu [n, 8], nc [n]) float32 / int32: every scene on two of the poses"""
    st, lists = pressed_states()
    names, q, qd, con, mu, ncs = [], [], [], [], [], []
    for k, scene in enumerate(SCENES):
        for pose in (k % 4, (k + 1) % 4):
            full = lists[pose]
            f1, f2 = [c for c in full if c[0] == 0], [c for c in full if c[0] == 1]
            pick = {'one corner of finger 1': f1[pose % 4:pose % 4 + 1], 'finger 1 flat': f1, 'finger 1 flat and one corner of finger 2': f1 + f2[pose % 4:pose % 4 + 1],
                    'both flat': f1 + f2, 'finger 2 only': f2, 'tilted normals, five contacts': f2[:2] + f1[:3]}[scene]
            row = np.zeros((8, 12), np.float32)
            for c, (f, p, dist) in enumerate(pick):
                nrm = np.array([0.0, 0.0, 1.0])
                if scene.startswith('tilted'):
                    nrm = np.array([[0.8, 0.1, 0.59], [-0.2, 0.6, 0.77], [0.05, -0.9, 0.43], [0.3, 0.3, 0.9], [-0.7, 0.2, 0.68]][c])
                    nrm /= np.linalg.norm(nrm)
                row[c] = [BODY_FINGER1 if f == 0 else BODY_FINGER2, BODY_STATIC, *p, *(p - nrm * dist), *nrm, dist]
            names.append('%s, pose %d' % (scene, pose))
            q.append(st[pose, :9]), qd.append(st[pose, 9:18]), con.append(row), mu.append(np.full(8, MU, np.float32)), ncs.append(len(pick))
    out = dict(name=names, q=np.float32(q), qd=np.float32(qd), con=np.float32(con), mu=np.float32(mu), nc=np.int32(ncs))
    assert sorted(set(out['nc'].tolist())) == [1, 4, 5, 8]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def run(fn):
    """fn: pmge_rowsetup / pmgd_rowsetup -> dict(coef [n, 64, 24], resp [n, 64, 9], misc [n, 64, 4], S [n, 9, 6], minv [n, 9, 9])"""
    cs = cases()
    n = len(cs['nc'])
    out = dict(coef=np.full((n, 64, 24), -7777.0, np.float32), resp=np.full((n, 64, 9), -7777.0, np.float32), misc=np.full((n, 64, 4), -7777.0, np.float32),
               S=np.zeros((n, 9, 6), np.float32), minv=np.zeros((n, 9, 9), np.float32))
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    rc = fn(C.c_int(n), p(cs['q']), p(cs['qd']), p(cs['con']), p(cs['mu']), p(cs['nc']), p(out['coef']), p(out['resp']), p(out['misc']), p(out['S']), p(out['minv']))
    assert rc == 0, rc
    return out


def _plane_space(n):
    if abs(n[2]) > 0.7071067811865475244:
        a = n[1] * n[1] + n[2] * n[2]
        k = 1.0 / np.sqrt(a)
        p = np.array([0.0, -n[2] * k, n[1] * k])
        return p, np.array([a * k, -n[0] * p[2], n[0] * p[1]])
    a = n[0] * n[0] + n[1] * n[1]
    k = 1.0 / np.sqrt(a)
    p = np.array([-n[1] * k, n[0] * k, 0.0])
    return p, np.array([-n[2] * p[1], n[2] * p[0], a * k])


def reference(S, minv, con, qd, nc):
    """one case in float64 from the float32 operands -> dict(J, dJ [3 nc, 9], Rm, den, c, rhs and their bounds)"""
    S, M, con, qd = (np.asarray(x, np.float32).astype(np.float64) for x in (S, minv, con, qd))
    nr = 3 * nc
    J, dJ = np.zeros((nr, 9)), np.zeros((nr, 9))
    for c in range(nc):
        own = 7 if int(con[c, 0]) == BODY_FINGER1 else 8
        pt, n = con[c, 2:5], con[c, 8:11]
        t1, t2 = _plane_space(n)
        for t, d in enumerate((n, t1, t2)):
            for j in range(9):
                if j < 7 or j == own:
                    w, v = S[j, :3], S[j, 3:6]
                    J[3 * c + t, j] = (np.cross(w, pt) + v) @ d
                    mag = np.abs([w[1] * pt[2], w[2] * pt[0], w[0] * pt[1]]) + np.abs([w[2] * pt[1], w[0] * pt[2], w[1] * pt[0]]) + np.abs(v)
                    dJ[3 * c + t, j] = 16 * U * (mag @ np.abs(d))
    aJ, aM = np.abs(J), np.abs(M)
    Rm = J @ M.T                                           # Rm[j][d] = sum_e M[d][e] J_j[e]
    bRm = 32 * U * (aJ @ aM.T) + dJ @ aM.T
    A = aJ @ aM @ aJ.T
    den = np.einsum('jd,jd->j', J, Rm)
    dden = 32 * U * np.diag(A) + 2 * np.einsum('jd,de,je->j', dJ, aM, aJ)
    c64 = -(J @ M @ J.T) / den[:, None]                   # c[j][s]
    bc = 32 * U * A / den[:, None] + (dJ @ aM @ aJ.T + aJ @ aM @ dJ.T) / den[:, None] + np.abs(c64) * (dden / den + 4 * U)[:, None]
    rel = J @ qd
    drel = 16 * U * (aJ @ np.abs(qd)) + dJ @ np.abs(qd)
    rhs, brhs = np.zeros(nr), np.zeros(nr)
    for r in range(nr):
        c, t = divmod(r, 3)
        dist = float(np.float32(con[c, 11]) + LINEAR_SLOP)
        if t == 0:
            num = (-rel[r] - dist / float(DT)) if dist > 0 else (-dist * float(CONTACT_ERP) / float(DT) - rel[r])
        else:
            num = -rel[r]
        rhs[r] = num / den[r]
        brhs[r] = (drel[r] + 4 * U * (abs(rel[r]) + abs(dist) / float(DT))) / den[r] + abs(rhs[r]) * (dden[r] / den[r] + 4 * U)
    assert (den > 1e3 * SIMD_EPS).all()
    return dict(J=J, Rm=Rm, bRm=bRm, den=den, dden=dden, c=c64, bc=bc, rhs=rhs, brhs=brhs)


def check(fn, label, out=print, dof_equals_published=False):
    """every case of cases() through the probe `fn`, against the float64 reference; -> the probe's output"""
    cs, got = cases(), None
    got = run(fn)
    worst = {'c': 0.0, 'Rm': 0.0, 'den': 0.0, 'rhs': 0.0, 'dof': 0.0}
    for i, name in enumerate(cs['name']):
        nc = int(cs['nc'][i])
        nr = 3 * nc
        ref = reference(got['S'][i], got['minv'][i], cs['con'][i], cs['qd'][i], nc)
        coef, resp, misc = (got[k][i].astype(np.float64) for k in ('coef', 'resp', 'misc'))
        rows = np.arange(16, 16 + nr)
        # the rows that exist
        off = ~np.eye(nr, dtype=bool)
        ratio = lambda err, bound: float((err / bound).max()) if err.size else 0.0
        rc = ratio(np.abs(coef[rows, :nr] - ref['c'])[off], ref['bc'][off]) if nr > 1 else 0.0
        rR = ratio(np.abs(resp[rows] - ref['Rm']), np.maximum(ref['bRm'], 1e-300))
        rd = ratio(np.abs(misc[rows, 0] - ref['den']), ref['dden'] + 4 * U * ref['den'])
        rr = ratio(np.abs(misc[rows, 1] - ref['rhs']), ref['brhs'])
        # the DoF lanes' coefficients: (M^-1 J_s^T)_l
        rl = ratio(np.abs(coef[:9, :nr].T - ref['Rm']), np.maximum(ref['bRm'], 1e-300))
        for k, v in zip(('c', 'Rm', 'den', 'rhs', 'dof'), (rc, rR, rd, rr, rl)):
            worst[k] = max(worst[k], v)
        out('%-10s %-52s nc %d  error / bound: c %.3f  Rm %.3f  den %.3f  rhs %.3f  DoF lanes %.3f' % (label, name, nc, rc, rR, rd, rr, rl))
        assert max(rc, rR, rd, rr, rl) <= 1.0, (label, name, dict(c=rc, Rm=rR, den=rd, rhs=rr, dof=rl))
        assert (coef[rows, :nr][~off] == 0).all(), (label, name, 'a row lane keeps no coefficient for its own row')
        assert np.array_equal(got['misc'][i][rows, 3], np.full(nr, MU, np.float32)) and (misc[rows, 2] > 0).all()
        # rows that do not exist: exact zeros -- the missing sources of every lane, and everything in the lanes without a row
        assert (coef[:, nr:] == 0).all(), (label, name, 'coefficients of source rows that do not exist', np.argwhere(coef[:, nr:] != 0)[:4].tolist())
        idle = np.concatenate([np.arange(9, 16), np.arange(16 + nr, 64)])
        assert (coef[idle] == 0).all() and (misc[idle] == 0).all(), (label, name, 'lanes without a DoF or a row')
        assert (resp[np.arange(16 + nr, 40)] == 0).all(), (label, name, 'responses of rows that do not exist')
        if dof_equals_published:
            # the matrix-pipe build: a DoF lane's coefficient for source s IS entry l of the response row lane 16 + s publishes
            a, b = got['coef'][i][:9, :nr].T, got['resp'][i][rows]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, name, np.argwhere(a != b)[:4].tolist())
    out('%-10s worst error / bound over %d cases: %s' % (label, len(cs['name']), ', '.join('%s %.3f' % kv for kv in worst.items())))
    return got
