"""Cases, models and checks of PMG_IK_LEAN (csrc/pmg_wave.h: affine_shr, half_gram6, half_max; csrc/pmg_device_body.inc: ik_solve and
the scan of fk) -- TEST INFRASTRUCTURE, shared by the emulated tier (tests/test_ik_lean_emulated.py, tests/test_ik_lean_kernels_emulated.py)
and the device tier (tests/test_gpu_ik_lean.py, tests/test_gpu_ik_lean_kernels.py).

The switch takes out moves, fills and one add of zeros; it changes no arithmetic operation and no order.  So
  * each primitive must give the bits of a numpy model that states its tree (below; written from the comments of pmg_wave.h), and
  * a build with the switch on must give the BITS of a build with the switch off: ik_solve, fk, and whole env steps.
Nothing here has a tolerance but the float64 bar of ik_solve, which is tests/device_cases.py's (IK_BAR), as it is.

The two tiers differ in ONE respect, which the models take as `fused`: hipcc contracts `x y + z w` into fma(x, y, fl(z w)), g++ for
plain x86-64 contracts nothing.  The device primitives are that contraction written out; the emulator's branches are the rounded
products, which is what its switch-off build computes."""
import ctypes as C
import os
import subprocess

import numpy as np

import device_cases as D
import oracle_lib as O

NIN, NOUT = 16, 160
SENTINEL = np.float32(-7777.0)
F_AFFINE, F_GRAM, F_MAX = 0, 1, 2


# ----------------------------------------------------------------------------------------------------------------------
# float32 arithmetic, one rounding per operation
def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding.  a b is exact in float64; the float64 sum is made round-to-odd (TwoSum gives its error), and a
    round-to-odd float64 (53 bits >= 2 x 24 + 2) rounds to float32 as the exact value does"""
    a, b, c = [np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c)]
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _mul_add3(fused, x0, y0, x1, y1, x2, y2):
    """`x0 y0 + x1 y1 + x2 y2` as compiled: fused -> fma(x2, y2, fma(x0, y0, fl(x1 y1))); else every product rounded, summed left to right"""
    f = np.float32
    if fused:
        return fma32(x2, y2, fma32(x0, y0, f(x1) * f(y1)))
    return (f(x0) * f(y0) + f(x1) * f(y1)) + f(x2) * f(y2)


def _shr(v, s, fill):
    """lane i <- lane i - s inside its 16-lane row, `fill` where the row has no such lane"""
    out = np.full(64, fill, np.float32)
    for i in range(64):
        if (i & 15) >= s:
            out[i] = v[i - s]
    return out


def affine_shr_model(R, p, s, fused):
    """R [9][64], p [3][64] -> R' [9][64], p' [3][64]"""
    A = [_shr(R[a], s, 1.0 if a % 4 == 0 else 0.0) for a in range(9)]
    a3 = [_shr(p[a], s, 0.0) for a in range(3)]
    Rn = np.zeros((9, 64), np.float32)
    pn = np.zeros((3, 64), np.float32)
    for i in range(3):
        for j in range(3):
            Rn[3 * i + j] = _mul_add3(fused, A[3 * i], R[j], A[3 * i + 1], R[3 + j], A[3 * i + 2], R[6 + j])
        pn[i] = a3[i] + _mul_add3(fused, A[3 * i], p[0], A[3 * i + 1], p[1], A[3 * i + 2], p[2])
    return Rn, pn


def half_gram6_model(x, fused):
    """x [6][64] -> s [21][64]: pairs (i, i ^ 1), then (i, i ^ 2), then the two quads of the half row (i, 7 - i)"""
    lanes = np.arange(64)
    out = np.zeros((21, 64), np.float32)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            prod = x[a] * x[b]
            t = fma32(x[a], x[b], prod[lanes ^ 1]) if fused else prod + prod[lanes ^ 1]
            u = t + t[lanes ^ 2]
            out[k] = u + u[(lanes & ~7) + 7 - (lanes & 7)]
            k += 1
    return out


def half_max_model(v):
    return np.repeat(v.reshape(8, 8).max(1), 8).astype(np.float32)


def prim_inputs():
    """-> [(name, in [NIN][64])]: distinct magnitudes and signs in every lane and slot (a wrong pairing, a wrong order or a fused /
    unfused mix-up changes the bits), exact zeros of both signs, and zeros mixed into the first"""
    rs = np.random.RandomState(77)
    a = (rs.choice([-1.0, 1.0], (NIN, 64)) * rs.uniform(1, 2, (NIN, 64)) * 2.0 ** rs.randint(-6, 7, (NIN, 64))).astype(np.float32)
    z = np.where(rs.randint(0, 2, (NIN, 64)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    m = np.where(rs.randint(0, 3, (NIN, 64)) == 0, z, a).astype(np.float32)
    return [('magnitudes', a), ('zeros of both signs', z), ('zeros among magnitudes', m)]


def run_prim(fn, wr_ns, fam, inp):
    out = np.full((NOUT, 64), SENTINEL, np.float32)
    rc = fn(C.c_int(wr_ns), C.c_int(fam), np.ascontiguousarray(inp, np.float32).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def _bits_equal(got, want, what):
    same = np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)
    assert same.all(), (what, 'first (slot, lane) that differ', np.argwhere(~same)[:6].tolist(), got[~same][:3].tolist(), want[~same][:3].tolist())


def check_primitives(fn, fused, label, out=print):
    """every lane of all four rows, both namespaces, the three inputs: the model's bits"""
    for ns in (0, 1):
        for name, inp in prim_inputs():
            got = run_prim(fn, ns, F_AFFINE, inp)
            for k, s in enumerate((1, 2, 4)):
                Rn, pn = affine_shr_model(inp[0:9], inp[9:12], s, fused)
                _bits_equal(got[12 * k:12 * k + 9], Rn, (label, ns, name, 'affine_shr R', s))
                _bits_equal(got[12 * k + 9:12 * k + 12], pn, (label, ns, name, 'affine_shr p', s))
            assert (got[36:] == SENTINEL).all()
            got = run_prim(fn, ns, F_GRAM, inp)
            _bits_equal(got[:21], half_gram6_model(inp[0:6], fused), (label, ns, name, 'half_gram6'))
            assert (got[21:] == SENTINEL).all()
            v = np.abs(inp[0:1])                      # (fmaxf leaves the sign of max(+0, -0) open: the product calls it on |dq|)
            got = run_prim(fn, ns, F_MAX, np.concatenate([v, inp[1:]]))
            _bits_equal(got[0], half_max_model(v[0]), (label, ns, name, 'half_max'))
            out('%-4s %s %-24s affine_shr<1, 2, 4>, half_gram6, half_max: the model\'s bits in all 64 lanes' % (label, 'wr' if ns else 'wv', name))


# ----------------------------------------------------------------------------------------------------------------------
# ik_solve
def _quat_branch(R):
    """the branch quat_from_R takes on the rotation R [3][3]"""
    m = R.ravel()
    if m[0] + m[4] + m[8] > 0:
        return 'trace'
    if m[0] < m[4]:
        return 'z' if m[4] < m[8] else 'y'
    return 'z' if m[0] < m[8] else 'x'


def branch_starts():
    """-> {branch: q [9]}: for each branch of quat_from_R the first of 400 seeded random poses of the arm whose tip frame takes it"""
    rs = np.random.RandomState(5)
    found = {}
    for _ in range(400):
        q = np.float32(np.r_[rs.uniform(D.JLO[:7], D.JHI[:7]), 0.035, 0.035])
        br = _quat_branch(O.fk_tip(q.astype(float))[1])
        found.setdefault(br, q)
    return found


def ik_cases():
    """-> [(name, q0 [9], target [3])], 32 of them"""
    mid = np.float32(0.5 * (D.EE_LO + D.EE_HI))
    near = np.float32([-0.52, 0.0, 0.25])
    tip = O.fk_tip(D.Q_START.astype(float))[0]
    # targets at the tip and a little off it: reached after 1, 32, 34 and 36 iterations (the oracle's counts) -- one packed wavefront
    out = [('%g off the tip' % d, D.Q_START.copy(), np.float32(tip + np.array([d, -d, d]))) for d in (0.0, 1e-5, 1e-4, 3e-4)]
    out += [('basic %d' % i, q, t) for i, (q, t) in enumerate(D.ik_cases_basic())]
    out += [('out of reach %d' % i, D.Q_START.copy(), np.float32(t)) for i, t in enumerate(([-1.5, 0.0, 0.3], [-0.3, 0.9, 1.2]))]
    corners = [np.float32([x, y, z]) for x in (D.EE_LO[0], D.EE_HI[0]) for y in (D.EE_LO[1], D.EE_HI[1]) for z in (D.EE_LO[2], D.EE_HI[2])]
    out += [('corner %d' % i, D.Q_START.copy(), corners[i]) for i in (0, 3, 5, 6)]         # far targets: the step clamp is active
    zero = np.float32(np.r_[np.zeros(7), 0.035, 0.035])
    out += [('q = 0, %s' % n, zero.copy(), t) for n, t in (('near', near), ('mid', mid), ('corner', corners[5]))]
    for j in range(7):                                                                    # exact-zero Jacobian entries
        q = D.Q_START.copy()
        q[j] = 0
        out.append(('joint %d zero' % j, q, corners[j] if j % 2 else near))
    for br, q in sorted(branch_starts().items()):
        out += [('start on the %s branch, %s' % (br, n), q.copy(), t) for n, t in (('near', near), ('mid', mid))]
    rs = np.random.RandomState(9)
    while len(out) < 32:
        out.append(('box %d' % len(out), D.Q_START.copy(), np.float32(rs.uniform(D.EE_LO, D.EE_HI))))
    return out[:32]


def ik_properties(cases):
    """what the cases must cover, from the float64 oracle: iteration counts on both sides of the limit, four different counts in a
    packed wavefront, every branch of quat_from_R the arm reaches, a clamped first step"""
    its = np.array([O.ik(q.astype(float), t.astype(float))[1] for _, q, t in cases])
    assert (its < 40).any() and (its >= 40).any(), its
    assert any(len(set(its[i:i + 4])) >= 3 for i in range(0, len(cases), 4)), its
    br = branch_starts()
    assert {'trace', 'y'} <= set(br), sorted(br)
    return its, sorted(br)


def run_ik(fn, packed, cases):
    q = np.ascontiguousarray(np.stack([c[1] for c in cases]), np.float32)
    t = np.ascontiguousarray(np.stack([c[2] for c in cases]), np.float32)
    out = np.zeros((len(cases), 9), np.float32)
    rc = fn(C.c_int(packed), C.c_int(len(cases)), q.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def check_ik(fn_on, fn_off, label, out=print):
    cases = ik_cases()
    its, branches = ik_properties(cases)
    out('%s ik_solve: %d cases, oracle iteration counts %s, quat_from_R branches %s' % (label, len(cases), its.tolist(), branches))
    for packed in (0, 1):
        on, off = run_ik(fn_on, packed, cases), run_ik(fn_off, packed, cases)
        same = on.view(np.uint32) == off.view(np.uint32)
        assert same.all(), (label, packed, 'cases that differ', [cases[i][0] for i in np.unique(np.argwhere(~same)[:, 0])],
                            float(np.abs(on.astype(np.float64) - off.astype(np.float64)).max()))
        assert (on[:, :7] != np.stack([c[1] for c in cases])[:, :7]).any(1).all()          # every case moved the arm
        pairs = [(c[1], c[2]) for c in cases]
        err = D.ik_errors(pairs, lambda q, t, on=on: on)
        out('%s ik_solve, %s: switch on = switch off in all %d cases, bit for bit; against the float64 oracle %.3g (bar %.0e, worst: %s)' % (
            label, 'four envs per wavefront' if packed else 'one env per wavefront', len(cases), err.max(), D.IK_BAR, cases[int(err.argmax())][0]))
        assert err.max() < D.IK_BAR, (label, packed, err.max(), cases[int(err.argmax())][0])


# ----------------------------------------------------------------------------------------------------------------------
# fk
def fk_cases():
    """-> q [16][9]: zeros, the start pose, both limits, alternating limits, single zero joints, random poses"""
    rs = np.random.RandomState(13)
    alt = np.where(np.arange(9) % 2 == 0, D.JLO, D.JHI)
    qs = [np.zeros(9), D.Q_START, D.JLO, D.JHI, alt, D.JLO + D.JHI - alt]
    for j in (1, 3, 5):
        q = D.Q_START.astype(float)
        q[j] = 0
        qs.append(q)
    while len(qs) < 16:
        qs.append(rs.uniform(D.JLO, D.JHI))
    return np.ascontiguousarray(np.stack(qs), np.float32)


def run_fk(fn, packed, q):
    out = np.full((len(q), 16, 18), SENTINEL, np.float32)
    rc = fn(C.c_int(packed), C.c_int(len(q)), q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def check_fk(fn_on, fn_off, label, out=print):
    q = fk_cases()
    for packed in (0, 1):
        on, off = run_fk(fn_on, packed, q), run_fk(fn_off, packed, q)
        assert not (on == SENTINEL).any()
        _bits_equal(on, off, (label, packed, 'fk: R, p, S of lanes 0-8, the tip frame in lanes 9-15'))
        for i in range(len(q)):                                                           # ... and it IS the forward kinematics
            p, R = O.fk_tip(q[i].astype(float))
            assert np.abs(on[i, 9:, :9].reshape(-1, 3, 3) - on[i, 6, :9].reshape(3, 3)).max() == 0 and np.abs(on[i, 6, :9].reshape(3, 3) - R).max() < 1e-5, i
        out('%s fk, %s: R, p, S of all sixteen lanes, switch on = switch off in %d poses, bit for bit' % (
            label, 'four envs per wavefront' if packed else 'one env per wavefront', len(q)))


# ----------------------------------------------------------------------------------------------------------------------
# whole env steps
def _step(pmg, library, task, st, act, switches):
    import warnings
    import substep_cases as SC
    keys = ('PMG_REACH_TWO_WAVES', 'PMG_PACKED', 'PMG_ENV_CYCLES')
    saved = {k: os.environ.get(k) for k in keys}
    os.environ.update(dict({'PMG_ENV_CYCLES': '1'}, **switches))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            env, _ = SC._handle_banner(lambda: pmg.make_env(task=task, num_envs=len(act), seed=11, seed_stride=1, max_episode_steps=1000, _library=library))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        env.reset()
        if st is not None:
            env.set_state(st)
        o, r, d, info = env.step(act)
        sch = env.handle.schedule()
        return dict(state=env.get_state(), obs=o['observation'], ag=o['achieved_goal'], dg=o['desired_goal'], reward=r,
                    prone=np.sort(sch['prone']), free=np.sort(sch['free']), redo=np.sort(sch['redo']))
    finally:
        env.close()


def _same(a, b, label):
    for k in ('state', 'obs', 'ag', 'dg', 'reward'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (label, k, np.argwhere(x != y)[:4].tolist())


def reach_scene(high):
    """-> states [8, D]: four pressed envs (both fingers flat on the table) and four hovering ones (the reset state)"""
    import reach_mfma_cases as KC
    import rowsetup_cases as RC
    st = KC.scenes(False)
    hover = st[7].copy()
    st[0:4] = RC.pressed_states()[0]
    st[4:8] = hover
    st[4:8, 18:21] += np.float32([[0.02, 0.0, 0.05], [-0.03, 0.04, 0.1], [0.0, -0.05, 0.02], [0.04, 0.03, 0.0]])     # four tip targets
    st[:, 29] = 0
    if high:
        st[0:4, 20] = np.float32(0.30)
    return st


def kernel_runs(pmg, library):
    """one env step on each kernel that holds ik_solve or fk -> {name: record}"""
    rs = np.random.RandomState(3)
    act8 = np.float32(np.r_[[[0.2, 0.1, -1.0], [-0.3, 0.2, -1.0], [0.1, -0.2, -1.0], [-0.1, -0.1, -1.0]], rs.uniform(-1, 1, (4, 3))])
    zero8 = np.zeros((8, 3), np.float32)
    runs = dict(two=_step(pmg, library, 'reach', reach_scene(False), act8, {'PMG_REACH_TWO_WAVES': '1', 'PMG_PACKED': '1'}),
                one=_step(pmg, library, 'reach', reach_scene(False), act8, {'PMG_REACH_TWO_WAVES': '0', 'PMG_PACKED': '1'}),
                redo=_step(pmg, library, 'reach', reach_scene(True), zero8, {'PMG_PACKED': '1'}),
                packed13=_step(pmg, library, 'reach', None, np.float32(rs.uniform(-1, 1, (13, 3))), {'PMG_PACKED': '1'}),
                push8=_step(pmg, library, 'push', None, np.float32(rs.uniform(-1, 1, (8, 3))), {}))
    four = np.arange(4)
    assert np.array_equal(runs['two']['prone'], four) and np.array_equal(runs['one']['prone'], four), (runs['two']['prone'], runs['one']['prone'])
    assert np.array_equal(runs['two']['free'], four + 4), runs['two']['free']
    assert np.array_equal(runs['redo']['redo'], four), (runs['redo']['redo'], runs['redo']['prone'])
    assert len(runs['packed13']['free']) == 13 and len(runs['packed13']['prone']) == 0, (runs['packed13']['free'], runs['packed13']['prone'])
    return runs


def check_kernels(pmg, lib_on, lib_off, label, out=print):
    on, off = kernel_runs(pmg, lib_on), kernel_runs(pmg, lib_off)
    names = dict(two='pmg_k_step_reach2 (4 pressed) + the packed list (4 hovering)', one='pmg_k_step_reach + the packed list', redo='pmg_k_redo (4 mispredicted)',
                 packed13='the packed reach list, 13 envs', push8='push, 8 envs')
    for k, name in names.items():
        _same(on[k], off[k], '%s: %s, switch on against switch off' % (label, name))
        out('%s %s: states, observations, goals and rewards are the switch-off library\'s, bit for bit' % (label, name))
    _same(on['two'], on['one'], label + ': pmg_k_step_reach2 against pmg_k_step_reach')


_EMU_OFF = {}


def emu_library_switch_off(root, tmp_path_factory):
    """the emulator build of the product sources and the probes with -DPMG_IK_LEAN=0, built once per session -> its path"""
    if 'path' not in _EMU_OFF:
        out = str(tmp_path_factory.mktemp('emu_iklean0') / 'libpmg_emu_iklean0.so')
        emu, src = os.path.join(root, 'tests', 'emu'), os.path.join(root, 'pybullet_multigoal_gym_amd', 'csrc')
        subprocess.check_call(['g++', '-O2', '-fPIC', '-std=c++17', '-I' + emu, '-I' + src, '-Wno-unknown-pragmas', '-w', '-DPMG_IK_LEAN=0',
                               '-shared', '-o', out, os.path.join(emu, 'hip_emu.cpp'), os.path.join(emu, 'pmg_probe.cpp'),
                               os.path.join(src, 'pmg_api.cpp'), '-x', 'c++', os.path.join(src, 'pmg_kernels.hip'), '-lrt'])
        _EMU_OFF['path'] = out
    return _EMU_OFF['path']
