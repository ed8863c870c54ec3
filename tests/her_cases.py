"""The cases of the HER-sampler tests (include/pmg.h pmg_her_sample_device, pmg_device_copy) and their numpy
model, shared by three files: tests/test_her_emulated.py runs them on the g++ build of the product sources over the fiber
emulator, tests/test_gpu_her.py on libpmg_hip.so on the MI355X, tests/test_her_host.py covers env.her and the model's
statistics.  Every case takes the loaded library and goes through the C ABI with buffers from pmg_device_alloc.

Fixtures.  Every element of a row table / an action table holds an integer code of (e, t, column) below 2^24 (exact in
float32), so a value read from a wrong source shows in the value itself; cases that need distances or clips overwrite
the columns concerned.  Bars.  Draws, raw rows and normalised rows are integer arithmetic / bit copies / IEEE float32
operations in a stated order: bit-equal.  Rewards: the band of tests/test_gpu_reward_edges.py, a relative (G / 2 + 4) 2^-24
around the threshold (the float32 distance's error bound); the fixtures hold no pair inside it."""
import ctypes as C

import numpy as np

import normalizer_cases as NC
import pybullet_multigoal_gym_amd as pmg
from normalizer_cases import GOAL, OBS, POL, SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PMG_BUF_PACKED, PmgHerBatch, PmgHerSource

TASK_NAMES = NC.TASK_NAMES
E_INVALID = -1
OUTPUTS = ('x', 'x_next', 'action', 'reward', 'goal_achieved', 'index')
CANARY_BYTES = 64
POISON = np.float32(7e4)          # padding between rows: anything read from it shows
SEEDS = ((0, 0), (12345, 7), (2 ** 63 + 5, 2 ** 64 - 1))
PINNED = {'seed': 3, 'counter': 5, 'E': 1000, 'T': 50, 'future_p': 0.8,
          'e': (46, 824, 774, 462), 't': (42, 7, 36, 35), 'relabelled': (False, True, True, True), 'f': (44, 25, 49, 40)}


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model of the draws (the normative specification of include/pmg.h)
U = np.uint64
GOLD = U(0x9E3779B97F4A7C15)


def mix(z):
    """SplitMix64's finaliser on a uint64 array (arithmetic modulo 2^64)."""
    z = np.asarray(z, U)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def draws(seed, counter, B, E, T, future_p=0.8):
    """-> index [B, 3] int32 = e, t, f (f = -1 where the goal is not relabelled)"""
    seed, counter = np.array([seed % 2 ** 64], U), np.array([counter % 2 ** 64], U)
    key = mix(seed ^ mix(counter + GOLD))
    b = np.arange(B, dtype=U)
    r = [mix(key + (U(4) * b + U(k + 1)) * GOLD) >> U(32) for k in range(4)]
    e = (r[0] * U(E)) >> U(32)
    t = (r[1] * U(T)) >> U(32)
    rel = r[2].astype(np.float64) < float(np.float32(future_p)) * 4294967296.0
    f = t + U(1) + ((r[3] * (U(T) - t)) >> U(32))
    return np.stack([e.astype(np.int64), t.astype(np.int64), np.where(rel, f.astype(np.int64), -1)], 1).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# fixtures and the numpy model of the outputs
def offsets(d, kind):
    """-> first column of the state kind, of the achieved and of the desired goal in a packed row; Ds, G"""
    so = 0 if kind == OBS else d.observation_dim
    ago = d.observation_dim + d.policy_state_dim
    return so, ago, ago + d.goal_dim, (d.observation_dim if kind == OBS else d.policy_state_dim), d.goal_dim


def coded_tables(d, E, T):
    """rows [T + 1, E, P], actions [T, E, A] (time-major), every element an integer code of its (e, t, column)"""
    P, A = d.packed_dim, d.action_dim
    t, e = np.arange(T + 1)[:, None, None], np.arange(E)[None, :, None]
    rows = (e * (T + 1) + t) * P + np.arange(P)[None, None, :] + 1
    acts = -((e * T + t[:T]) * A + np.arange(A)[None, None, :] + 1)
    assert rows.max() < 2 ** 24 and -acts.min() < 2 ** 24
    return rows.astype(np.float32), acts.astype(np.float32)


def gather(d, kind, rows, acts, index):
    """numpy indexing with given indices -> x, x_next [B, Ds + G], action [B, A], achieved_goal(e, t + 1), g' [B, G]"""
    so, ago, dgo, Ds, G = offsets(d, kind)
    e, t, f = index[:, 0], index[:, 1], index[:, 2]
    rel = f >= 0
    g = np.where(rel[:, None], rows[np.where(rel, f, 0), e, ago:ago + G], rows[t, e, dgo:dgo + G])
    x = np.concatenate([rows[t, e, so:so + Ds], g], 1)
    xn = np.concatenate([rows[t + 1, e, so:so + Ds], g], 1)
    return x, xn, acts[t, e], rows[t + 1, e, ago:ago + G], g


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


class Table:
    """A row table and an action table on the device, in one of the layouts of the ABI; freed with `dev`."""

    def __init__(self, h, dev, rows, acts, layout='time', pad=False, in_shift=0):
        T1, E, P = rows.shape
        A = acts.shape[2]
        Pp, Ap = (P + 5, A + 3) if pad else (P, A)

        def put(a, wp):
            buf = np.full(a.shape[:2] + (wp,), POISON, np.float32)
            buf[..., :a.shape[2]] = a
            buf = buf if layout == 'time' else np.ascontiguousarray(buf.transpose(1, 0, 2))
            p = dev.alloc(buf.nbytes + 16)
            h.upload(p + 4 * in_shift, buf)
            return p + 4 * in_shift, buf.nbytes
        (self.d_rows, self.rows_bytes), (self.d_acts, self.acts_bytes) = put(rows, Pp), put(acts, Ap)
        self.E, self.T = E, T1 - 1
        self.es, self.ts = (Pp, E * Pp) if layout == 'time' else (T1 * Pp, Pp)
        self.aes, self.ats = (Ap, E * Ap) if layout == 'time' else ((T1 - 1) * Ap, Ap)
        self.rows, self.acts = rows, acts


def out_specs(h, kind, B):
    d = h.dims
    W = h.norm_width(kind) + d.goal_dim
    return {'x': (np.float32, (B, W)), 'x_next': (np.float32, (B, W)), 'action': (np.float32, (B, d.action_dim)),
            'reward': (np.float32, (B,)), 'goal_achieved': (np.uint8, (B,)), 'index': (np.int32, (B, 3))}


def sample(h, tab, B, kind=POL, raw=True, future_p=0.8, seed=0, counter=0, shift=0, shifts=None, null=(), only=None, rc=0):
    """pmg_her_sample_device from `tab` into canary-framed buffers -> dict(name -> array, or None for a NULL output).
    shift: every output moved off its 16-byte boundary by that many floats (the flags by that many bytes); shifts: the same
    per output; null / only: the outputs passed as NULL / the only ones passed.  The CANARY_BYTES in front of and behind every
    output, and the whole buffer of a NULL output, must come back untouched."""
    specs = out_specs(h, kind, B)
    null = set(null) if only is None else set(OUTPUTS) - set(only)
    shifts = dict({n: shift for n in OUTPUTS}, **(shifts or {}))
    with Dev(h) as dev:
        bufs = {}
        for name, (dt, shape) in specs.items():
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            off = CANARY_BYTES + shifts[name] * (1 if name == 'goal_achieved' else 4)
            base = dev.put(np.full(off + nbytes + CANARY_BYTES, SENTINEL, np.uint8))
            bufs[name] = (base, off, nbytes)
        ptr = {n: (None if n in null else bufs[n][0] + bufs[n][1]) for n in OUTPUTS}
        src, out = h.her_structs(tab.d_rows, tab.E, tab.T, tab.es, tab.ts, B, tab.d_acts, tab.aes, tab.ats, state_kind=kind, raw=raw,
                                 future_p=future_p, seed=seed, counter=counter, d_x=ptr['x'], d_x_next=ptr['x_next'], d_action=ptr['action'],
                                 d_reward=ptr['reward'], d_goal_achieved=ptr['goal_achieved'], d_index=ptr['index'])
        got = h.L.lib.pmg_her_sample_device(h.h, C.byref(src), C.byref(out))
        assert got == rc, (got, h.L.error(h.h))
        res = {}
        for name, (dt, shape) in specs.items():
            base, off, nbytes = bufs[name]
            rawb = dev.get(base, off + nbytes + CANARY_BYTES, np.uint8)
            assert (rawb[:off] == SENTINEL).all() and (rawb[off + nbytes:] == SENTINEL).all(), 'bytes around %s were written' % name
            if name in null or rc != 0:
                assert (rawb == SENTINEL).all(), '%s was written although it was NULL or the call was refused' % name
                res[name] = None
            else:
                res[name] = rawb[off:off + nbytes].copy().view(dt).reshape(shape)
    return res


def check_raw(h, tab, kind, got, index=None, label=''):
    """raw outputs against numpy indexing with the model's (or the given) indices"""
    x, xn, act, _, _ = gather(h.dims, kind, tab.rows, tab.acts, got['index'] if index is None else index)
    for name, want in (('x', x), ('x_next', xn), ('action', act)):
        if got[name] is not None:
            assert np.array_equal(bits(got[name]), bits(want)), (label, name, np.argwhere(got[name] != want)[:4])


def check_ranges(index, E, T):
    e, t, f = index[:, 0].astype(np.int64), index[:, 1].astype(np.int64), index[:, 2].astype(np.int64)
    assert ((0 <= e) & (e < E)).all() and ((0 <= t) & (t < T)).all()
    assert ((f == -1) | ((t < f) & (f <= T))).all()


# ----------------------------------------------------------------------------------------------------------------------
# 1. draws
def test_model_pinned_vector():
    p = PINNED
    ix = draws(p['seed'], p['counter'], 4, p['E'], p['T'], p['future_p'])
    assert tuple(ix[:, 0]) == p['e'] and tuple(ix[:, 1]) == p['t']
    assert tuple(ix[:, 2] >= 0) == p['relabelled']
    full = draws(p['seed'], p['counter'], 4, p['E'], p['T'], 1.0)
    assert tuple(full[:, 2]) == p['f'] and tuple(ix[1:, 2]) == p['f'][1:]


def case_draws(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for E, T in ((1, 1), (2, 1), (1, 2), (64, 50), (1000, 50)):
            rows, acts = coded_tables(h.dims, E, T)
            with Dev(h) as dev:
                tab = Table(h, dev, rows, acts)
                for B in (1, 63, 64, 65, 257, 4097):
                    for seed, counter in SEEDS:
                        got = sample(h, tab, B, seed=seed, counter=counter, only=('index',))['index']
                        want = draws(seed, counter, B, E, T)
                        assert np.array_equal(got, want), (E, T, B, seed, counter, np.argwhere(got != want)[:4])
                        check_ranges(got, E, T)
                        if T == 1:
                            assert (got[:, 1] == 0).all() and np.isin(got[:, 2], (-1, 1)).all()
                # future_p = 0 relabels nothing (the goal is desired_goal(e, t)), future_p = 1 everything
                for p in (0.0, 1.0):
                    got = sample(h, tab, 257, future_p=p, seed=9, counter=1)
                    assert np.array_equal(got['index'], draws(9, 1, 257, E, T, p))
                    assert ((got['index'][:, 2] == -1) if p == 0.0 else (got['index'][:, 2] > got['index'][:, 1])).all()
                    check_raw(h, tab, POL, got, label='future_p %g' % p)
                    if p == 0.0:
                        e, t = got['index'][:, 0], got['index'][:, 1]
                        assert np.array_equal(got['x'][:, 3:], rows[t, e, 9:12]) and np.array_equal(got['x_next'][:, 3:], rows[t, e, 9:12])
                if (E, T) == (PINNED['E'], PINNED['T']):
                    p = PINNED
                    ix = sample(h, tab, 4, future_p=p['future_p'], seed=p['seed'], counter=p['counter'], only=('index',))['index']
                    assert tuple(ix[:, 0]) == p['e'] and tuple(ix[:, 1]) == p['t'] and tuple(ix[:, 2] >= 0) == p['relabelled']
                    assert tuple(ix[1:, 2]) == p['f'][1:]
                    ix = sample(h, tab, 4, future_p=1.0, seed=p['seed'], counter=p['counter'], only=('index',))['index']
                    assert tuple(ix[:, 2]) == p['f']


# 2. raw gather
def case_raw_gather(library, task):
    with handle(library, task, num_envs=8) as env:
        h = env.handle
        rows, acts = coded_tables(h.dims, 5, 7)
        for layout in ('time', 'episode'):
            for pad in (False, True):
                with Dev(h) as dev:
                    tab = Table(h, dev, rows, acts, layout, pad)
                    for kind in (OBS, POL):
                        got = sample(h, tab, 257, kind=kind, seed=4, counter=2)
                        assert np.array_equal(got['index'], draws(4, 2, 257, 5, 7))
                        check_raw(h, tab, kind, got, label=(task, layout, pad, kind))
                        assert (got['index'][:, 2] >= 0).any() and (got['index'][:, 2] < 0).any()


# 3. normalised rows
def clip_tables(h, E, T, seed):
    """coded tables whose state and goal columns hold normalizer_cases.input_rows: values beyond both clips"""
    d = h.dims
    rows, acts = coded_tables(d, E, T)
    n = d.packed_dim - 3
    rows[:, :, :n] = NC.input_rows(seed, (T + 1) * E, n).reshape(T + 1, E, n)
    return rows, acts


def case_normalised_rows(library, task):
    with handle(library, task, num_envs=8) as env:
        h = env.handle
        NC.prime(h)
        rows, acts = clip_tables(h, 6, 9, 21)
        with Dev(h) as dev:
            tab = Table(h, dev, rows, acts)
            for kind in (OBS, POL):
                Ds = h.norm_width(kind)
                got = sample(h, tab, 513, kind=kind, raw=False, seed=8, counter=3)
                assert np.array_equal(got['index'], draws(8, 3, 513, 6, 9))
                x, xn, act, _, _ = gather(h.dims, kind, rows, acts, got['index'])
                assert np.array_equal(bits(got['action']), bits(act))
                for name, src in (('x', x), ('x_next', xn)):
                    want = NC.policy_model(h, kind, src[:, :Ds], src[:, Ds:])
                    assert (np.abs(src) > NC.CLIP_IN).any() and (np.abs(want) == NC.CLIP_OUT).any()
                    assert np.array_equal(bits(got[name]), bits(want)), (task, kind, name, np.argwhere(got[name] != want)[:4])
                    own = NC.device_policy_input(h, kind, np.ascontiguousarray(src[:, :Ds]), np.ascontiguousarray(src[:, Ds:]))
                    assert np.array_equal(bits(got[name]), bits(own)), (task, kind, name, 'pmg_policy_input_device')


# 4. reward and flag
def band(G):
    return (G / 2.0 + 4.0) * 2.0 ** -24


def walk_tables(d, E, T, thr, seed):
    """coded tables whose goal columns are random walks: the achieved goal moves thr / sqrt(8 G) per step and column, so
    a relabelled pair is achieved when f is within about 8 steps of t + 1; the desired goal sits near the walk's end"""
    rows, acts = coded_tables(d, E, T)
    G, ago = d.goal_dim, d.observation_dim + d.policy_state_dim
    rs = np.random.RandomState(seed)
    ag = np.cumsum(rs.normal(0, thr / np.sqrt(8 * G), (T + 1, E, G)), 0)
    rows[:, :, ago:ago + G] = ag
    rows[:, :, ago + G:ago + 2 * G] = ag[-1][None] + rs.normal(0, thr / np.sqrt(4 * G), (T + 1, E, G))
    return rows, acts


def all_pair_distances(d, rows):
    """float64 distance of every pair the sampler can form: (achieved(e, t + 1), achieved(e, f)), t < f <= T, and
    (achieved(e, t + 1), desired(e, t))"""
    G, ago = d.goal_dim, d.observation_dim + d.policy_state_dim
    ag = rows[:, :, ago:ago + G].astype(np.float64)
    dg = rows[:, :, ago + G:ago + 2 * G].astype(np.float64)
    T = rows.shape[0] - 1
    out = [np.linalg.norm(ag[1:] - dg[:-1], axis=2).ravel()]
    for t in range(T):
        out.append(np.linalg.norm(ag[t + 1][None] - ag[t + 1:], axis=2).ravel())
    return np.concatenate(out)


def case_reward_and_flag(library, task):
    for binary, thr in ((True, 0.05), (False, 0.05), (True, 0.08)):
        with handle(library, task, num_envs=8, binary_reward=binary, distance_threshold=thr) as env:
            h, d = env.handle, env.handle.dims
            G = d.goal_dim
            thr32 = float(np.float32(thr))                           # the threshold as the library holds it
            rows, acts = walk_tables(d, 64, 50, thr32, 31)
            dall = all_pair_distances(d, rows)
            assert not (np.abs(dall / thr32 - 1.0) <= band(G)).any(), 'the fixture holds a pair inside the band: pick another seed'
            B = 4097
            index = draws(6, 11, B, 64, 50)
            _, _, _, ag1, g = gather(d, POL, rows, acts, index)
            dist = np.linalg.norm(ag1.astype(np.float64) - g.astype(np.float64), axis=1)
            na = dist > thr32
            assert na.mean() >= 0.1 and (~na).mean() >= 0.1, na.mean()
            with Dev(h) as dev:
                tab = Table(h, dev, rows, acts)
                got = sample(h, tab, B, seed=6, counter=11)
            assert np.array_equal(got['index'], index)
            r, ok = got['reward'], got['goal_achieved']
            print('%s binary=%d thr=%g: achieved %.3f of %d samples' % (task, binary, thr, (~na).mean(), B))
            assert set(np.unique(ok)) <= {0, 1} and np.array_equal(ok, (~na).astype(np.uint8))
            same = (index[:, 2] == index[:, 1] + 1)
            assert same.any() and (dist[same] == 0).all() and (ok[same] == 1).all()
            if binary:
                assert np.array_equal(r, -(na.astype(np.float32))) and np.signbit(r).all()      # -0.0 or -1.0
                assert (r[same] == 0).all() and np.signbit(r[same]).all()
            else:
                assert (np.abs(r.astype(np.float64) + dist) <= band(G) * dist + 1e-45).all(), np.abs(r + dist).max()
                assert (r[same] == 0).all()


def case_reward_is_the_reward_kernels(library, task):
    """The sampler's reward and flag against pmg_compute_reward_device on the pairs it formed, bit for bit, dense and binary:
    achieved_goal(e, t + 1) and g' gathered on the host from the sampler's own index and uploaded four bytes behind a 16-byte
    boundary, so that pmg_k_reward -- the kernel whose sum pmg_k_her_draw shares -- serves every item (the aligned kernels
    sum in another shape).  B = 257: one workgroup and one item more."""
    E, T, B = 7, 5, 257
    for binary in (False, True):
        with handle(library, task, num_envs=8, binary_reward=binary, distance_threshold=0.05) as env:
            h, d = env.handle, env.handle.dims
            rows, acts = walk_tables(d, E, T, 3 * float(np.float32(0.05)), 37)
            with Dev(h) as dev:
                got = sample(h, Table(h, dev, rows, acts), B, seed=10, counter=4)
                _, _, _, ag1, g = gather(d, POL, rows, acts, got['index'])
                d_ag, d_g = dev.alloc(ag1.nbytes + 32), dev.alloc(g.nbytes + 32)
                d_ag, d_g = d_ag + (-d_ag) % 16 + 4, d_g + (-d_g) % 16 + 4
                h.upload(d_ag, ag1)
                h.upload(d_g, g)
                d_r, d_ok = dev.alloc(4 * B), dev.alloc(B)
                rc = h.L.lib.pmg_compute_reward_device(h.h, C.c_void_p(d_ag), C.c_void_p(d_g), C.c_int64(B), C.c_void_p(d_r), C.c_void_p(d_ok))
                assert rc == 0, h.L.error(h.h)
                r, ok = dev.get(d_r, B, np.float32), dev.get(d_ok, B, np.uint8)
            assert set(np.unique(ok)) == {0, 1}, 'the fixture holds achieved and missed pairs'
            assert np.array_equal(bits(got['reward']), bits(r)), (task, binary, np.argwhere(bits(got['reward']) != bits(r))[:4])
            assert np.array_equal(got['goal_achieved'], ok), (task, binary, np.argwhere(got['goal_achieved'] != ok)[:4])


# 5. edges of the sweep
def case_sweep_edges(library):
    """block_stack observation rows, the widest W = 88 + 15: outputs off their 16-byte boundary by 4, 8 and 12 bytes, inputs by 4,
    each output NULL in turn, x and x_next on different boundaries (two launches instead of one), and B around the hand-overs:
    one workgroup / two, and 4 * 2048 * 256 / W rows, from where the grid strides"""
    with handle(library, 'block_stack', num_envs=8) as env:
        h = env.handle
        NC.prime(h)
        W = h.norm_width(OBS) + h.dims.goal_dim
        assert W == 103
        stride_from = 4 * 2048 * 256 // W
        rows, acts = clip_tables(h, 7, 5, 23)
        with Dev(h) as dev:
            tab = Table(h, dev, rows, acts, in_shift=1)
            k = 0
            for B in (1, 255, 256, 257, stride_from - 1, stride_from, stride_from + 1):
                index = draws(2, B, B, 7, 5)
                x, xn, _, _, _ = gather(h.dims, OBS, rows, acts, index)
                for shift in ((1, 2, 3) if B < 1000 else (1 + k % 3,)):
                    k += 1
                    for raw in (True, False):
                        got = sample(h, tab, B, kind=OBS, raw=raw, seed=2, counter=B, shift=shift)
                        assert np.array_equal(got['index'], index)
                        if raw:
                            check_raw(h, tab, OBS, got, label=(B, shift))
                        else:
                            assert np.array_equal(bits(got['x']), bits(NC.policy_model(h, OBS, x[:, :88], x[:, 88:]))), (B, shift)
                            assert np.array_equal(bits(got['x_next']), bits(NC.policy_model(h, OBS, xn[:, :88], xn[:, 88:]))), (B, shift)
            # x and x_next on different 16-byte phases; every output NULL in turn
            B = 257
            full = sample(h, tab, B, kind=OBS, seed=5, counter=5)
            check_raw(h, tab, OBS, full)
            split = sample(h, tab, B, kind=OBS, seed=5, counter=5, shifts={'x': 1, 'x_next': 3, 'index': 2})
            for name in OUTPUTS:
                assert np.array_equal(bits(split[name]), bits(full[name])), name
            for name in OUTPUTS:
                got = sample(h, tab, B, kind=OBS, seed=5, counter=5, shift=1, null=(name,))
                for other in OUTPUTS:
                    if other != name:
                        assert np.array_equal(bits(got[other]), bits(full[other])), (name, other)
            got = sample(h, tab, B, kind=OBS, seed=5, counter=5, only=('x_next',))      # indices in the handle's scratch
            assert np.array_equal(bits(got['x_next']), bits(full['x_next']))
            got = sample(h, tab, 2 * B, kind=OBS, seed=5, counter=5, only=('x',))       # ... which grows
            assert np.array_equal(bits(got['x'][:B]), bits(full['x']))


# 6. determinism and independence
def case_determinism(library):
    with handle(library, 'push', num_envs=8) as env:
        h = env.handle
        NC.prime(h)
        rows, acts = coded_tables(h.dims, 64, 50)
        with Dev(h) as dev:
            tab = Table(h, dev, rows, acts)
            a, b = sample(h, tab, 4097, seed=1, counter=2), sample(h, tab, 4097, seed=1, counter=2)
            small = sample(h, tab, 64, seed=1, counter=2)
            for name in OUTPUTS:
                assert np.array_equal(bits(a[name]), bits(b[name])), name
                assert np.array_equal(bits(a[name][:64]), bits(small[name])), name
            other = sample(h, tab, 4097, seed=1, counter=3, only=('index',))['index']
            assert (other != a['index']).any(1).mean() > 0.9
            for kind in (OBS, POL):
                for raw in (True, False):
                    got = sample(h, tab, 4097, kind=kind, raw=raw, seed=1, counter=2)
                    assert np.array_equal(got['index'], a['index']) and np.array_equal(bits(got['reward']), bits(a['reward']))


# 7. the handle is untouched
def case_handle_untouched(library):
    with handle(library, 'push', num_envs=8) as env:
        h = env.handle
        NC.prime(h)
        env.reset()
        env.step(np.random.RandomState(0).uniform(-1, 1, (8, 3)).astype(np.float32))
        rows, acts = coded_tables(h.dims, 16, 10)

        def snapshot(dev, tab):
            packed = dev.get(h.device_ptr(PMG_BUF_PACKED), (8, h.dims.packed_dim), np.uint32)
            derived = [np.concatenate([v for k, v in sorted(h.norm_read(w).items()) if k in ('mean', 'std', 'inv_std')]) for w in NC.KINDS]
            return (NC.all_totals(h) + derived + [packed, h.get_state(), h.get_rng(), dev.get(tab.d_rows, tab.rows_bytes, np.uint8),
                                                  dev.get(tab.d_acts, tab.acts_bytes, np.uint8)])
        with Dev(h) as dev:
            tab = Table(h, dev, rows, acts, pad=True)
            before = snapshot(dev, tab)
            for raw in (True, False):
                sample(h, tab, 1025, kind=OBS, raw=raw, seed=3, counter=4)
                sample(h, tab, 1025, kind=POL, raw=raw, seed=3, counter=4, only=('x', 'x_next'))
            after = snapshot(dev, tab)
        for a, b in zip(before, after):
            assert np.array_equal(bits(a) if a.dtype.itemsize == 4 else a.view(np.uint8), bits(b) if b.dtype.itemsize == 4 else b.view(np.uint8))


# 8. with the env
def case_with_the_env(library, overlap=False):
    """push x 8, episodes of 3 steps, two episodes: rows and actions recorded on the device with pmg_device_copy into a
    time-major table [T + 1, 2 N, P] (episode ep of env n = table episode ep * N + n), host copies from pmg_read_outputs"""
    N, T = 8, 3
    env = pmg.make_env(task='push', num_envs=N, seed=5, seed_stride=1, max_episode_steps=T, _library=library)
    h, d = env.handle, env.handle.dims
    P, A = d.packed_dim, d.action_dim
    if overlap:
        h.comm_overlap(True)
    NC.prime(h)
    rs = np.random.RandomState(13)
    rows, acts = np.zeros((T + 1, 2 * N, P), np.float32), np.zeros((T, 2 * N, A), np.float32)

    def host_rows():
        o, p, ag, dg, r, ok, dn = h.read_outputs()
        return np.concatenate([o, p, ag, dg, r[:, None], ok[:, None].astype(np.float32), dn[:, None].astype(np.float32)], 1)
    with Dev(h) as dev:
        d_rows, d_acts, d_act = dev.alloc(rows.nbytes), dev.alloc(acts.nbytes), dev.alloc(4 * N * A)
        seen = set()
        for ep in range(2):
            env.reset()
            for t in range(T + 1):
                if t:
                    a = rs.uniform(-1, 1, (N, A)).astype(np.float32)
                    h.upload(d_act, a)
                    h.step_device(d_act)
                    h.device_copy(d_acts + 4 * ((t - 1) * 2 * N + ep * N) * A, d_act, 4 * N * A)
                    acts[t - 1, ep * N:(ep + 1) * N] = a
                seen.add(h.device_ptr(PMG_BUF_PACKED))
                h.device_copy(d_rows + 4 * (t * 2 * N + ep * N) * P, h.device_ptr(PMG_BUF_PACKED), 4 * N * P)
                rows[t, ep * N:(ep + 1) * N] = host_rows()
        assert len(seen) == (2 if overlap else 1)                    # with the overlap on the row buffer alternates
        assert np.array_equal(bits(dev.get(d_rows, rows.shape, np.float32)), bits(rows))
        assert np.array_equal(bits(dev.get(d_acts, acts.shape, np.float32)), bits(acts))
        assert (rows[T, :, P - 1] == 1).all() and (rows[1:T, :, P - 1] == 0).all()     # done exactly at the TimeLimit
        tab = Table.__new__(Table)
        tab.d_rows, tab.d_acts, tab.E, tab.T, tab.es, tab.ts, tab.aes, tab.ats = d_rows, d_acts, 2 * N, T, P, 2 * N * P, A, 2 * N * A
        tab.rows, tab.acts = rows, acts
        B = 257
        index = draws(7, 1, B, 2 * N, T)
        for kind in (OBS, POL):
            got = sample(h, tab, B, kind=kind, seed=7, counter=1)
            assert np.array_equal(got['index'], index)
            check_raw(h, tab, kind, got, label='env rows')
            x, xn, _, ag1, g = gather(d, kind, rows, acts, index)
            Ds = h.norm_width(kind)
            got = sample(h, tab, B, kind=kind, raw=False, seed=7, counter=1)
            assert np.array_equal(bits(got['x']), bits(NC.policy_model(h, kind, x[:, :Ds], x[:, Ds:])))
            assert np.array_equal(bits(got['x_next']), bits(NC.policy_model(h, kind, xn[:, :Ds], xn[:, Ds:])))
            dist = np.linalg.norm(ag1.astype(np.float64) - g.astype(np.float64), axis=1)
            thr = float(np.float32(0.05))
            clear = np.abs(dist / thr - 1.0) > band(d.goal_dim)
            assert np.array_equal(got['goal_achieved'][clear], (dist <= thr)[clear].astype(np.uint8))
            assert np.array_equal(got['reward'][clear], -((dist > thr)[clear].astype(np.float32))) and np.signbit(got['reward']).all()
    env.close()


# 9. invalid calls
def case_invalid_calls(library):
    with handle(library, 'push', num_envs=8) as env:
        h, d = env.handle, env.handle.dims
        P, A = d.packed_dim, d.action_dim
        rows, acts = coded_tables(d, 4, 6)
        specs = out_specs(h, POL, 8)
        with Dev(h) as dev:
            tab = Table(h, dev, rows, acts)
            bufs = {n: dev.put(np.full(int(np.prod(s)) * np.dtype(dt).itemsize, SENTINEL, np.uint8)) for n, (dt, s) in specs.items()}

            def call(src_kw=None, out_kw=None, **kw):
                a = dict(d_rows=tab.d_rows, num_episodes=4, episode_steps=6, row_episode_stride=tab.es, row_time_stride=tab.ts, batch=8,
                         d_actions=tab.d_acts, action_episode_stride=tab.aes, action_time_stride=tab.ats, d_x=bufs['x'], d_x_next=bufs['x_next'],
                         d_action=bufs['action'], d_reward=bufs['reward'], d_goal_achieved=bufs['goal_achieved'], d_index=bufs['index'])
                a.update(kw)
                src, out = h.her_structs(**a)
                for k, v in (src_kw or {}).items():
                    setattr(src, k, v)
                for k, v in (out_kw or {}).items():
                    setattr(out, k, v)
                return h.L.lib.pmg_her_sample_device(h.h, C.byref(src), C.byref(out))
            bad = [
                dict(src_kw={'struct_size': C.sizeof(PmgHerSource) - 8}), dict(out_kw={'struct_size': 0}),
                dict(num_episodes=0), dict(num_episodes=-3), dict(episode_steps=0),
                dict(num_episodes=1 << 20, episode_steps=2047), dict(num_episodes=2 ** 31 - 1, episode_steps=1),
                dict(batch=-1), dict(d_rows=None),
                dict(row_episode_stride=P - 1), dict(row_time_stride=P - 1), dict(row_episode_stride=0), dict(row_time_stride=0),
                dict(row_episode_stride=-P),
                dict(action_episode_stride=A - 1), dict(action_time_stride=A - 1), dict(action_episode_stride=0), dict(action_time_stride=0),
                dict(state_kind=GOAL), dict(state_kind=7), dict(state_kind=-1),
                dict(future_p=-0.01), dict(future_p=1.5), dict(future_p=float('nan')),
                dict(d_actions=None),
            ]
            for k, kw in enumerate(bad):
                assert call(**kw) == E_INVALID, (k, kw)
                assert h.L.error(h.h), k
            h.sync()
            for n, (dt, s) in specs.items():
                assert (dev.get(bufs[n], int(np.prod(s)) * np.dtype(dt).itemsize, np.uint8) == SENTINEL).all(), n
            assert call(batch=0) == 0
            # zero strides where the extent is 1; d_actions may be NULL when d_action is
            assert call(num_episodes=1, row_episode_stride=0, action_episode_stride=0) == 0
            assert call(d_actions=None, d_action=None) == 0
            h.sync()
            assert (dev.get(bufs['goal_achieved'], 8, np.uint8) != SENTINEL).all()
        with Dev(h) as dev:      # T = 1: the time stride of the actions may be 0
            r1, a1 = coded_tables(d, 3, 1)
            tab = Table(h, dev, r1, a1)
            tab.ats = 0
            got = sample(h, tab, 65, seed=1, counter=1)
            check_raw(h, tab, POL, got)


# 10. host face
def case_host_face(library):
    with handle(library, 'push', num_envs=8) as env:
        h = env.handle
        NC.prime(h)
        rows, acts = clip_tables(h, 5, 4, 41)
        for kind, name in ((OBS, 'observation'), (POL, 'policy_state')):
            for raw in (True, False):
                with Dev(h) as dev:
                    want = sample(h, Table(h, dev, rows, acts), 130, kind=kind, raw=raw, future_p=0.7, seed=2 ** 63 + 1, counter=9)
                for tm in (True, False):
                    r, a = (rows, acts) if tm else (rows.transpose(1, 0, 2), acts.transpose(1, 0, 2))
                    got = env.her.sample(r, a, 130, future_p=0.7, seed=2 ** 63 + 1, counter=9, kind=name, raw=raw, time_major=tm)
                    assert set(got) == set(OUTPUTS)
                    for n in OUTPUTS:
                        assert np.array_equal(bits(np.ascontiguousarray(got[n]).astype(want[n].dtype)), bits(want[n])), (n, kind, raw, tm)
                    assert got['goal_achieved'].dtype == np.bool_
        assert env.her is env.her
        assert env.her.sample(rows, acts, 0)['x'].shape == (0, 10)
        import pytest
        for args, kw in (((rows[:, :, :-1], acts, 4), {}), ((rows, acts[:-1], 4), {}), ((rows[:1], acts[:0], 4), {}), ((rows[0], acts, 4), {}),
                         ((rows, acts[:, :, :-1], 4), {}), ((rows, acts, -1), {}), ((rows, acts, 4), {'kind': 'goal'}),
                         ((rows, acts, 4), {'future_p': 1.5}), ((rows, acts, 4), {'time_major': False})):
            with pytest.raises(ValueError):
                env.her.sample(*args, **kw)


def test_model_statistics():
    """the draws on the model alone: B = 65536, E = 8, T = 4, future_p = 0.8 -- every (e, t) cell count within 5 standard
    deviations of B / 32, the relabelled share within 5 standard deviations of 0.8"""
    B, E, T, p = 65536, 8, 4, 0.8
    for seed, counter in ((0, 0), (1, 0), (0, 1), (12345, 7), (2 ** 63 + 5, 2 ** 40)):
        ix = draws(seed, counter, B, E, T, p)
        check_ranges(ix, E, T)
        cells = np.bincount(ix[:, 0] * T + ix[:, 1], minlength=E * T)
        q = 1.0 / (E * T)
        dev_cells = np.abs(cells - B * q).max() / np.sqrt(B * q * (1 - q))
        share = (ix[:, 2] >= 0).mean()
        dev_share = abs(share - p) / np.sqrt(p * (1 - p) / B)
        print('seed %d counter %d: worst cell %.2f sd, relabelled share %.4f (%.2f sd)' % (seed, counter, dev_cells, share, dev_share))
        assert dev_cells < 5 and dev_share < 5
        f = ix[ix[:, 2] >= 0]
        assert (f[:, 2] > f[:, 1]).all() and (f[:, 2] <= T).all() and (f[:, 2] == T).any() and (f[:, 2] == f[:, 1] + 1).any()
