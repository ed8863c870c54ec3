"""The cases of the running-normaliser / policy-input tests (include/pmg.h pmg_norm_*, pmg_policy_input*) and
their numpy model, shared by two tiers: tests/test_normalizer_emulated.py runs them on the g++ build of the product
sources over the fiber emulator, tests/test_gpu_normalizer.py on libpmg_hip.so on the MI355X.  Every case takes the loaded
library and goes through the C ABI with caller-owned device buffers (pmg_device_alloc / pmg_upload / pmg_download).

Bars.  S and Q are sums of B float64 terms in some fixed order; any order of recursive double summation is within
(B - 1) 2^-53 sum|term| of the exact sum, the bar is B 2^-52 sum|term| against math.fsum of the float32-clipped values
(their squares are exact in float64: 48 bits).  mean / std / inv_std are one float32 rounding (2^-24) of a float64 value
that is itself good to a few 2^-53: the bar is 2^-22 relative to the float64 formulas evaluated on the DEVICE's own S, Q, n.
Policy inputs are float32 IEEE subtract / multiply / min / max in a stated order: bit-equal to numpy."""
import contextlib
import ctypes as C
import math

import numpy as np

import pybullet_multigoal_gym_amd as pmg
from pybullet_multigoal_gym_amd._lib import PMG_BUF_PACKED

OBS, POL, GOAL = 0, 1, 2
KINDS = (OBS, POL, GOAL)
TASKS = {'reach': ({}, (3, 3, 3)), 'push': ({}, (20, 7, 3)), 'block_stack': ({'num_block': 5}, (88, 19, 15))}
TASK_NAMES = list(TASKS)
UPDATE_BATCHES = (1, 63, 64, 65, 257, 4097)
INPUT_BATCHES = (1, 5, 64, 4097)
EPS, CLIP_IN, CLIP_OUT = 0.01, 200.0, 5.0
E_INVALID = -1
REL = 2.0 ** -22
SENTINEL = 0xA5


# ----------------------------------------------------------------------------------------------------------------------
# handles and device buffers
@contextlib.contextmanager
def handle(library, task, num_envs=64, **kw):
    """A fresh env of `task` (its constructor resets once) -> env; widths checked against the table of the issue."""
    opts, widths = TASKS[task]
    env = pmg.make_env(task=task, num_envs=num_envs, seed=3, seed_stride=1, _library=library, **dict(opts, **kw))
    d = env.dims
    assert (d.observation_dim, d.policy_state_dim, d.goal_dim) == widths
    try:
        yield env
    finally:
        env.close()


class Dev:
    """Device buffers of one handle, freed together."""

    def __init__(self, h):
        self.h, self.ptrs = h, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.h.device_free(p)

    def alloc(self, nbytes):
        p = self.h.device_alloc(nbytes)
        self.ptrs.append(p)
        return p

    def put(self, array, pad_bytes=0):
        a = np.ascontiguousarray(array)
        p = self.alloc(a.nbytes + pad_bytes + 16)
        self.h.upload(p, a)
        return p

    def get(self, ptr, shape, dtype):
        out = np.empty(shape, dtype)
        self.h.sync()
        self.h.download(out, ptr)
        return out


def width(h, which):
    return h.norm_width(which)


def totals(h, which):
    r = h.norm_read(which)
    return r['sum'], r['sumsq'], r['count']


def all_totals(h):
    return [np.concatenate([np.r_[t[0], t[1]], [t[2]]]) for t in (totals(h, w) for w in KINDS)]


def update_device(h, which, rows, mask=None):
    """pmg_norm_update_device on a contiguous copy of rows [B, D] on the device."""
    rows = np.ascontiguousarray(rows, np.float32)
    with Dev(h) as dev:
        d_rows = dev.put(rows)
        d_mask = dev.put(np.ascontiguousarray(mask, np.uint8)) if mask is not None else None
        h.norm_update_device(which, d_rows, rows.shape[1], rows.shape[0], d_mask)
        h.sync()


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def clip32(x, c):
    c = np.float32(c)
    return np.minimum(np.maximum(np.asarray(x, np.float32), -c), c)


def ref_totals(rows, clip_in=CLIP_IN):
    """exact float64 reference of S, Q per column + the sums of magnitudes the bars scale with"""
    x = clip32(rows, clip_in).astype(np.float64)
    D = x.shape[1]
    S = np.array([math.fsum(x[:, c]) for c in range(D)])
    Q = np.array([math.fsum(x[:, c] * x[:, c]) for c in range(D)])
    A = np.array([math.fsum(np.abs(x[:, c])) for c in range(D)])
    return S, Q, A, float(x.shape[0])


def check_totals(h, which, rows, clip_in=CLIP_IN, label=''):
    """the device's totals against the exact sums of `rows` (everything the normaliser was shown since it was empty)"""
    S, Q, A, B = ref_totals(rows, clip_in)
    s, q, n = totals(h, which)
    assert n == B, (label, n, B)
    es, eq = np.abs(s - S), np.abs(q - Q)
    bs, bq = B * 2.0 ** -52 * A, B * 2.0 ** -52 * Q
    print('%s which=%d B=%d: max |S err| / bar = %.3g, |Q err| / bar = %.3g' %
          (label, which, int(B), (es / np.maximum(bs, 1e-300)).max() if B else 0, (eq / np.maximum(bq, 1e-300)).max() if B else 0))
    assert (es <= bs).all(), (label, es.max(), bs.min())
    assert (eq <= bq).all(), (label, eq.max(), bq.min())


def derived_model(s, q, n, eps=EPS):
    """float64 formulas of the derived values on given totals"""
    if n == 0:
        return np.zeros_like(s), np.ones_like(s), np.ones_like(s)
    eps = float(np.float32(eps))
    m = s / n
    var = np.maximum(eps * eps, q / n - m * m)
    return m, np.sqrt(var), 1.0 / np.sqrt(var)


def check_derived(h, which, eps=EPS, label=''):
    r = h.norm_read(which)
    m, sd, inv = derived_model(r['sum'], r['sumsq'], r['count'], eps)
    for name, dev, ref in (('mean', r['mean'], m), ('std', r['std'], sd), ('inv_std', r['inv_std'], inv)):
        err = np.abs(dev.astype(np.float64) - ref)
        print('%s which=%d %s: max rel err = %.3g (bar %.3g)' % (label, which, name, (err / np.maximum(np.abs(ref), 1e-300)).max(), REL))
        assert (err <= REL * np.abs(ref)).all(), (label, name, err.max())


def policy_model(h, state_kind, state, goal, clip_in=CLIP_IN, clip_out=CLIP_OUT):
    """the float32 model of section 1, from the mean / inv_std the library reports, ops in the stated order"""
    out = []
    for which, v in ((state_kind, state), (GOAL, goal)):
        r = h.norm_read(which)
        c = clip32(v, clip_in)
        y = (c - r['mean'][None, :]) * r['inv_std'][None, :]
        assert y.dtype == np.float32
        out.append(clip32(y, clip_out))
    return np.concatenate(out, axis=1)


def uniform_rows(seed, B, D, lo=-3.0, hi=3.0):
    return np.random.RandomState(seed).uniform(lo, hi, (B, D)).astype(np.float32)


def input_rows(seed, B, D):
    """finite, no subnormals, with values beyond the input clip and values whose normalised value is beyond the output clip"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3, 3, (B, D))
    k = rs.randint(0, 8, (B, D))
    x = np.where(k == 0, rs.uniform(-60, 60, (B, D)), x)       # far beyond 5 standard deviations
    x = np.where(k == 1, rs.choice([-1e3, 1e3, -201.0, 250.0], (B, D)), x)   # beyond clip_input
    x = x.astype(np.float32)
    x.flat[0], x.flat[x.size // 2] = 1e3, -47.0                 # (a single row has them too)
    x[(x != 0) & (np.abs(x) < 1e-30)] = 0.0
    return x


def prime(h, seed=11):
    """give the three normalisers of a handle something to normalise with"""
    for which in KINDS:
        h.norm_update(which, uniform_rows(seed + which, 300, width(h, which)))


# ----------------------------------------------------------------------------------------------------------------------
# 1. fresh handle
def case_fresh_handle(library, task):
    with handle(library, task) as env:
        h = env.handle
        for which in KINDS:
            r = h.norm_read(which)
            D = width(h, which)
            assert r['count'] == 0 and not r['sum'].any() and not r['sumsq'].any()
            assert np.array_equal(r['mean'], np.zeros(D, np.float32))
            assert np.array_equal(r['std'], np.ones(D, np.float32)) and np.array_equal(r['inv_std'], np.ones(D, np.float32))
        for kind in (OBS, POL):
            s, g = input_rows(1, 65, width(h, kind)), input_rows(2, 65, width(h, GOAL))
            out = h.policy_input(kind, s, g)
            assert np.array_equal(out, clip32(clip32(np.concatenate([s, g], 1), CLIP_IN), CLIP_OUT))


# 2. update against float64
def case_update_against_float64(library, task):
    with handle(library, task) as env:
        h = env.handle
        for which in KINDS:
            for k, B in enumerate(UPDATE_BATCHES):
                h.norm_write(which, np.zeros(width(h, which)), np.zeros(width(h, which)), 0.0)
                rows = uniform_rows(100 * which + k, B, width(h, which))
                update_device(h, which, rows)
                check_totals(h, which, rows, label='%s update' % task)
                check_derived(h, which, label='%s update' % task)


# 3. float32 accumulators would fail
def case_catches_float32_accumulators(library, task):
    with handle(library, task) as env:
        h = env.handle
        h.norm_configure(1e-6, CLIP_IN, CLIP_OUT)
        for which in KINDS:
            D = width(h, which)
            rows = (1.0 + 1e-3 * np.random.RandomState(7 + which).uniform(-1, 1, (4097, D))).astype(np.float32)
            update_device(h, which, rows)
            S, Q, _, n = ref_totals(rows)
            _, sd, _ = derived_model(S, Q, n, 1e-6)
            assert (np.abs(sd - 1e-3 / math.sqrt(3)) < 0.05 * 1e-3 / math.sqrt(3)).all()      # ~ 5.8e-4
            std = h.norm_read(which)['std'].astype(np.float64)
            print('%s which=%d: std rel err vs the float64 model = %.3g' % (task, which, (np.abs(std - sd) / sd).max()))
            assert (np.abs(std - sd) <= REL * sd).all()


# 4. floors and clips
def case_floors_and_clips(library, task):
    with handle(library, task) as env:
        h = env.handle
        for which in KINDS:
            D = width(h, which)
            u = np.random.RandomState(which).uniform(-1, 1, (257, D))
            h.norm_update(which, (1000.0 + u).astype(np.float32))      # every value clipped to 200: variance 0
            r = h.norm_read(which)
            assert np.array_equal(r['std'], np.full(D, EPS, np.float32)) and np.array_equal(r['mean'], np.full(D, 200, np.float32))
            assert np.array_equal(r['sum'], np.full(D, 200.0 * 257)) and np.array_equal(r['sumsq'], np.full(D, 40000.0 * 257))
            h.norm_write(which, np.zeros(D), np.zeros(D), 0.0)
            h.norm_update(which, (3.0 + 1e-3 * u).astype(np.float32))   # std 5.8e-4 < eps
            assert np.array_equal(h.norm_read(which)['std'], np.full(D, 0.01, np.float32))


# 5. stride and alignment
def case_stride_and_alignment(library, task):
    with handle(library, task) as env:
        h, d = env.handle, env.dims
        offs = {POL: d.observation_dim, GOAL: d.observation_dim + d.policy_state_dim + d.goal_dim}
        if task == 'reach':
            assert offs[GOAL] == 9                                      # 36 bytes: not 16-byte aligned
        o, p, ag, dg = h.read_outputs()[:4]
        packed = h.device_ptr(PMG_BUF_PACKED)
        # a synthetic table of 257 packed-shaped rows as well: more than one chunk, J row slots not dividing it
        big = uniform_rows(5, 257, d.packed_dim)
        with Dev(h) as dev:
            d_big = dev.put(big)
            for which, env_rows in ((POL, p), (GOAL, dg)):
                D = width(h, which)
                for base, B, rows in ((packed, h.N, env_rows), (d_big, 257, big[:, offs[which]:offs[which] + D])):
                    h.norm_write(which, np.zeros(D), np.zeros(D), 0.0)
                    h.norm_update_device(which, base + 4 * offs[which], d.packed_dim, B)
                    in_place = totals(h, which)
                    h.norm_write(which, np.zeros(D), np.zeros(D), 0.0)
                    update_device(h, which, rows)
                    copied = totals(h, which)
                    assert in_place[2] == copied[2] == B
                    assert np.array_equal(in_place[0], copied[0]) and np.array_equal(in_place[1], copied[1])
                    check_totals(h, which, rows, label='%s in place' % task)


# 6. mask
def case_mask(library, task):
    with handle(library, task) as env:
        h = env.handle
        rs = np.random.RandomState(17)
        for which in KINDS:
            D, B = width(h, which), 257
            rows = uniform_rows(40 + which, B, D)
            single = np.zeros(B, np.uint8)
            single[200] = 1
            for mask in ((rs.uniform(size=B) < 0.4).astype(np.uint8) * 3, single):      # any nonzero byte takes the row
                h.norm_write(which, np.zeros(D), np.zeros(D), 0.0)
                update_device(h, which, rows, mask)
                check_totals(h, which, rows[mask != 0], label='%s masked' % task)
                check_derived(h, which, label='%s masked' % task)
            before = h.norm_read(which)
            update_device(h, which, rows, np.zeros(B, np.uint8))
            after = h.norm_read(which)
            for k in before:
                assert np.array_equal(np.atleast_1d(before[k]).view(np.uint8), np.atleast_1d(after[k]).view(np.uint8)), k


# 7. incremental and deterministic
def case_incremental_and_deterministic(library, task):
    def run(h):
        for which in KINDS:
            for k, B in enumerate((65, 257, 64)):
                update_device(h, which, uniform_rows(60 + 3 * which + k, B, width(h, which)))
        return all_totals(h)

    with handle(library, task) as env, handle(library, task) as env2:
        h = env.handle
        first, second = run(h), run(env2.handle)
        for a, b in zip(first, second):
            assert np.array_equal(a, b)
        for which in KINDS:
            D = width(h, which)
            rows = np.concatenate([uniform_rows(60 + 3 * which + k, B, D) for k, B in enumerate((65, 257, 64))])
            check_totals(h, which, rows, label='%s three updates' % task)
            h.norm_write(which, np.zeros(D), np.zeros(D), 0.0)
            update_device(h, which, rows)
            check_totals(h, which, rows, label='%s one update' % task)


# 8. policy input, exact
def device_policy_input(h, kind, state, goal, packed_layout=False, out_shift=0):
    """pmg_policy_input_device on caller-owned buffers -> out [B, Ds + Dg].  packed_layout: both inputs sit in ONE table of
    packed-shaped rows at the columns of that kind / the desired goal; out_shift floats move d_out off its 16-byte boundary.
    The floats of d_out in front of and behind the result must keep their sentinel."""
    d = h.dims
    B, Ds, Dg = state.shape[0], state.shape[1], goal.shape[1]
    W = Ds + Dg
    with Dev(h) as dev:
        if packed_layout:
            so, go = (0 if kind == OBS else d.observation_dim), d.observation_dim + d.policy_state_dim + d.goal_dim
            table = np.full((B, d.packed_dim), np.float32(7e4))      # anything read outside the two column ranges would show
            table[:, so:so + Ds] = state
            table[:, go:go + Dg] = goal
            d_tab = dev.put(table)
            d_s, ss, d_g, gs = d_tab + 4 * so, d.packed_dim, d_tab + 4 * go, d.packed_dim
        else:
            d_s, ss, d_g, gs = dev.put(state), Ds, dev.put(goal), Dg
        nbytes = 4 * (out_shift + B * W) + 64
        d_out = dev.put(np.full(nbytes, SENTINEL, np.uint8))
        h.policy_input_device(kind, d_s, ss, d_g, gs, B, d_out + 4 * out_shift)
        raw = dev.get(d_out, nbytes, np.uint8)
    assert (raw[:4 * out_shift] == SENTINEL).all() and (raw[4 * (out_shift + B * W):] == SENTINEL).all(), 'floats outside d_out written'
    return raw[4 * out_shift:4 * (out_shift + B * W)].copy().view(np.float32).reshape(B, W)


def case_policy_input_exact(library, task):
    with handle(library, task) as env:
        h = env.handle
        prime(h)
        both_paths = 0
        for kind in (OBS, POL):
            Ds, Dg = width(h, kind), width(h, GOAL)
            for k, B in enumerate(INPUT_BATCHES):
                state, goal = input_rows(200 + k, B, Ds), input_rows(300 + k, B, Dg)
                want = policy_model(h, kind, state, goal)
                assert (np.abs(np.concatenate([state, goal], 1)) > CLIP_IN).any() and (np.abs(want) == CLIP_OUT).any()
                for packed_layout, shift in ((False, 0), (True, 0), (False, 1), (True, 3)):
                    got = device_policy_input(h, kind, state, goal, packed_layout, shift)
                    assert np.array_equal(got, want), (task, kind, B, packed_layout, shift, np.argwhere(got != want)[:4])
                if (B * (Ds + Dg)) % 4 and B * (Ds + Dg) >= 4:
                    both_paths += 1                                   # full float4s and a dword tail in one call
                assert np.array_equal(h.policy_input(kind, state, goal), want)      # the host variant
        assert both_paths >= 2


# 9. with the env
_plain_rollouts = {}     # the rollout without any normaliser call, once per library: it does not depend on the row buffers


def case_with_the_env(library, overlap=False):
    def rollout(normalise):
        env = pmg.make_env(task='reach', num_envs=64, seed=5, seed_stride=1, _library=library)
        h = env.handle
        if overlap and normalise:
            h.comm_overlap(True)
        rs = np.random.RandomState(9)
        shown = {w: [] for w in KINDS}
        packed = []
        env.reset()
        for step in range(4):
            if step:
                env.step(rs.uniform(-1, 1, (64, 3)).astype(np.float32))
            o, p, ag, dg = h.read_outputs()[:4]
            rows = np.empty((64, env.dims.packed_dim), np.float32)
            h.sync()
            h.download(rows, h.device_ptr(PMG_BUF_PACKED))
            packed.append(rows)
            if normalise:
                env.normalizer.update_from_env()
                for w, v in ((OBS, o), (POL, p), (GOAL, dg)):
                    shown[w].append(v)
                for kind, name, v in ((OBS, 'observation', o), (POL, 'policy_state', p)):
                    from_env = env.normalizer.policy_input_from_env(name)
                    assert np.array_equal(from_env, env.normalizer.policy_input(v, dg, name))
                    assert np.array_equal(from_env, policy_model(h, kind, v, dg))
        if normalise:
            for w in KINDS:
                check_totals(h, w, np.concatenate(shown[w]), label='reach env rows')
                check_derived(h, w, label='reach env rows')
            assert h.norm_read(GOAL)['std'].max() > EPS          # the goals of 64 seeded envs do differ
        env.close()
        return packed

    if id(library) not in _plain_rollouts:
        _plain_rollouts[id(library)] = rollout(False)
    with_norm, without = rollout(True), _plain_rollouts[id(library)]
    for a, b in zip(with_norm, without):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))          # the normaliser only reads
    assert not np.array_equal(with_norm[0], with_norm[3])


# 10. state and errors
def case_state_dict_round_trip(library, task):
    with handle(library, task) as env, handle(library, task) as env2:
        env.normalizer.configure(0.02, 150.0, 4.0)
        prime(env.handle)
        sd = env.normalizer.state_dict()
        env2.normalizer.load_state_dict(sd)
        for kind, name in ((OBS, 'observation'), (POL, 'policy_state')):
            s, g = input_rows(1, 65, width(env.handle, kind)), input_rows(2, 65, width(env.handle, GOAL))
            a, b = env.normalizer.policy_input(s, g, name), env2.normalizer.policy_input(s, g, name)
            assert np.array_equal(a, b) and np.array_equal(a, policy_model(env.handle, kind, s, g, 150.0, 4.0))
        for a, b in zip(all_totals(env.handle), all_totals(env2.handle)):
            assert np.array_equal(a, b)


def case_write_and_configure(library, task):
    with handle(library, task) as env:
        h = env.handle
        prime(h)
        for which in KINDS:
            D = width(h, which)
            before = totals(h, which)
            std_before = h.norm_read(which)['std']
            h.norm_configure(2.5, CLIP_IN, CLIP_OUT)                 # a floor above the data's spread (uniform [-3, 3]: 1.73)
            r = h.norm_read(which)
            assert np.array_equal(r['std'], np.full(D, 2.5, np.float32)) and np.array_equal(r['inv_std'], np.full(D, 0.4, np.float32))
            assert np.array_equal(r['sum'], before[0]) and np.array_equal(r['sumsq'], before[1]) and r['count'] == before[2]
            h.norm_configure(EPS, CLIP_IN, CLIP_OUT)
            assert np.array_equal(h.norm_read(which)['std'], std_before)
            h.norm_write(which, np.zeros(D), np.zeros(D), 0.0)       # zeros = reset
            r = h.norm_read(which)
            assert r['count'] == 0 and not r['mean'].any() and (r['std'] == 1).all() and (r['inv_std'] == 1).all()
            # NULL totals with count 0 reset as well; a restore brings the statistics back
            assert h.L.lib.pmg_norm_write(h.h, C.c_int(which), None, None, C.c_double(0.0)) == 0
            h.norm_write(which, before[0], before[1], before[2])
            assert np.array_equal(h.norm_read(which)['std'], std_before)
            check_derived(h, which, label='%s restored' % task)


def case_invalid_calls(library, task):
    with handle(library, task) as env:
        h, L = env.handle, env.handle.L.lib
        prime(h)
        before = all_totals(h)
        i64, vp, f32 = C.c_int64, C.c_void_p, C.c_float
        with Dev(h) as dev:
            D = [width(h, w) for w in KINDS]
            d_rows = dev.put(np.zeros((8, max(D)), np.float32))
            d_out = dev.alloc(4 * 8 * (max(D) + D[GOAL]))
            host = np.zeros((8, max(D)), np.float32)
            hp = host.ctypes.data_as(vp)
            bad = [
                lambda: L.pmg_norm_configure(h.h, f32(0.0), f32(200), f32(5)),
                lambda: L.pmg_norm_configure(h.h, f32(0.01), f32(-1), f32(5)),
                lambda: L.pmg_norm_configure(h.h, f32(0.01), f32(200), f32(float('nan'))),
                lambda: L.pmg_norm_update_device(h.h, 3, vp(d_rows), i64(D[0]), i64(8), None),
                lambda: L.pmg_norm_update_device(h.h, -1, vp(d_rows), i64(D[0]), i64(8), None),
                lambda: L.pmg_norm_update_device(h.h, OBS, None, i64(D[OBS]), i64(8), None),
                lambda: L.pmg_norm_update_device(h.h, OBS, vp(d_rows), i64(D[OBS]), i64(-1), None),
                lambda: L.pmg_norm_update_device(h.h, OBS, vp(d_rows), i64(D[OBS] - 1), i64(8), None),
                lambda: L.pmg_norm_update(h.h, 3, hp, i64(8), None),
                lambda: L.pmg_norm_update(h.h, GOAL, None, i64(8), None),
                lambda: L.pmg_norm_update(h.h, GOAL, hp, i64(-2), None),
                lambda: L.pmg_norm_read(h.h, 5, None, None, None, None, None, None),
                lambda: L.pmg_norm_write(h.h, 3, hp, hp, C.c_double(1.0)),
                lambda: L.pmg_norm_write(h.h, OBS, hp, hp, C.c_double(-1.0)),
                lambda: L.pmg_norm_write(h.h, OBS, None, hp, C.c_double(2.0)),
                lambda: L.pmg_policy_input_device(h.h, GOAL, vp(d_rows), i64(D[GOAL]), vp(d_rows), i64(D[GOAL]), i64(8), vp(d_out)),
                lambda: L.pmg_policy_input_device(h.h, 7, vp(d_rows), i64(D[OBS]), vp(d_rows), i64(D[GOAL]), i64(8), vp(d_out)),
                lambda: L.pmg_policy_input_device(h.h, OBS, None, i64(D[OBS]), vp(d_rows), i64(D[GOAL]), i64(8), vp(d_out)),
                lambda: L.pmg_policy_input_device(h.h, OBS, vp(d_rows), i64(D[OBS]), None, i64(D[GOAL]), i64(8), vp(d_out)),
                lambda: L.pmg_policy_input_device(h.h, OBS, vp(d_rows), i64(D[OBS]), vp(d_rows), i64(D[GOAL]), i64(8), None),
                lambda: L.pmg_policy_input_device(h.h, OBS, vp(d_rows), i64(D[OBS]), vp(d_rows), i64(D[GOAL]), i64(-8), vp(d_out)),
                lambda: L.pmg_policy_input_device(h.h, OBS, vp(d_rows), i64(D[OBS] - 1), vp(d_rows), i64(D[GOAL]), i64(8), vp(d_out)),
                lambda: L.pmg_policy_input_device(h.h, POL, vp(d_rows), i64(D[POL]), vp(d_rows), i64(D[GOAL] - 1), i64(8), vp(d_out)),
                lambda: L.pmg_policy_input(h.h, GOAL, hp, hp, i64(8), hp),
                lambda: L.pmg_policy_input(h.h, OBS, None, hp, i64(8), hp),
                lambda: L.pmg_policy_input(h.h, OBS, hp, hp, i64(8), None),
                lambda: L.pmg_policy_input(h.h, OBS, hp, hp, i64(-1), hp),
                lambda: L.pmg_policy_input_env_device(h.h, GOAL, vp(d_out)),
                lambda: L.pmg_policy_input_env_device(h.h, OBS, None),
            ]
            for k, call in enumerate(bad):
                assert call() == E_INVALID, k
                assert h.L.error(h.h), k
            # batch == 0 succeeds and changes nothing
            assert L.pmg_norm_update_device(h.h, OBS, vp(d_rows), i64(D[OBS]), i64(0), None) == 0
            assert L.pmg_norm_update(h.h, POL, hp, i64(0), None) == 0
            assert L.pmg_policy_input_device(h.h, OBS, vp(d_rows), i64(D[OBS]), vp(d_rows), i64(D[GOAL]), i64(0), vp(d_out)) == 0
            assert L.pmg_policy_input(h.h, OBS, hp, hp, i64(0), hp) == 0
            h.sync()
        for a, b in zip(before, all_totals(h)):
            assert np.array_equal(a, b)
        r = h.norm_read(OBS)
        assert r['count'] == 300 and (np.abs(r['std'] - 1.73) < 0.2).all()      # the settings survived the refused calls too
