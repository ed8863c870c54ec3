"""The cases of the critic / TD-target tests (include/pmg.h pmg_q_device, pmg_td_target_device) and their numpy model,
shared by three files: tests/test_td_emulated.py runs them on the g++ build of the product sources over the fiber emulator,
tests/test_gpu_td.py on libpmg_hip.so on the MI355X, tests/test_td_host.py covers env.critic.  The model of a network is
tests/actor_cases.py's (the exact float32 fmaf chain); every case takes the loaded library and goes through the C ABI with buffers from
pmg_device_alloc.

Bars.  Both networks are float32 fmaf chains in ascending k, the clip is min / max, the epilogue is one fmaf and a min / max: with an
identity actor output everything is compared bit for bit with the numpy model (chain, clip, chain, fmaf, clip); the one thing left open
is the sign of a zero y where t and a clip are zeros of opposite sign (eq_y).  With a tanh actor
output a' is the float32 library tanh: it is held to the float64 tanh of the model's bit-exact z within actor_cases.ACTION_TOL (the
project's bar for the same function), and q' and y are bit-equal to the model evaluated from the DEVICE's own a'."""
import ctypes as C

import numpy as np

import actor_cases as AC
import her_cases as HC
import normalizer_cases as NC
import pybullet_multigoal_gym_amd as pmg
from actor_cases import ACTION_TOL, CANARY_BYTES, POISON, Net, bits, check_z, fmaf, forward, network
from normalizer_cases import POL, SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PMG_BUF_PACKED, PmgMlp, PmgTdTarget

E_INVALID = -1
TILE = AC.TILE
BATCHES = (1, 31, 32, 33, 101)
Q_XDIMS, Q_ADIMS = (1, 2, 31, 32, 252), (1, 3, 4)
TD_DX, TD_A = (1, 6, 31, 33), (1, 3, 4)
TD_HIDDEN = ((33,), (256, 256, 256))
INF = float('inf')
F32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def clip1(z):
    return np.minimum(np.maximum(np.asarray(z, F32), F32(-1)), F32(1))


def q_model(x, a, Wc, bc):
    """the critic's chain on the rows x | a -> [B]"""
    return forward(np.concatenate([x, a], 1), Wc, bc)[:, 0]


def epilogue(q, r, gamma, lo=-INF, hi=INF, term=None):
    """t = terminal ? r : fmaf(gamma, q, r); y = fminf(fmaxf(t, lo), hi) -> t, y"""
    t = fmaf(np.full(q.shape, gamma, F32), q, r).reshape(q.shape)
    if term is not None:
        t = np.where(np.asarray(term) != 0, np.asarray(r, F32), t)
    return t, np.minimum(np.maximum(t, F32(lo)), F32(hi))


def td_model(x, r, Wa, ba, Wc, bc, gamma, lo=-INF, hi=INF, term=None, a=None):
    """-> dict(z, a, q, t, y) of an identity-output actor, or from the given a' (the device's own, tanh actors)"""
    z = forward(x, Wa, ba)
    a = clip1(z) if a is None else a
    q = q_model(x, a, Wc, bc)
    t, y = epilogue(q, r, gamma, lo, hi, term)
    return {'z': z, 'a': a, 'q': q, 't': t, 'y': y}


_cache = {}      # models per key: computed once, shared by the tiers, never written


def cached(key, make):
    if key not in _cache:
        v = make()
        for a in (v.values() if isinstance(v, dict) else v):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def eq_bits(got, want, label):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (label, np.argwhere(bits(got) != bits(want))[:4], got[bits(got) != bits(want)][:4],
                                                                                want[bits(got) != bits(want)][:4])


# ----------------------------------------------------------------------------------------------------------------------
# device calls
def put_rows(h, dev, rows, pad=0, shift=0):
    """[B, W] rows with `pad` floats of poison behind each, `shift` floats off a 16-byte boundary -> pointer, stride"""
    B, W = rows.shape
    buf = np.full((B, W + pad), POISON, F32)
    buf[:, :W] = rows
    p = dev.alloc(buf.nbytes + 32)
    p += (-p) % 16 + 4 * shift
    h.upload(p, buf)
    return p, W + pad


class Out:
    """a canary-framed output of `nbytes`, `shift` bytes off a 16-byte boundary"""

    def __init__(self, dev, nbytes, shift=0):
        self.dev, self.off, self.nbytes = dev, CANARY_BYTES + shift, nbytes
        self.base = dev.put(np.full(self.off + nbytes + CANARY_BYTES, SENTINEL, np.uint8))
        assert self.base % 16 == 0
        self.ptr = self.base + self.off

    def read(self, dtype=F32, written=True):
        raw = self.dev.get(self.base, self.off + self.nbytes + CANARY_BYTES, np.uint8)
        assert (raw[:self.off] == SENTINEL).all() and (raw[self.off + self.nbytes:] == SENTINEL).all(), 'bytes around an output were written'
        if not written:
            assert (raw == SENTINEL).all(), 'an output was written although it was NULL or the call was refused'
            return None
        return raw[self.off:self.off + self.nbytes].copy().view(dtype)


def device_q(h, Wc, bc, x, a, x_pad=0, a_pad=0, x_shift=0, a_shift=0, q_pad=0, q_shift=0):
    """pmg_q_device on canary-framed buffers -> q [B]"""
    B = x.shape[0]
    with Dev(h) as dev:
        net = Net(h, dev, Wc, bc, 0)
        d_x, xs = put_rows(h, dev, x, x_pad, x_shift)
        d_a, as_ = put_rows(h, dev, a, a_pad, a_shift)
        out = Out(dev, 4 * B * (1 + q_pad), 4 * q_shift)
        h.q_device(net.mlp, d_x, xs, x.shape[1], d_a, as_, a.shape[1], B, out.ptr, 1 + q_pad)
        rows = out.read(np.uint8).reshape(B, 4 * (1 + q_pad))
    assert (rows[:, 4:] == SENTINEL).all(), 'the padding between outputs was written'
    return np.ascontiguousarray(rows[:, :4]).view(F32)[:, 0]


def device_td(h, Wa, ba, Wc, bc, x, r, gamma, lo=-INF, hi=INF, term=None, act_out=0, critic_out=0, x_pad=0, shift=0, null=()):
    """pmg_td_target_device on canary-framed buffers -> dict(y, q, a) (None for an output passed as NULL).  shift: floats off the
    16-byte boundary for every float pointer; d_terminal sits at an odd address."""
    B, A = x.shape[0], Wa[-1].shape[0]
    with Dev(h) as dev:
        actor, critic = Net(h, dev, Wa, ba, act_out), Net(h, dev, Wc, bc, critic_out)
        d_x, xs = put_rows(h, dev, x, x_pad, shift)
        d_r, _ = put_rows(h, dev, np.asarray(r, F32)[None, :], 0, (shift + 1) & 3)
        d_t = None
        if term is not None:
            d_t = dev.alloc(B + 32)
            d_t += (-d_t) % 16 + 1
            h.upload(d_t, np.ascontiguousarray(term, np.uint8))
        outs = {'y': Out(dev, 4 * B, 4 * shift), 'q': Out(dev, 4 * B, 4 * ((shift + 2) & 3)), 'a': Out(dev, 4 * B * A, 4 * ((shift + 3) & 3))}
        td = h.td_struct(B, d_x, xs, d_r, outs['y'].ptr, gamma, lo, hi, d_t, None if 'q' in null else outs['q'].ptr, None if 'a' in null else outs['a'].ptr)
        h.td_target_device(actor.mlp, critic.mlp, td)
        res = {k: o.read(written=k not in null) for k, o in outs.items()}
    if res['a'] is not None:
        res['a'] = res['a'].reshape(B, A)
    return res


def eq_y(got, want, label):
    """y bit for bit, except the sign of a zero: fminf / fmaxf of -0.0 and +0.0 may return either (C leaves it open; v_min_f32 takes
    -0.0 as the smaller, x86's minss returns its second operand), and HER meets exactly that: r = -0.0 against clip_hi = +0.0"""
    eq_bits(np.asarray(got, F32) + F32(0), np.asarray(want, F32) + F32(0), label)


def check_td(got, want, label):
    eq_y(got['y'], want['y'], (label, 'y'))
    for k in ('q', 'a'):
        if got[k] is not None:
            eq_bits(got[k], want[k], (label, k))


# ----------------------------------------------------------------------------------------------------------------------
# 1. q equals the forward on concatenated rows
def q_case(x_dim, a_dim, hidden, B):
    def make():
        Wc, bc = network(300 + 7 * x_dim + a_dim + len(hidden), (x_dim + a_dim,) + hidden + (1,))
        rs = np.random.RandomState(x_dim * 11 + a_dim)
        x, a = rs.uniform(-2, 2, (B, x_dim)).astype(F32), rs.uniform(-1, 1, (B, a_dim)).astype(F32)
        return Wc, bc, x, a, q_model(x, a, Wc, bc)
    return cached(('q', x_dim, a_dim, hidden, B), make)


def case_q_is_forward(library, x_dims=Q_XDIMS):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        n = 0
        for x_dim in x_dims:
            for a_dim in Q_ADIMS:
                for hidden in ((33,), (256, 256)):
                    B = BATCHES[n % len(BATCHES)]
                    n += 1
                    Wc, bc, x, a, q = q_case(x_dim, a_dim, hidden, B)
                    got = device_q(h, Wc, bc, x, a, x_pad=n % 3, a_pad=(n + 1) % 4, x_shift=n % 4, a_shift=(n + 2) % 4, q_pad=n % 2, q_shift=(n + 1) % 4)
                    check_z(got, q, (x_dim, a_dim, hidden, B, 'model'))
                    eq_bits(got, q, (x_dim, a_dim, hidden, B, 'model, bits'))
                    own = AC.device_forward(h, Wc, bc, np.concatenate([x, a], 1))[:, 0]
                    eq_bits(got, own, (x_dim, a_dim, hidden, B, 'pmg_mlp_forward_device'))


# 2. exact integers name the column
def case_exact_integers(library):
    """one-layer identity critic W[0][k] = k + 1 on one-hot rows x | a: q is the integer of the hot column, so a swapped or shifted
    concatenation names itself.  The TD path: x' one-hot at c, an identity actor W[j][c] = (j == c % A), so a' is one-hot at c % A (exactly 1,
    which the clip leaves) and q' = (c + 1) + (Dx + c % A + 1); gamma = 1, r = 0: y = q'."""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for x_dim, a_dim in ((1, 1), (29, 4), (32, 3), (252, 4)):
            D = x_dim + a_dim
            Wc = [np.arange(1, D + 1, dtype=F32)[None, :]]
            rows = np.eye(D, dtype=F32)
            got = device_q(h, Wc, None, np.ascontiguousarray(rows[:, :x_dim]), np.ascontiguousarray(rows[:, x_dim:]), x_pad=1, a_pad=2, a_shift=1)
            assert np.array_equal(got, np.arange(1, D + 1, dtype=F32)), (x_dim, a_dim, got)
            c = np.arange(x_dim)
            Wa = np.zeros((a_dim, x_dim), F32)
            Wa[c % a_dim, c] = 1
            x = np.eye(x_dim, dtype=F32)
            got = device_td(h, [Wa], None, Wc, None, x, np.zeros(x_dim, F32), 1.0)
            hot = np.zeros((x_dim, a_dim), F32)
            hot[c, c % a_dim] = 1
            want = (c + 1 + x_dim + c % a_dim + 1).astype(F32)
            assert np.array_equal(got['a'], hot), (x_dim, a_dim, 'a')
            assert np.array_equal(got['q'], want) and np.array_equal(got['y'], want), (x_dim, a_dim, got['q'], want)


# 3. TD target, identity actor output: bit-exact end to end
def td_case(Dx, A, hidden, B, tanh=False):
    def make():
        big = len(hidden) > 1
        Wa, ba = network(500 + 13 * Dx + A + big, (Dx,) + hidden + (A,))
        Wc, bc = network(700 + 13 * Dx + A + big, (Dx + A,) + ((256, 33) if big else (33,)) + (1,))
        rs = np.random.RandomState(Dx * 17 + A + B)
        x = rs.uniform(-2, 2, (B, Dx)).astype(F32)
        r = -rs.randint(0, 2, B).astype(F32)
        # |z| up to about 1.5: the clip to [-1, 1] shows and most actions are off it
        scale = F32(2.0 ** np.floor(np.log2(1.5 / np.abs(forward(x, Wa, ba)).max())))
        Wa[-1], ba[-1] = Wa[-1] * scale, ba[-1] * scale
        m = td_model(x, r, Wa, ba, Wc, bc, 0.98)
        return dict(m, Wa=Wa, ba=ba, Wc=Wc, bc=bc, x=x, r=r)
    return cached(('td', Dx, A, hidden, B), make)


def case_td_identity(library, hidden, dxs=TD_DX):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        n = TD_HIDDEN.index(hidden)
        clipped = inside = False
        for Dx in dxs:
            for A in TD_A:
                B = BATCHES[n % len(BATCHES)]
                n += 1
                m = td_case(Dx, A, hidden, B)
                clipped |= bool((np.abs(m['z']) > 1).any())
                inside |= bool((np.abs(m['z']) < 1).any())
                got = device_td(h, m['Wa'], m['ba'], m['Wc'], m['bc'], m['x'], m['r'], 0.98, x_pad=n % 3, shift=n % 4)
                check_td(got, m, (Dx, A, hidden, B))
        assert inside and (clipped or len(dxs) < len(TD_DX))


def case_td_batches(library):
    """every batch size on one shape per hidden width, and a sample's result does not depend on the batch it is in"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for hidden, Dx, A in (((33,), 6, 3), ((256, 256, 256), 31, 4)):
            full = td_case(Dx, A, hidden, BATCHES[-1])
            for B in BATCHES:
                got = device_td(h, full['Wa'], full['ba'], full['Wc'], full['bc'], full['x'][:B], full['r'][:B], 0.98, x_pad=1, shift=B % 4)
                check_td(got, {k: full[k][:B] for k in ('y', 'q', 'a')}, (hidden, B))


# 4. TD target, tanh actor
def case_td_tanh(library):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A, hidden) in enumerate(((6, 3, (33,)), (33, 4, (256, 256, 256)), (1, 1, (33,)), (31, 3, (256, 256, 256)))):
            B = BATCHES[(n + 3) % len(BATCHES)]
            m = td_case(Dx, A, hidden, B)
            for lo, hi in ((-INF, INF), (-50.0, 0.0)):
                got = device_td(h, m['Wa'], m['ba'], m['Wc'], m['bc'], m['x'], m['r'], 0.98, lo, hi, act_out=1, shift=n)
                a64 = np.clip(np.tanh(m['z'].astype(np.float64)), -1.0, 1.0)
                err = np.abs(got['a'] - a64).max()
                worst = max(worst, err)
                assert err <= ACTION_TOL, (Dx, A, hidden, err)
                assert (np.abs(got['a']) < 1).all()
                q = q_model(m['x'], got['a'], m['Wc'], m['bc'])
                eq_bits(got['q'], q, (Dx, A, hidden, 'q from the device a'))
                eq_y(got['y'], epilogue(q, m['r'], 0.98, lo, hi)[1], (Dx, A, hidden, 'y from the device a'))
    print('tanh actor: largest |a - a64| = %.3g (bar %.3g)' % (worst, ACTION_TOL))
    return worst


# 5. stale tile contents
def stale_case(regime, B):
    """Dx = 29, A = 4: Dx + A = 33 is odd, so the critic's layer 0 multiplies column 33 of the tile by its stand-in zero.  The actor's
    hidden layer of 256 units leaves that column (and every column from 32 on) huge or inf:
      'huge': 29 -> 256 -> 4, hidden weights 1e30 on inputs in [0.5, 2) (activations of some 1e31), last layer 1e-38: z stays about 1e-4;
      'inf':  29 -> 256 -> 32 -> 4, hidden weights 1e30 on inputs of 1e9 (inf).  An inf activation times a zero weight is NaN in the
              chain itself, so the layer that READS the infs has negative weights: its sums are -inf, its ReLU is +0.0, and the actor's z is its
              last bias.  That layer writes columns 0..31 only: columns 32..255 keep the infs."""
    def make():
        rs = np.random.RandomState(90 + B)
        Dx, A = 29, 4
        if regime == 'huge':
            x = rs.uniform(0.5, 2, (B, Dx)).astype(F32)
            Wa = [np.full((256, Dx), 1e30, F32), (rs.uniform(0.5, 1, (A, 256)) * 1e-38).astype(F32)]
            ba = [None, rs.uniform(-0.5, 0.5, A).astype(F32)]
        else:
            x = (rs.uniform(0.5, 2, (B, Dx)) * 1e9).astype(F32)
            Wa = [np.full((256, Dx), 1e30, F32), -rs.uniform(0.5, 1, (32, 256)).astype(F32), rs.uniform(-1, 1, (A, 32)).astype(F32)]
            ba = [None, None, rs.uniform(-0.9, 0.9, A).astype(F32)]
        Wc, bc = network(95, (Dx + A, 33, 1))
        Wc[0] = (Wc[0] * (1.0 if regime == 'huge' else 1e-9)).astype(F32)
        r = -rs.randint(0, 2, B).astype(F32)
        with np.errstate(over='ignore', invalid='ignore'):
            hid = np.maximum(forward(x, Wa[:1], None), 0)
            m = td_model(x, r, Wa, ba, Wc, bc, 0.98)
        assert (np.isinf(hid).all() if regime == 'inf' else (np.isfinite(hid).all() and hid.min() > 1e30))
        assert np.isfinite(m['z']).all() and np.isfinite(m['y']).all() and len(set(m['y'].tolist())) > B // 2
        return dict(m, Wa=Wa, ba=ba, Wc=Wc, bc=bc, x=x, r=r)
    return cached(('stale', regime, B), make)


def case_stale_tile(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for regime in ('huge', 'inf'):
            last = None
            for B in (TILE, TILE + 1):
                m = stale_case(regime, B)
                got = device_td(h, m['Wa'], m['ba'], m['Wc'], m['bc'], m['x'], m['r'], 0.98, x_pad=1)
                for k in ('y', 'q', 'a'):
                    assert np.isfinite(got[k]).all(), (regime, B, k)
                check_td(got, m, (regime, B))
                last = got
            # row 32 sits in a tile with 31 rows past the batch: alone in a batch of one it gives the same bits
            m = stale_case(regime, TILE + 1)
            one = device_td(h, m['Wa'], m['ba'], m['Wc'], m['bc'], m['x'][TILE:], m['r'][TILE:], 0.98)
            for k in ('y', 'q', 'a'):
                eq_bits(one[k], last[k][TILE:], (regime, 'row 32', k))


# 6. epilogue
def case_epilogue(library):
    B, Dx, A = 101, 6, 3
    gamma = 0.98
    lo, hi = -1.0 / (1.0 - gamma), 0.0

    def make():
        Wa, ba = network(61, (Dx, 33, A))
        Wc, bc = network(62, (Dx + A, 33, 1))
        rs = np.random.RandomState(63)
        x = rs.uniform(-2, 2, (B, Dx)).astype(F32)
        r = -rs.randint(0, 2, B).astype(F32)
        scale = F32(2.0 ** np.ceil(np.log2(150.0 / np.abs(td_model(x, r, Wa, ba, Wc, bc, gamma)['q']).max())))
        Wc[-1], bc[-1] = Wc[-1] * scale, bc[-1] * scale          # |q'| up to 150 .. 300: both clips of [-50, 0] are reached
        term = (rs.uniform(0, 1, B) < 0.3).astype(np.uint8) * rs.randint(1, 256, B).astype(np.uint8)   # any non-zero byte is terminal
        return dict(td_model(x, r, Wa, ba, Wc, bc, gamma), Wa=Wa, ba=ba, Wc=Wc, bc=bc, x=x, r=r, term=term)
    m = cached(('epilogue',), make)
    net = (m['Wa'], m['ba'], m['Wc'], m['bc'], m['x'], m['r'])
    q, r, term = m['q'], m['r'], m['term']
    assert (m['t'] < lo).any() and (m['t'] > hi).any() and ((m['t'] > lo) & (m['t'] < hi)).any() and term.any() and not term.all()
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        # infinite clips change nothing: y is t
        got = device_td(h, *net, gamma)
        eq_bits(got['y'], m['t'], 'no clip')
        eq_bits(got['q'], q, 'q')
        # HER's clips
        got = device_td(h, *net, gamma, lo, hi, shift=1)
        want = epilogue(q, r, gamma, lo, hi)[1]
        assert (want == F32(lo)).any() and (want == 0).any()
        eq_y(got['y'], want, 'clips')
        # terminal rows: y = clip(r), q' still written
        for clips in ((-INF, INF), (lo, hi), (-0.5, -0.25)):
            got = device_td(h, *net, gamma, clips[0], clips[1], term=term, shift=2)
            t, y = epilogue(q, r, gamma, clips[0], clips[1], term)
            assert np.array_equal(t[term != 0], r[term != 0])
            eq_y(got['y'], y, ('terminal', clips))
            eq_bits(got['q'], q, ('terminal q', clips))
        # gamma = 0
        got = device_td(h, *net, 0.0, shift=3)
        eq_bits(got['y'], epilogue(q, r, 0.0)[1], 'gamma 0')
        assert np.array_equal(got['y'], r)
        # every optional output NULL independently, with and without d_terminal
        full = epilogue(q, r, gamma, lo, hi, term)[1]
        for null in ((), ('q',), ('a',), ('q', 'a')):
            for tm in (None, term):
                got = device_td(h, *net, gamma, lo, hi, term=tm, null=null, x_pad=2, shift=len(null))
                eq_y(got['y'], full if tm is not None else want, ('null', null))
                check_td(got, dict(m, y=got['y']), ('null', null))
        # the critic's own output activation is applied
        got = device_td(h, *net, gamma, critic_out=1)
        qt = np.tanh(q.astype(np.float64))
        assert np.abs(got['q'] - qt).max() <= ACTION_TOL
        eq_bits(got['y'], epilogue(got['q'], r, gamma)[1], 'tanh critic')


# 7. from the sampler
def case_from_the_sampler(library):
    """reach x 8, episodes of 5 steps recorded on the device, HER minibatch of 33 through the normalisers, then env.critic on the
    sampler's own device buffers: d_x_next, d_reward and d_goal_achieved (as d_terminal) for the TD target, d_x and d_action for q"""
    N, T, B = 8, 5, 33
    env = pmg.make_env(task='reach', num_envs=N, seed=5, seed_stride=1, max_episode_steps=T, _library=library)
    h, d = env.handle, env.handle.dims
    P, A, Dx = d.packed_dim, d.action_dim, d.policy_state_dim + d.goal_dim
    NC.prime(h)
    rs = np.random.RandomState(17)
    Wa, ba = network(71, (Dx, 64, A))
    Wc, bc = network(72, (Dx + A, 64, 1))
    env.actor.load(Wa, ba, out_activation='identity')
    env.critic.load(Wc, bc)
    assert env.critic is env.critic
    gamma, lo, hi = 0.98, -50.0, 0.0
    with Dev(h) as dev:
        d_rows, d_acts, d_act = dev.alloc(4 * (T + 1) * N * P), dev.alloc(4 * T * N * A), dev.alloc(4 * N * A)
        env.reset()
        for t in range(T + 1):
            if t:
                h.upload(d_act, rs.uniform(-1, 1, (N, A)).astype(F32))
                h.step_device(d_act)
            h.device_copy(d_rows + 4 * t * N * P, h.device_ptr(PMG_BUF_PACKED), 4 * N * P)
            if t:
                h.device_copy(d_acts + 4 * (t - 1) * N * A, d_act, 4 * N * A)
        specs = HC.out_specs(h, POL, B)
        outs = {k: Out(dev, int(np.prod(s)) * np.dtype(dt).itemsize) for k, (dt, s) in specs.items()}
        h.her_sample_device(d_rows, N, T, P, N * P, B, d_acts, A, N * A, state_kind=POL, raw=False, future_p=0.8, seed=4, counter=9,
                            d_x=outs['x'].ptr, d_x_next=outs['x_next'].ptr, d_action=outs['action'].ptr, d_reward=outs['reward'].ptr,
                            d_goal_achieved=outs['goal_achieved'].ptr, d_index=outs['index'].ptr)
        batch = {k: outs[k].read(specs[k][0]).reshape(specs[k][1]) for k in specs}
        assert batch['goal_achieved'].any() and not batch['goal_achieved'].all(), 'the batch holds terminal and other samples'

        def snapshot():
            packed = dev.get(h.device_ptr(PMG_BUF_PACKED), (N, P), np.uint32)
            derived = [np.concatenate([v for k, v in sorted(h.norm_read(w).items()) if k in ('mean', 'std', 'inv_std')]) for w in NC.KINDS]
            return NC.all_totals(h) + derived + [packed, h.get_state(), h.get_rng()] + [outs[k].read(np.uint8) for k in specs]
        before = snapshot()
        y, qn, na, q = Out(dev, 4 * B), Out(dev, 4 * B), Out(dev, 4 * B * A), Out(dev, 4 * B)
        env.critic.td_target_device(env.actor, outs['x_next'].ptr, outs['reward'].ptr, y.ptr, gamma, lo, hi, d_terminal=outs['goal_achieved'].ptr,
                                    d_q_next=qn.ptr, d_next_action=na.ptr, batch=B)
        env.critic.q_device(outs['x'].ptr, Dx, outs['action'].ptr, A, B, q.ptr)
        got = {'y': y.read(), 'q': qn.read(), 'a': na.read().reshape(B, A)}
        got_q = q.read()
        after = snapshot()
    m = td_model(batch['x_next'], batch['reward'], Wa, ba, Wc, bc, gamma, lo, hi, batch['goal_achieved'])
    check_td(got, m, 'sampler batch')
    eq_bits(got_q, q_model(batch['x'], batch['action'], Wc, bc), 'q of the sampled (x, action)')
    for a, b in zip(before, after):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    env.close()


# 8. invalid calls
def case_invalid_calls(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B = 6, 3, 8
        Wa, ba = network(81, (Dx, 16, A))
        Wc, bc = network(82, (Dx + A, 16, 1))
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        with Dev(h) as dev:
            actor, critic = Net(h, dev, Wa, ba, 1), Net(h, dev, Wc, bc, 0)
            wide, two = Net(h, dev, *network(83, (Dx + A + 1, 16, 1))), Net(h, dev, *network(84, (Dx + A, 16, 2)))
            big_actor, big_critic = Net(h, dev, *network(85, (254, 3))), Net(h, dev, *network(86, (256, 1)))      # Dx + A = 257
            d_x, d_a, d_r = dev.put(np.zeros((B, 254), F32)), dev.put(np.zeros((B, A), F32)), dev.put(np.zeros(B, F32))
            d_t = dev.put(np.zeros(B + 1, np.uint8))
            outs = [dev.put(np.full(4 * B * A, SENTINEL, np.uint8)) for _ in range(4)]

            def mlp(net, **kw):
                m = h.mlp_struct(net.widths, net.d_w, net.d_b, 0)
                for k, v in kw.items():
                    if k in ('width', 'd_weight', 'd_bias'):
                        getattr(m, k)[v[0]] = v[1]
                    else:
                        setattr(m, k, v)
                return m

            def q(m=None, d_x=d_x, x_stride=Dx, x_dim=Dx, d_a=d_a, a_stride=A, a_dim=A, batch=B, d_q=outs[0], q_stride=1):
                return h.L.lib.pmg_q_device(h.h, C.byref(m or mlp(critic)), vp(d_x), i64(x_stride), i32(x_dim), vp(d_a), i64(a_stride), i32(a_dim), i64(batch),
                                            vp(d_q), i64(q_stride))

            def td(am=None, cm=None, null_td=False, **kw):
                a = dict(batch=B, d_x_next=d_x, x_stride=Dx, d_reward=d_r, d_y=outs[1], gamma=0.98, clip_lo=-50.0, clip_hi=0.0, d_terminal=d_t + 1,
                         d_q_next=outs[2], d_next_action=outs[3])
                size = kw.pop('struct_size', None)
                a.update(kw)
                s = h.td_struct(**a)
                if size is not None:
                    s.struct_size = size
                return h.L.lib.pmg_td_target_device(h.h, C.byref(am or mlp(actor)), C.byref(cm or mlp(critic)), None if null_td else C.byref(s))
            def bad_nets(net):
                return [mlp(net, **kw) for kw in (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                                  dict(width=(1, 0)), dict(d_weight=(0, None)), dict(out_activation=2), dict(d_weight=(1, net.d_w[1] + 2)))]
            nan = float('nan')
            bad = [lambda m=m: q(m) for m in bad_nets(critic)] + [lambda m=m: td(cm=m) for m in bad_nets(critic)] + [lambda m=m: td(am=m) for m in bad_nets(actor)] + [
                lambda: q(mlp(wide)), lambda: q(mlp(two)), lambda: q(x_dim=Dx - 1), lambda: q(a_dim=A + 1), lambda: q(x_dim=0, a_dim=Dx + A),
                lambda: q(x_dim=Dx + A, a_dim=0), lambda: q(x_dim=Dx + A + 1, a_dim=-1), lambda: q(d_x=None), lambda: q(d_a=None), lambda: q(d_q=None),
                lambda: q(d_x=d_x + 2), lambda: q(d_a=d_a + 1), lambda: q(d_q=outs[0] + 2), lambda: q(x_stride=Dx - 1), lambda: q(a_stride=A - 1),
                lambda: q(q_stride=0), lambda: q(batch=-1), lambda: q(mlp(big_critic), x_dim=254, x_stride=254, a_dim=3),
                lambda: td(cm=mlp(wide)), lambda: td(cm=mlp(two)), lambda: td(am=mlp(big_actor), cm=mlp(big_critic), x_stride=254),
                lambda: td(null_td=True), lambda: td(struct_size=C.sizeof(PmgTdTarget) - 8), lambda: td(struct_size=0),
                lambda: td(d_x_next=None), lambda: td(d_reward=None), lambda: td(d_y=None),
                lambda: td(d_x_next=d_x + 2), lambda: td(d_reward=d_r + 1), lambda: td(d_y=outs[1] + 2), lambda: td(d_q_next=outs[2] + 1),
                lambda: td(d_next_action=outs[3] + 3), lambda: td(x_stride=Dx - 1), lambda: td(batch=-1),
                lambda: td(gamma=-0.1), lambda: td(gamma=INF), lambda: td(gamma=nan),
                lambda: td(clip_lo=0.0, clip_hi=-1.0), lambda: td(clip_lo=nan), lambda: td(clip_hi=nan), lambda: td(clip_lo=nan, clip_hi=nan)]
            assert h.L.lib.pmg_q_device(h.h, None, vp(d_x), i64(Dx), i32(Dx), vp(d_a), i64(A), i32(A), i64(B), vp(outs[0]), i64(1)) == E_INVALID
            good = h.td_struct(B, d_x, Dx, d_r, outs[1], 0.98)
            assert h.L.lib.pmg_td_target_device(h.h, None, C.byref(mlp(critic)), C.byref(good)) == E_INVALID
            assert h.L.lib.pmg_td_target_device(h.h, C.byref(mlp(actor)), None, C.byref(good)) == E_INVALID
            for k, call in enumerate(bad):
                assert call() == E_INVALID, k
                assert h.L.error(h.h), k
            h.sync()
            for o in outs:
                assert (dev.get(o, 4 * B * A, np.uint8) == SENTINEL).all()
            assert q(batch=0) == 0 and td(batch=0) == 0
            h.sync()
            for o in outs:
                assert (dev.get(o, 4 * B * A, np.uint8) == SENTINEL).all()
            # what is allowed: an odd d_terminal, no d_terminal, infinite and equal clips
            assert td() == 0 and td(d_terminal=None, clip_lo=-INF, clip_hi=INF) == 0 and td(clip_lo=-1.0, clip_hi=-1.0, d_q_next=None, d_next_action=None) == 0
            assert q() == 0
            h.sync()
            assert (dev.get(outs[1], 4 * B, np.uint8).view(F32) == -1).all()


# 9. host face
def case_host_face(library):
    import pytest
    env = AC.stepped(library, 'reach', 8)
    Dx, A = 6, 3
    Wa, ba = network(91, (Dx, 64, A))
    Wc, bc = network(92, (Dx + A, 64, 1))
    critic, actor = env.critic, env.actor
    assert critic is env.critic
    rs = np.random.RandomState(93)
    x, a = rs.uniform(-2, 2, (5, 7, Dx)).astype(F32), rs.uniform(-1, 1, (5, 7, A)).astype(F32)
    with pytest.raises(ValueError):
        critic.q(x, a)                                       # nothing loaded
    for args in (([Wc[0], Wc[1][:, :-1]], bc), (Wc, bc[:1]), ([], []), ([Wc[0]] * 5, None), ([np.zeros((257, 3), F32)], None), ([Wc[0][0]], None),
                 ([Wc[0]], [bc[0]]), (network(94, (Dx + A, 64, 2))), (Wc, [bc[0][:-1], bc[1]])):
        with pytest.raises(ValueError):
            critic.load(*args)
    with pytest.raises(ValueError):
        critic.load(Wc, bc, out_activation='relu')
    critic.load(Wc, bc)
    assert critic.widths == [Dx + A, 64, 1]
    got = critic.q(x, a)
    assert got.shape == (5, 7)
    eq_bits(got.reshape(35), q_model(x.reshape(35, Dx), a.reshape(35, A), Wc, bc), 'q')
    assert critic.q(x[:0], a[:0]).shape == (0, 7)
    for bad in ((x, a[:4]), (x[..., :-1], a), (x, a[..., :-1]), (x, np.zeros((5, 7, 0), F32))):
        with pytest.raises(ValueError):
            critic.q(*bad)
    xn, r = rs.uniform(-2, 2, (37, Dx)).astype(F32), -rs.randint(0, 2, 37).astype(F32)
    term = rs.randint(0, 2, 37).astype(bool)
    with pytest.raises(ValueError):
        critic.td_target(actor, xn, r, 0.98)                 # no target actor loaded
    actor.load(Wa, ba, out_activation='identity')
    for kw in ({}, {'clip_lo': -50.0, 'clip_hi': 0.0}, {'terminal': term}, {'clip_lo': -50.0, 'clip_hi': 0.0, 'terminal': term}):
        y, qn, na = critic.td_target(actor, xn, r, 0.98, **kw)
        m = td_model(xn, r, Wa, ba, Wc, bc, 0.98, kw.get('clip_lo', -INF), kw.get('clip_hi', INF), kw.get('terminal'))
        check_td({'y': y, 'q': qn, 'a': na}, m, kw)
    y, qn, na = critic.td_target(actor, xn[:0], r[:0], 0.98)
    assert y.shape == (0,) and qn.shape == (0,) and na.shape == (0, A)
    for args, kw in (((actor, xn[:, :-1], r, 0.98), {}), ((actor, xn, r[:-1], 0.98), {}), ((actor, xn, r, -1.0), {}), ((actor, xn, r, INF), {}),
                     ((actor, xn, r, 0.98), {'clip_lo': 1.0, 'clip_hi': 0.0}), ((actor, xn, r, 0.98), {'clip_lo': float('nan')}),
                     ((actor, xn, r, 0.98), {'terminal': term[:-1]}), ((critic, xn, r, 0.98), {})):
        with pytest.raises(ValueError):
            critic.td_target(*args, **kw)
    actor.load(*network(95, (Dx + 1, 8, A)))                 # an actor the critic does not fit
    with pytest.raises(ValueError):
        critic.td_target(actor, np.zeros((2, Dx + 1), F32), np.zeros(2, F32), 0.98)
    assert len(critic._ptrs) == 4
    critic.close()
    with pytest.raises(ValueError):
        critic.q(x, a)
    with pytest.raises(ValueError):
        critic.td_target(actor, xn, r, 0.98)
    critic.load(Wc, bc)                                      # a closed critic can be loaded again; env.close() frees it
    env.close()
    assert critic._mlp is None and critic._ptrs == []
