"""The cases of the TD3-target tests (include/pmg.h pmg_td3_target_device) and their numpy model, shared by four files:
tests/test_td3_emulated.py runs them on the g++ build of the product sources over the fiber emulator, tests/test_gpu_td3.py on libpmg_hip.so
on the MI355X, tests/test_td3_host.py covers the model alone and the numpy face, tests/test_td3_wave_order.py the kernel under permuted
wavefront order.  The pieces are those of tests/td_cases.py and tests/actor_cases.py: the exact float32 fmaf chain, the clip, the epilogue,
the integer draws.  Every case takes the loaded library and goes through the C ABI with buffers from pmg_device_alloc.

Bars.  Everything but the smoothing term is min / max / fmaf on float32 chains: bit for bit, the sign of a zero y left open (td_cases.eq_y).
The smoothing term goes through the build's logf / sqrtf / cosf (and tanhf for a tanh actor): a~ is held to the float64 model of the same
expression, evaluated from the model's bit-exact z and the integer draws, within actor_cases.ACTION_TOL -- the project's bar for this very
expression at noise_eps = 0.2, so the cases use sigma = 0.2 (SIGMA) and c = 0.5 (NOISE_CLIP); q1, q2, q_min and y are then bit-equal to
pmg_q_device and the epilogue evaluated from the DEVICE's own a~ (DESIGN.md 3.10's rule)."""
import ctypes as C

import numpy as np

import actor_cases as AC
import td_cases as TC
from actor_cases import ACTION_TOL, Net, bits, explore_draws, fmaf, forward, network
from normalizer_cases import SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PmgMlp, PmgTd3Target
from td_cases import BATCHES, INF, Out, clip1, eq_bits, eq_y, epilogue, put_rows, q_model

E_INVALID = -1
F32 = np.float32
TILE = AC.TILE
SIGMA, NOISE_CLIP = 0.2, 0.5
PAIRS = ((6, 3), (1, 1), (2, 5), (3, 12), (29, 4))
HIDDEN = ((), (33,), (256, 256, 256))
OUTPUTS = ('y', 'qmin', 'q1', 'q2', 'a')
TWO_PI32 = F32(6.28318530717958647692)


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def draws(seed, counter, row_offset, B, A):
    """u1, u2 [B, A] float64 (exact float32 values) of the rows row_offset ... row_offset + B - 1: sample index (row_offset + b) * A + j"""
    u1, u2, _, _ = explore_draws(seed, counter, np.arange(B, dtype=np.uint64) + np.uint64(row_offset), A, 0.0)
    return u1, u2


def noise32(u1, u2, sigma, c):
    """e in float32, the normative order: clip((sigma * sqrt(-2 ln u1)) * cos(2 pi u2), -c, c); numpy's float32 functions stand in for the build's"""
    u1, u2 = u1.astype(F32), u2.astype(F32)
    return np.minimum(np.maximum(F32(sigma) * np.sqrt(F32(-2) * np.log(u1)) * np.cos(TWO_PI32 * u2), F32(-c)), F32(c))


def noise64(u1, u2, sigma, c):
    """e in float64 from the integer draws"""
    return np.clip(float(F32(sigma)) * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2), -float(F32(c)), float(F32(c)))


def smooth64(z, out_act, u1, u2, sigma, c):
    """the float64 model of a~ from pre-activations and draws"""
    a0 = np.clip(np.tanh(z.astype(np.float64)) if out_act else z.astype(np.float64), -1.0, 1.0)
    return np.clip(a0 + noise64(u1, u2, sigma, c), -1.0, 1.0) if sigma > 0 else a0


def td3_model(x, r, Wa, ba, W1, b1, W2=None, b2=None, gamma=0.98, lo=-INF, hi=INF, term=None, sigma=0.0, c=INF, seed=0, counter=0, row_offset=0, a=None):
    """-> dict(z, a0, a, q1, q2, qmin, t, y) of an identity-output actor and identity critics, or from the given a~ (the device's own)"""
    z = forward(x, Wa, ba)
    a0 = clip1(z)
    if a is None:
        a = a0
        if sigma > 0:
            u1, u2 = draws(seed, counter, row_offset, x.shape[0], a0.shape[1])
            a = clip1(a0 + noise32(u1, u2, sigma, c))
    q1 = q_model(x, a, W1, b1)
    q2 = q_model(x, a, W2, b2) if W2 is not None else None
    qmin = np.minimum(q1, q2) if q2 is not None else q1
    t, y = epilogue(qmin, r, gamma, lo, hi, term)
    return {'z': z, 'a0': a0, 'a': a, 'q1': q1, 'q2': q2, 'qmin': qmin, 't': t, 'y': y}


def clipped_normal_moments(k):
    """mean 0; second and fourth moment of min(max(n, -k), k), n ~ N(0, 1), and P(|n| >= k): the density on a fine grid plus the two atoms"""
    from math import erfc, sqrt
    g = np.linspace(-k, k, 400001)
    pdf = np.exp(-0.5 * g * g) / np.sqrt(2 * np.pi)
    tail = erfc(k / sqrt(2.0))                                  # both tails
    trap = lambda f: float(((f[1:] + f[:-1]) * 0.5 * np.diff(g)).sum())
    return trap(g ** 2 * pdf) + tail * k ** 2, trap(g ** 4 * pdf) + tail * k ** 4, tail


def model_vs_float64(seed, B=101, Dx=6, A=3):
    """the float32 model against float64 torch of the same formula fed the model's own n -> (largest |y32 - y64| / max |y64|, predicates equal)"""
    import torch
    gamma, lo, hi = 0.98, -50.0, 0.0
    Wa, ba = network(seed, (Dx, 33, A))
    W1, b1 = network(seed + 1, (Dx + A, 64, 33, 1))
    W2, b2 = network(seed + 2, (Dx + A, 33, 1))
    rs = np.random.RandomState(seed + 3)
    x, r = rs.uniform(-2, 2, (B, Dx)).astype(F32), -rs.randint(0, 2, B).astype(F32)
    scale = F32(2.0 ** np.floor(np.log2(1.5 / np.abs(forward(x, Wa, ba)).max())))
    Wa[-1], ba[-1] = Wa[-1] * scale, ba[-1] * scale               # |z| up to about 1.5, as td_cases.td_case
    base = td3_model(x, r, Wa, ba, W1, b1, W2, b2, gamma)
    for k, (W, b) in enumerate(((W1, b1), (W2, b2))):
        scale = F32(2.0 ** np.ceil(np.log2(100.0 / np.abs(base['q%d' % (k + 1)]).max())))
        W[-1], b[-1] = W[-1] * scale, b[-1] * scale               # |q| up to 100 .. 200: t on both sides of both clips of [-50, 0]
    term = (rs.uniform(0, 1, B) < 0.2).astype(np.uint8)
    m = td3_model(x, r, Wa, ba, W1, b1, W2, b2, gamma, lo, hi, term, SIGMA, NOISE_CLIP, seed, 1, 7)
    u1, u2 = draws(seed, 1, 7, B, A)
    u1, u2 = u1.astype(F32), u2.astype(F32)
    n = np.sqrt(F32(-2) * np.log(u1)) * np.cos(TWO_PI32 * u2)   # the model's own n, float32
    t64 = lambda v: torch.tensor(np.asarray(v, np.float64))

    def net64(h, Ws, bs):
        for l, (W, b) in enumerate(zip(Ws, bs)):
            h = h @ t64(W).T + t64(b)
            if l + 1 < len(Ws):
                h = torch.relu(h)
        return h
    z = net64(t64(x), Wa, ba)
    a0 = torch.clamp(z, -1.0, 1.0)
    s = float(F32(SIGMA)) * t64(n)
    e = torch.clamp(s, -NOISE_CLIP, NOISE_CLIP)
    a = torch.clamp(a0 + e, -1.0, 1.0)
    xa = torch.cat([t64(x), a], 1)
    q1, q2 = net64(xa, W1, b1)[:, 0], net64(xa, W2, b2)[:, 0]
    qmin = torch.minimum(q1, q2)
    t = torch.where(t64(term) != 0, t64(r), gamma * qmin + t64(r))
    y = torch.clamp(t, lo, hi).numpy()
    s32 = F32(SIGMA) * n
    sums32 = m['a0'] + noise32(u1, u2, SIGMA, NOISE_CLIP)
    same = all(np.array_equal(p, q.numpy() if hasattr(q, 'numpy') else q) for p, q in (
        (m['z'] > 1, z > 1), (m['z'] < -1, z < -1), (s32 > F32(NOISE_CLIP), s > NOISE_CLIP), (s32 < F32(-NOISE_CLIP), s < -NOISE_CLIP),
        (sums32 > 1, a0 + e > 1), (sums32 < -1, a0 + e < -1), (m['q2'] < m['q1'], q2 < q1), (m['t'] < F32(lo), t < lo), (m['t'] > F32(hi), t > hi)))
    used = bool((np.abs(m['z']) > 1).any() and (np.abs(s32) > F32(NOISE_CLIP)).any() and (np.abs(sums32) > 1).any() and (m['q2'] < m['q1']).any()
                and (m['q1'] < m['q2']).any() and (m['t'] < F32(lo)).any() and (m['t'] > F32(hi)).any())
    return float(np.abs(m['y'].astype(np.float64) - y).max() / np.abs(y).max()), same, used


# ----------------------------------------------------------------------------------------------------------------------
# device calls
def device_td3(h, Wa, ba, W1, b1, W2=None, b2=None, x=None, r=None, gamma=0.98, lo=-INF, hi=INF, term=None, sigma=0.0, c=INF, seed=0, counter=0,
               row_offset=0, act_out=0, c1_out=0, c2_out=0, x_pad=0, shift=0, null=()):
    """pmg_td3_target_device on canary-framed buffers -> dict(y, qmin, q1, q2, a) (None for an output passed as NULL).  The workspace is
    canary-framed and sized exactly pmg_td3_target_work_floats (NULL where that is 0).  shift: floats off the 16-byte boundary for every
    float pointer; d_terminal sits at an odd address."""
    B, A = x.shape[0], Wa[-1].shape[0]
    with Dev(h) as dev:
        actor, c1 = Net(h, dev, Wa, ba, act_out), Net(h, dev, W1, b1, c1_out)
        c2 = Net(h, dev, W2, b2, c2_out) if W2 is not None else None
        d_x, xs = put_rows(h, dev, x, x_pad, shift)
        d_r, _ = put_rows(h, dev, np.asarray(r, F32)[None, :], 0, (shift + 1) & 3)
        d_t = None
        if term is not None:
            d_t = dev.alloc(B + 32)
            d_t += (-d_t) % 16 + 1
            h.upload(d_t, np.ascontiguousarray(term, np.uint8))
        outs = {k: Out(dev, 4 * B * (A if k == 'a' else 1), 4 * ((shift + n) & 3)) for n, k in enumerate(OUTPUTS)}
        ptr = lambda k: None if k in null else outs[k].ptr
        need = h.td3_target_work_floats(actor.mlp, c2 is not None, 'a' not in null, B)
        assert need == (B * A if c2 is not None and 'a' in null else 0)
        work = Out(dev, 4 * need, 4 * ((shift + 1) & 3)) if need else None
        td = h.td3_struct(B, d_x, xs, d_r, outs['y'].ptr, gamma, lo, hi, sigma, c, seed, counter, row_offset, d_t, ptr('qmin'), ptr('q1'), ptr('q2'), ptr('a'),
                          work.ptr if work else None, need)
        h.td3_target_device(actor.mlp, c1.mlp, c2.mlp if c2 is not None else None, td)
        res = {k: o.read(written=k not in null and not (k == 'q2' and c2 is None)) for k, o in outs.items()}
        if work:
            work.read()
    if res['a'] is not None:
        res['a'] = res['a'].reshape(B, A)
    return res


def device_qs(h, W1, b1, W2, b2, x, a, c1_out=0, c2_out=0):
    """pmg_q_device of each critic on (x, a) -> q1, q2"""
    with Dev(h) as dev:
        out = []
        d_x, d_a = dev.put(x), dev.put(a)
        for W, b, act in ((W1, b1, c1_out), (W2, b2, c2_out)):
            if W is None:
                out.append(None)
                continue
            net = Net(h, dev, W, b, act)
            d_q = dev.alloc(4 * x.shape[0])
            h.q_device(net.mlp, d_x, x.shape[1], x.shape[1], d_a, a.shape[1], a.shape[1], x.shape[0], d_q)
            out.append(dev.get(d_q, x.shape[0], F32))
    return out


def check_from_own_action(h, got, nets, x, r, gamma, lo, hi, term, label, c1_out=0, c2_out=0):
    """q1, q2 bit for bit pmg_q_device on the call's own a~; q_min and y the epilogue on np.minimum of them"""
    W1, b1, W2, b2 = nets
    q1, q2 = device_qs(h, W1, b1, W2, b2, x, got['a'], c1_out, c2_out)
    eq_bits(got['q1'], q1, (label, 'q1'))
    if q2 is not None:
        eq_bits(got['q2'], q2, (label, 'q2'))
    qmin = np.minimum(q1, q2) if q2 is not None else q1
    eq_bits(got['qmin'] + F32(0), qmin + F32(0), (label, 'qmin'))
    eq_y(got['y'], epilogue(qmin, r, gamma, lo, hi, term)[1], (label, 'y'))


def critics(seed, Dx, A, h1=(33,), h2=(64, 33)):
    W1, b1 = network(seed, (Dx + A,) + tuple(h1) + (1,))
    W2, b2 = network(seed + 1, (Dx + A,) + tuple(h2) + (1,))
    return W1, b1, W2, b2


def actor_case(Dx, A, hidden, B):
    """an actor with |z| up to about 1.5 (the clip shows, most actions are off it), rows and rewards"""
    def make():
        Wa, ba = network(900 + 13 * Dx + A + len(hidden), (Dx,) + tuple(hidden) + (A,))
        rs = np.random.RandomState(Dx * 19 + A + B)
        x = rs.uniform(-2, 2, (B, Dx)).astype(F32)
        r = -rs.randint(0, 2, B).astype(F32)
        scale = F32(2.0 ** np.floor(np.log2(1.5 / np.abs(forward(x, Wa, ba)).max())))
        Wa[-1], ba[-1] = Wa[-1] * scale, ba[-1] * scale
        return {'Wa': Wa, 'ba': ba, 'x': x, 'r': r, 'z': forward(x, Wa, ba)}
    return TC.cached(('td3 actor', Dx, A, tuple(hidden), B), make)


# ----------------------------------------------------------------------------------------------------------------------
# 2. one critic, no noise: the bits of pmg_td_target_device
def case_degenerate(library, hidden, pairs=PAIRS):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        n = HIDDEN.index(hidden)
        for Dx, A in pairs:
            n += 1
            for B in BATCHES:
                m = actor_case(Dx, A, hidden, BATCHES[-1])
                x, r = m['x'][:B], m['r'][:B]
                W1, b1 = network(950 + Dx + A, (Dx + A,) + ((256, 33) if len(hidden) > 1 else (33,)) + (1,))
                for act in (0, 1):
                    kw = dict(gamma=0.98, lo=-50.0, hi=0.0, act_out=act, x_pad=(n + B) % 3, shift=(n + B) % 4)
                    old = TC.device_td(h, m['Wa'], m['ba'], W1, b1, x, r, 0.98, -50.0, 0.0, act_out=act, x_pad=kw['x_pad'], shift=kw['shift'])
                    got = device_td3(h, m['Wa'], m['ba'], W1, b1, None, None, x, r, sigma=0.0, c=0.5, seed=5, counter=n, row_offset=B, **kw)
                    for k, k_old in (('y', 'y'), ('q1', 'q'), ('qmin', 'q'), ('a', 'a')):
                        eq_bits(got[k], old[k_old], (Dx, A, hidden, B, act, k))
                    assert got['q2'] is None


# 3. twin critics, no noise
def case_twin(library):
    relations = set()
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        shapes = (((6, 3), (33,), (33,), (64, 33), 0, 0), ((29, 4), (256, 256, 256), (256,), (33, 255, 31), 0, 0), ((3, 12), (), (256, 256, 256), (), 0, 0),
                  ((2, 5), (33,), (), (256, 33), 1, 1), ((1, 1), (256, 256, 256), (33, 33), (33,), 0, 1))
        for n, ((Dx, A), ah, h1, h2, o1, o2) in enumerate(shapes):
            B = BATCHES[(n + 1) % len(BATCHES)]                  # the steep pair runs on 101 rows
            m = actor_case(Dx, A, ah, BATCHES[-1])
            x, r = m['x'][:B], m['r'][:B]
            nets = critics(1000 + 10 * n, Dx, A, h1, h2)
            if o1 and o2:                                        # both tanh and steep: rows where both saturate at the same +-1
                for W, b in ((nets[0], nets[1]), (nets[2], nets[3])):
                    W[-1], b[-1] = W[-1] * F32(8), b[-1] * F32(8)
            gamma, lo, hi = 0.98, -50.0, 0.0
            rs = np.random.RandomState(n)
            term = (rs.uniform(0, 1, B) < 0.3).astype(np.uint8)
            nulls = [(), ('a',), ('qmin',), ('q1',), ('q2',), ('qmin', 'q1', 'q2', 'a')] if n < 2 else [(), ('a',)]
            full = None
            for k, null in enumerate(nulls):
                got = device_td3(h, m['Wa'], m['ba'], *nets, x, r, gamma, lo, hi, term, c1_out=o1, c2_out=o2, x_pad=(n + k) % 3, shift=(n + k) % 4, null=null)
                if full is None:
                    full = got
                    eq_bits(got['a'], clip1(m['z'][:B]), (n, 'a'))
                    check_from_own_action(h, got, nets, x, r, gamma, lo, hi, term, n, o1, o2)
                    if not (o1 or o2):
                        want = td3_model(x, r, m['Wa'], m['ba'], *nets, gamma, lo, hi, term)
                        for key in ('q1', 'q2'):
                            eq_bits(got[key], want[key], (n, key, 'model'))
                        eq_y(got['y'], want['y'], (n, 'y', 'model'))
                    q1, q2 = got['q1'], got['q2']
                    relations |= {s for s, hit in (('<', q1 < q2), ('>', q1 > q2), ('=', q1 == q2)) if hit.any()}
                else:
                    for key in OUTPUTS:
                        if got[key] is not None:
                            eq_bits(got[key], full[key], (n, null, key))
    assert relations == {'<', '>', '='}, relations


# 4. smoothing
def case_smoothing(library):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        gamma, lo, hi = 0.98, -50.0, 0.0
        for n, ((Dx, A), ah, act) in enumerate((((6, 3), (33,), 0), ((3, 12), (256, 256, 256), 1), ((29, 4), (), 0), ((2, 5), (33,), 1))):
            B = (101, 33, 32, 31)[n]
            m = actor_case(Dx, A, ah, BATCHES[-1])
            x, r = m['x'][:B], m['r'][:B]
            nets = critics(1100 + 10 * n, Dx, A)
            seed, counter, off = 11 + n, 2 ** 40 + n, (0, 5, 2 ** 33, 1)[n]
            for null in ((), ('a',)) if n == 0 else ((),):
                got = device_td3(h, m['Wa'], m['ba'], *nets, x, r, gamma, lo, hi, None, SIGMA, NOISE_CLIP, seed, counter, off, act_out=act, x_pad=n % 3, shift=n,
                                 null=null)
                if null:
                    for key in ('y', 'qmin', 'q1', 'q2'):
                        eq_bits(got[key], full[key], (n, 'workspace path', key))
                    continue
                full = got
                u1, u2 = draws(seed, counter, off, B, A)
                a64 = smooth64(m['z'][:B], act, u1, u2, SIGMA, NOISE_CLIP)
                err = float(np.abs(got['a'] - a64).max())
                worst = max(worst, err)
                assert err <= ACTION_TOL, (n, err)
                assert (np.abs(got['a']) <= 1).all() and (np.abs(got['a'] - smooth64(m['z'][:B], act, u1, u2, 0.0, 0.0)).max() > 0.1)
                check_from_own_action(h, got, nets, x, r, gamma, lo, hi, None, n)
                # one critic sees the same smoothed action
                one = device_td3(h, m['Wa'], m['ba'], nets[0], nets[1], None, None, x, r, gamma, lo, hi, None, SIGMA, NOISE_CLIP, seed, counter, off, act_out=act)
                eq_bits(one['a'], got['a'], (n, 'one critic, a'))
                eq_bits(one['q1'], got['q1'], (n, 'one critic, q1'))
                eq_bits(one['qmin'], got['q1'], (n, 'one critic, qmin'))
        # c = 0: a~ == a0 bit for bit; c = inf with a large sigma: saturated at +-1
        m = actor_case(6, 3, (33,), BATCHES[-1])
        nets = critics(1100, 6, 3)
        plain = device_td3(h, m['Wa'], m['ba'], *nets, m['x'], m['r'], gamma, lo, hi, act_out=1)
        zero = device_td3(h, m['Wa'], m['ba'], *nets, m['x'], m['r'], gamma, lo, hi, None, SIGMA, 0.0, 1, 2, 3, act_out=1)
        for key in OUTPUTS:
            eq_bits(zero[key], plain[key], ('c = 0', key))
        sat = device_td3(h, m['Wa'], m['ba'], *nets, m['x'], m['r'], gamma, lo, hi, None, 1e6, INF, 1, 2, 3, act_out=1)
        assert (np.abs(sat['a']) == 1).all() and (sat['a'] == 1).any() and (sat['a'] == -1).any()
        check_from_own_action(h, sat, nets, m['x'], m['r'], gamma, lo, hi, None, 'saturated')
        # row_offset: rows [40, 101) of the batch are a call on those rows with row_offset = 40; another counter changes a~
        whole = device_td3(h, m['Wa'], m['ba'], *nets, m['x'], m['r'], gamma, lo, hi, None, SIGMA, NOISE_CLIP, 7, 8, 0)
        part = device_td3(h, m['Wa'], m['ba'], *nets, m['x'][40:], m['r'][40:], gamma, lo, hi, None, SIGMA, NOISE_CLIP, 7, 8, 40, x_pad=1, shift=1)
        for key in OUTPUTS:
            eq_bits(part[key], whole[key][40:], ('row_offset', key))
        again = device_td3(h, m['Wa'], m['ba'], *nets, m['x'], m['r'], gamma, lo, hi, None, SIGMA, NOISE_CLIP, 7, 8, 0, null=('a',))
        for key in ('y', 'qmin', 'q1', 'q2'):
            eq_bits(again[key], whole[key], ('twice', key))
        other = device_td3(h, m['Wa'], m['ba'], *nets, m['x'], m['r'], gamma, lo, hi, None, SIGMA, NOISE_CLIP, 7, 9, 0)
        shifted = device_td3(h, m['Wa'], m['ba'], *nets, m['x'], m['r'], gamma, lo, hi, None, SIGMA, NOISE_CLIP, 7, 8, 1)
        assert (other['a'] != whole['a']).mean() > 0.9 and (shifted['a'] != whole['a']).mean() > 0.9
    print('smoothing: largest |a~ - a64| = %.3g (bar %.3g)' % (worst, ACTION_TOL))
    return worst


# 5. stale tile contents
def stale_critics(regime, B):
    """critic 1 -> critic 2 on Dx = 29, A = 4 (Dx + A = 33 is odd: critic 2's layer 0 multiplies column 33 of the tile by its stand-in zero),
    on the rows and the actor of td_cases.stale_case.  Critic 1's first hidden layer of 256 units leaves that column (and every column from
    32 on) huge or inf, as the actor's does there:
      'huge': 33 -> 256 -> 1, hidden weights 1e30 on x in [0.5, 2) (activations of some 1e31), last layer 1e-38;
      'inf':  33 -> 256 -> 32 -> 1, hidden weights 1e30 on x of 1e9 (inf); the layer that reads the infs has negative weights (ReLU: +0.0), so
              q1 is critic 1's last bias, and that layer writes columns 0..31 only: columns 32..255 keep the infs."""
    def make():
        m = TC.stale_case(regime, B)
        rs = np.random.RandomState(190 + B)
        Dx, A = 29, 4
        if regime == 'huge':
            W1 = [np.full((256, Dx + A), 1e30, F32), (rs.uniform(0.5, 1, (1, 256)) * 1e-38).astype(F32)]
            b1 = [None, np.array([-0.25], F32)]
        else:
            W1 = [np.full((256, Dx + A), 1e30, F32), -rs.uniform(0.5, 1, (32, 256)).astype(F32), rs.uniform(-1, 1, (1, 32)).astype(F32)]
            b1 = [None, None, np.array([-0.25], F32)]
        W2, b2 = network(195, (Dx + A, 33, 1))
        W2[0] = (W2[0] * (1.0 if regime == 'huge' else 1e-9)).astype(F32)
        b2[-1] = b2[-1] - F32(0.25) - F32(np.median(q_model(m['x'], m['a'], W2, b2)))      # q2 on both sides of q1
        with np.errstate(over='ignore', invalid='ignore'):
            hid = np.maximum(forward(np.concatenate([m['x'], m['a']], 1), W1[:1], None), 0)
            t = td3_model(m['x'], m['r'], m['Wa'], m['ba'], W1, b1, W2, b2, 0.98)
        assert (np.isinf(hid).all() if regime == 'inf' else (np.isfinite(hid).all() and hid.min() > 1e30))
        assert all(np.isfinite(t[k]).all() for k in ('y', 'q1', 'q2')) and (t['q2'] < t['q1']).any() and (t['q1'] < t['q2']).any()
        return dict(t, Wa=m['Wa'], ba=m['ba'], W1=W1, b1=b1, W2=W2, b2=b2, x=m['x'], r=m['r'])
    return TC.cached(('td3 stale', regime, B), make)


def run_stale(h, m, sl=slice(None), **kw):
    return device_td3(h, m['Wa'], m['ba'], m['W1'], m['b1'], m['W2'], m['b2'], m['x'][sl], m['r'][sl], 0.98, **kw)


def check_td3(got, want, label):
    eq_y(got['y'], want['y'], (label, 'y'))
    for k in ('q1', 'q2', 'a'):
        if got[k] is not None:
            eq_bits(got[k], want[k], (label, k))
    if got['qmin'] is not None:
        eq_bits(got['qmin'] + F32(0), want['qmin'] + F32(0), (label, 'qmin'))


def case_stale_tile(library):
    B = TILE + 1                                                 # row 32 sits in a tile with 31 rows past the batch
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for regime in ('huge', 'inf'):
            # actor -> critic 1: td_cases' regimes, with a second critic behind
            m = TC.stale_case(regime, B)
            W2, b2 = network(196, (33, 64, 1))
            W2[0] = (W2[0] * (1.0 if regime == 'huge' else 1e-9)).astype(F32)
            want = td3_model(m['x'], m['r'], m['Wa'], m['ba'], m['Wc'], m['bc'], W2, b2, 0.98)
            got = device_td3(h, m['Wa'], m['ba'], m['Wc'], m['bc'], W2, b2, m['x'], m['r'], 0.98, x_pad=1)
            assert all(np.isfinite(got[k]).all() for k in OUTPUTS), regime
            check_td3(got, want, (regime, 'actor -> critic 1'))
            # critic 1 -> critic 2, through d_next_action and through the workspace
            m = stale_critics(regime, B)
            whole = run_stale(h, m, x_pad=1)
            for got, null in ((whole, ()), (run_stale(h, m, x_pad=1, null=('a',)), ('a',))):
                assert all(np.isfinite(got[k]).all() for k in OUTPUTS if got[k] is not None), (regime, null)
                check_td3(got, m, (regime, 'critic 1 -> critic 2', null))
            # alone in a batch of one, row 32 gives the same bits
            one = run_stale(h, m, slice(TILE, None))
            for k in OUTPUTS:
                eq_bits(one[k], whole[k][TILE:], (regime, 'row 32', k))


# 6. epilogue and invalid calls
def case_epilogue(library):
    gamma = 0.98
    lo, hi = -1.0 / (1.0 - gamma), 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        B, Dx, A = 101, 6, 3

        def make():
            Wa, ba = network(61, (Dx, 33, A))
            rs = np.random.RandomState(63)
            x = rs.uniform(-2, 2, (B, Dx)).astype(F32)
            r = -rs.randint(0, 2, B).astype(F32)
            nets = critics(1200, Dx, A)
            base = td3_model(x, r, Wa, ba, *nets, gamma)
            for k, (W, b) in enumerate(((nets[0], nets[1]), (nets[2], nets[3]))):
                scale = F32(2.0 ** np.ceil(np.log2(150.0 / np.abs(base['q%d' % (k + 1)]).max())))
                W[-1], b[-1] = W[-1] * scale, b[-1] * scale      # |q| up to 150 .. 300: both clips of [-50, 0] are reached
            term = (rs.uniform(0, 1, B) < 0.3).astype(np.uint8) * rs.randint(1, 256, B).astype(np.uint8)
            return dict(td3_model(x, r, Wa, ba, *nets, gamma), Wa=Wa, ba=ba, nets=nets, x=x, r=r, term=term)
        m = TC.cached(('td3 epilogue',), make)
        net = (m['Wa'], m['ba']) + tuple(m['nets']) + (m['x'], m['r'])
        qmin, r, term = m['qmin'], m['r'], m['term']
        assert (m['t'] < lo).any() and (m['t'] > hi).any() and ((m['t'] > lo) & (m['t'] < hi)).any() and term.any() and not term.all()
        assert (m['q1'] < m['q2']).any() and (m['q2'] < m['q1']).any()
        got = device_td3(h, *net, gamma)
        eq_bits(got['y'], m['t'], 'no clip')
        check_td3(got, m, 'no clip')
        got = device_td3(h, *net, gamma, lo, hi, shift=1)
        want = epilogue(qmin, r, gamma, lo, hi)[1]
        assert (want == F32(lo)).any() and (want == 0).any()
        eq_y(got['y'], want, 'clips')
        for clips in ((-INF, INF), (lo, hi), (-0.5, -0.25)):
            got = device_td3(h, *net, gamma, clips[0], clips[1], term, shift=2)
            t, y = epilogue(qmin, r, gamma, clips[0], clips[1], term)
            assert np.array_equal(t[term != 0], r[term != 0])
            eq_y(got['y'], y, ('terminal', clips))
            check_td3(got, dict(m, y=y), ('terminal', clips))
        got = device_td3(h, *net, 0.0, shift=3)
        assert np.array_equal(got['y'], r)
        # NaN loses against a number: critic 2's bias NaN -> q2 NaN, q_min = q1
        W2, b2 = [w.copy() for w in m['nets'][2]], [b.copy() for b in m['nets'][3]]
        b2[-1][:] = np.nan
        got = device_td3(h, m['Wa'], m['ba'], m['nets'][0], m['nets'][1], W2, b2, m['x'], m['r'], gamma)
        assert np.isnan(got['q2']).all()
        eq_bits(got['qmin'], m['q1'], 'NaN q2')
        eq_bits(got['y'], epilogue(m['q1'], r, gamma)[1], 'NaN q2, y')


def case_invalid_calls(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B = 6, 3, 8
        Wa, ba = network(81, (Dx, 16, A))
        vp = C.c_void_p
        with Dev(h) as dev:
            actor, c1, c2 = Net(h, dev, Wa, ba, 1), Net(h, dev, *network(82, (Dx + A, 16, 1))), Net(h, dev, *network(87, (Dx + A, 8, 8, 1)))
            wide, two = Net(h, dev, *network(83, (Dx + A + 1, 16, 1))), Net(h, dev, *network(84, (Dx + A, 16, 2)))
            big_actor, big_critic = Net(h, dev, *network(85, (254, 3))), Net(h, dev, *network(86, (256, 1)))      # Dx + A = 257
            d_x, d_r = dev.put(np.zeros((B, 254), F32)), dev.put(np.zeros(B, F32))
            d_t = dev.put(np.zeros(B + 1, np.uint8))
            outs = [dev.put(np.full(4 * B * A, SENTINEL, np.uint8)) for _ in range(6)]

            def mlp(net, **kw):
                m = h.mlp_struct(net.widths, net.d_w, net.d_b, 0)
                for k, v in kw.items():
                    if k in ('width', 'd_weight', 'd_bias'):
                        getattr(m, k)[v[0]] = v[1]
                    else:
                        setattr(m, k, v)
                return m

            def td(am=None, m1=None, m2='c2', null_td=False, **kw):
                a = dict(batch=B, d_x_next=d_x, x_stride=Dx, d_reward=d_r, d_y=outs[0], gamma=0.98, clip_lo=-50.0, clip_hi=0.0, sigma=SIGMA, noise_clip=NOISE_CLIP,
                         seed=1, counter=2, row_offset=3, d_terminal=d_t + 1, d_q_min=outs[1], d_q1=outs[2], d_q2=outs[3], d_next_action=outs[4], d_work=outs[5],
                         work_floats=B * A)
                size = kw.pop('struct_size', None)
                a.update(kw)
                s = h.td3_struct(**a)
                if size is not None:
                    s.struct_size = size
                m2 = mlp(c2) if isinstance(m2, str) else m2
                return h.L.lib.pmg_td3_target_device(h.h, C.byref(am or mlp(actor)), C.byref(m1 or mlp(c1)), C.byref(m2) if m2 is not None else None,
                                                     None if null_td else C.byref(s))

            def bad_nets(net):
                return [mlp(net, **kw) for kw in (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                                  dict(width=(1, 0)), dict(d_weight=(0, None)), dict(out_activation=2), dict(d_weight=(1, net.d_w[1] + 2)))]
            nan = float('nan')
            bad = [lambda m=m: td(am=m) for m in bad_nets(actor)] + [lambda m=m: td(m1=m) for m in bad_nets(c1)] + [lambda m=m: td(m2=m) for m in bad_nets(c2)] + [
                lambda: td(m1=mlp(wide)), lambda: td(m1=mlp(two)), lambda: td(m2=mlp(wide)), lambda: td(m2=mlp(two)),
                lambda: td(am=mlp(big_actor), m1=mlp(big_critic), m2=mlp(big_critic), x_stride=254),
                lambda: td(null_td=True), lambda: td(struct_size=C.sizeof(PmgTd3Target) - 8), lambda: td(struct_size=0),
                lambda: td(d_x_next=None), lambda: td(d_reward=None), lambda: td(d_y=None),
                lambda: td(d_x_next=d_x + 2), lambda: td(d_reward=d_r + 1), lambda: td(d_y=outs[0] + 2), lambda: td(d_q_min=outs[1] + 1), lambda: td(d_q1=outs[2] + 3),
                lambda: td(d_q2=outs[3] + 2), lambda: td(d_next_action=outs[4] + 3), lambda: td(d_work=outs[5] + 1), lambda: td(x_stride=Dx - 1), lambda: td(batch=-1),
                lambda: td(gamma=-0.1), lambda: td(gamma=INF), lambda: td(gamma=nan),
                lambda: td(clip_lo=0.0, clip_hi=-1.0), lambda: td(clip_lo=nan), lambda: td(clip_hi=nan),
                lambda: td(sigma=-0.1), lambda: td(sigma=INF), lambda: td(sigma=nan), lambda: td(noise_clip=-0.5), lambda: td(noise_clip=nan), lambda: td(noise_clip=-INF),
                lambda: td(row_offset=-1),
                lambda: td(d_next_action=None, d_work=None), lambda: td(d_next_action=None, work_floats=B * A - 1), lambda: td(d_next_action=None, work_floats=0)]
            good = h.td3_struct(B, d_x, Dx, d_r, outs[0], 0.98)
            assert h.L.lib.pmg_td3_target_device(h.h, None, C.byref(mlp(c1)), None, C.byref(good)) == E_INVALID
            assert h.L.lib.pmg_td3_target_device(h.h, C.byref(mlp(actor)), None, None, C.byref(good)) == E_INVALID
            for k, call in enumerate(bad):
                assert call() == E_INVALID, k
                assert h.L.error(h.h), k
            h.sync()
            for o in outs:
                assert (dev.get(o, 4 * B * A, np.uint8) == SENTINEL).all()
            assert td(batch=0) == 0 and td(batch=0, d_next_action=None, d_work=None, work_floats=0) == 0
            h.sync()
            for o in outs:
                assert (dev.get(o, 4 * B * A, np.uint8) == SENTINEL).all()
            # the workspace figure
            for twin in (0, 1):
                for na in (0, 1):
                    assert h.td3_target_work_floats(mlp(actor), twin, na, B) == (B * A if twin and not na else 0)
            assert h.td3_target_work_floats(mlp(actor), 1, 0, -1) < 0 and h.td3_target_work_floats(mlp(actor, num_layers=0), 1, 0, B) < 0
            # what is allowed: no workspace where none is needed, an infinite and a zero noise clip, sigma 0, one critic, an odd d_terminal
            assert td(d_work=None, work_floats=0) == 0 and td(m2=None, d_next_action=None, d_work=None, work_floats=0) == 0
            assert td(noise_clip=INF) == 0 and td(noise_clip=0.0) == 0 and td(sigma=0.0, row_offset=2 ** 40) == 0
            assert td(d_next_action=None, clip_lo=-1.0, clip_hi=-1.0, d_q_min=None, d_q1=None, d_q2=None, d_terminal=None) == 0
            h.sync()
            assert (dev.get(outs[0], 4 * B, np.uint8).view(F32) == -1).all()


# 7. the numpy face
def case_host_face(library):
    import pytest
    from pybullet_multigoal_gym_amd.critic import Critic
    env = AC.stepped(library, 'reach', 8)
    Dx, A = 6, 3
    Wa, ba = network(91, (Dx, 64, A))
    W1, b1, W2, b2 = critics(1300, Dx, A)
    critic, actor, critic2 = env.critic, env.actor, Critic(env)
    rs = np.random.RandomState(93)
    xn, r = rs.uniform(-2, 2, (37, Dx)).astype(F32), -rs.randint(0, 2, 37).astype(F32)
    term = rs.randint(0, 2, 37).astype(bool)
    critic.load(W1, b1)
    actor.load(Wa, ba, out_activation='identity')
    with pytest.raises(ValueError):
        critic.td3_target(actor, critic2, xn, r, 0.98)           # critic2 has no network
    critic2.load(W2, b2)
    assert critic.td3_target_work_floats(actor, critic2, 37) == 37 * A and critic.td3_target_work_floats(actor, critic2, 37, next_action=True) == 0
    assert critic.td3_target_work_floats(actor, None, 37) == 0
    for kw in ({}, {'clip_lo': -50.0, 'clip_hi': 0.0, 'terminal': term}):
        y, qm, q1, q2, na = critic.td3_target(actor, critic2, xn, r, 0.98, **kw)
        m = td3_model(xn, r, Wa, ba, W1, b1, W2, b2, 0.98, kw.get('clip_lo', -INF), kw.get('clip_hi', INF), kw.get('terminal'))
        check_td3({'y': y, 'qmin': qm, 'q1': q1, 'q2': q2, 'a': na}, m, kw)
    y, qm, q1, q2, na = critic.td3_target(actor, None, xn, r, 0.98)
    old = critic.td_target(actor, xn, r, 0.98)
    assert q2 is None
    for a, b in zip((y, q1, qm, na), (old[0], old[1], old[1], old[2])):
        eq_bits(a, b, 'one critic, no noise: td_target')
    y, qm, q1, q2, na = critic.td3_target(actor, critic2, xn, r, 0.98, sigma=SIGMA, noise_clip=NOISE_CLIP, seed=4, counter=5, row_offset=6)
    u1, u2 = draws(4, 5, 6, 37, A)
    assert np.abs(na - smooth64(forward(xn, Wa, ba), 0, u1, u2, SIGMA, NOISE_CLIP)).max() <= ACTION_TOL
    m = td3_model(xn, r, Wa, ba, W1, b1, W2, b2, 0.98, a=na)
    check_td3({'y': y, 'qmin': qm, 'q1': q1, 'q2': q2, 'a': na}, m, 'smoothed')
    y, qm, q1, q2, na = critic.td3_target(actor, critic2, xn[:0], r[:0], 0.98)
    assert y.shape == qm.shape == q1.shape == q2.shape == (0,) and na.shape == (0, A)
    for args, kw in (((actor, critic2, xn[:, :-1], r, 0.98), {}), ((actor, critic2, xn, r[:-1], 0.98), {}), ((actor, critic2, xn, r, -1.0), {}),
                     ((actor, critic2, xn, r, INF), {}), ((actor, critic2, xn, r, 0.98), {'clip_lo': 1.0, 'clip_hi': 0.0}),
                     ((actor, critic2, xn, r, 0.98), {'clip_lo': float('nan')}), ((actor, critic2, xn, r, 0.98), {'terminal': term[:-1]}),
                     ((critic, critic2, xn, r, 0.98), {}), ((actor, actor, xn, r, 0.98), {}), ((actor, critic2, xn, r, 0.98), {'sigma': -0.1}),
                     ((actor, critic2, xn, r, 0.98), {'sigma': INF}), ((actor, critic2, xn, r, 0.98), {'sigma': float('nan')}),
                     ((actor, critic2, xn, r, 0.98), {'noise_clip': -1.0}), ((actor, critic2, xn, r, 0.98), {'noise_clip': float('nan')}),
                     ((actor, critic2, xn, r, 0.98), {'row_offset': -1})):
        with pytest.raises(ValueError):
            critic.td3_target(*args, **kw)
    critic2.load(*network(96, (Dx + A + 1, 8, 1)))               # a second critic that does not fit
    with pytest.raises(ValueError):
        critic.td3_target(actor, critic2, xn, r, 0.98)
    critic2.close()
    env.close()


# 8. what tests/test_td3_wave_order.py runs under every wavefront order
def wave_order_run(library):
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        shapes = {'wide': (3, 12, (256, 256), (256,), (33, 255), 33, 1), 'far': (1, 20, (33,), (64,), (), 32, 0), 'small': (6, 3, (33,), (33,), (33,), 33, 0)}
        for name, (Dx, A, ah, h1, h2, B, act) in shapes.items():
            m = actor_case(Dx, A, ah, BATCHES[-1])
            nets = critics(1400 + Dx, Dx, A, h1, h2)
            for null in ((), ('a',)):
                got = device_td3(h, m['Wa'], m['ba'], *nets, m['x'][:B], m['r'][:B], 0.98, -50.0, 0.0, None, SIGMA, NOISE_CLIP, 3, 4, 5, act_out=act, x_pad=1, shift=1,
                                 null=null)
                for k in OUTPUTS:
                    if got[k] is not None:
                        res[name + k + str(len(null))] = got[k]
    return res
