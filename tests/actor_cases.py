"""The cases of the actor tests (include/pmg.h pmg_mlp_forward_device, pmg_act_env_device) and their numpy model,
shared by three files: tests/test_actor_emulated.py runs them on the g++ build of the product sources over the fiber emulator,
tests/test_gpu_actor.py on libpmg_hip.so on the MI355X, tests/test_actor_host.py covers env.actor and the model alone.  Every case
takes the loaded library and goes through the C ABI with buffers from pmg_device_alloc.

Bars.  A layer is one float32 fmaf chain per (row, unit) in ascending k: the pre-activations z are compared BY VALUE with the
exact numpy model of fmaf below (a padding product may turn -0 into +0, nothing else).  Draws are integer arithmetic: the set of
random envs and their actions v are bit-equal.  Actions with tanh / log / sqrt / cos are float32 library functions: they are held
to the float64 model evaluated from the device's own (bit-checked) z and the integer draws, within ACTION_TOL."""
import ctypes as C
import ctypes.util

import numpy as np

import her_cases as HC
import normalizer_cases as NC
import pybullet_multigoal_gym_amd as pmg
from normalizer_cases import GOAL, OBS, POL, SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PMG_BUF_PACKED, PmgError, PmgExplore, PmgMlp

TASK_NAMES = NC.TASK_NAMES
E_INVALID = -1
TILE = 32                          # rows per workgroup of pmg_k_mlp (MLP_ROWS)
BATCHES = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
KS = (1, 2, 3, 31, 32, 33, 255, 256)
OUTS = (1, 4, 31, 32, 33, 64, 65, 256)
CANARY_BYTES = 64
POISON = HC.POISON                 # padding between rows: anything read from it shows
NOISE_EPS = 0.2
# Largest |a - a64| measured over case_act (3 tasks x 2 state kinds x 2 handles x 2 activations, noise_eps = 0.2): 1.75e-7 on the
# MI355X, 1.74e-7 on the emulator; the bar is 4 x the larger.  A wrong draw index, column or row moves an action by
# the order of noise_eps.
ACTION_TOL = 4 * 1.75e-7
assert ACTION_TOL < 1e-4
PINNED = {'seed': 3, 'counter': 5, 'A': 4, 'g': (0, 1, 32, 2 ** 31 - 1), 'random_eps': 0.3}
U = np.uint64


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def fmaf(a, b, c):
    """float32 fma(a, b, c), exactly: the product is exact in float64, the sum is rounded to odd in float64 (TwoSum names the
    error), and a round-to-odd 53-bit value rounds to the same float32 as the exact one (53 >= 2 * 24 + 2)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over='ignore', invalid='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        s = np.array(s, np.float64, ndmin=1, copy=True)
        err = np.broadcast_to(err, s.shape)
        fix = (err != 0) & ((s.view(np.uint64) & U(1)) == 0) & np.isfinite(s)
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
        return s.astype(np.float32)


def forward(x, weights, biases):
    """-> z [B, width[L]] of the normative chain: acc = bias, acc = fmaf(h[k], W[j][k], acc) for ascending k, ReLU between layers"""
    h = np.asarray(x, np.float32)
    for l, W in enumerate(weights):
        b = biases[l] if biases is not None and biases[l] is not None else np.zeros(W.shape[0], np.float32)
        acc = np.broadcast_to(b.astype(np.float32), (h.shape[0], W.shape[0])).copy()
        for k in range(W.shape[1]):
            acc = fmaf(h[:, k:k + 1], W[None, :, k], acc).reshape(acc.shape)
        z, h = acc, np.maximum(acc, np.float32(0))
    return z


def explore_draws(seed, counter, g, A, random_eps):
    """-> u1, u2 [n, A] float64 (exact float32 values), v [n, A] float32, random [n] bool for the global envs g"""
    seed, counter = np.array([seed % 2 ** 64], U), np.array([counter % 2 ** 64], U)
    key = HC.mix(seed ^ HC.mix(counter + HC.GOLD))
    with np.errstate(over='ignore'):
        b = np.asarray(g, U)[:, None] * U(A) + np.arange(A, dtype=U)[None, :]
        r = [HC.mix(key + (U(4) * b + U(k + 1)) * HC.GOLD) >> U(32) for k in range(4)]
    u1 = ((r[0] >> U(8)) + U(1)).astype(np.float64) * 2.0 ** -24
    u2 = (r[1] >> U(8)).astype(np.float64) * 2.0 ** -24
    v = ((r[2] >> U(8)).astype(np.float64) * 2.0 ** -23 - 1.0).astype(np.float32)
    below = int(np.ceil(float(np.float32(random_eps)) * 4294967296.0))
    return u1, u2, v, r[3][:, 0].astype(object) < below


def actions64(z, out_act, noise_eps, u1, u2, v, random):
    """the float64 model of the action from given pre-activations and draws"""
    a = np.tanh(z.astype(np.float64)) if out_act else z.astype(np.float64)
    if noise_eps > 0:
        a = a + float(np.float32(noise_eps)) * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    a = np.clip(a, -1.0, 1.0)
    return np.where(np.asarray(random, bool)[:, None], v.astype(np.float64), a)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def network(seed, widths, bias=True):
    rs = np.random.RandomState(seed)
    Ws = [rs.uniform(-1, 1, (widths[l + 1], widths[l])).astype(np.float32) for l in range(len(widths) - 1)]
    bs = [rs.uniform(-0.5, 0.5, widths[l + 1]).astype(np.float32) for l in range(len(widths) - 1)] if bias else None
    return Ws, bs


_models = {}     # the model's z per (seed, widths, bias, B): computed once, shared by the tiers, never written


def random_case(seed, widths, bias, B):
    key = (seed, tuple(widths), bias, B)
    if key not in _models:
        Ws, bs = network(seed, widths, bias)
        x = np.random.RandomState(seed + 1000).uniform(-2, 2, (B, widths[0])).astype(np.float32)
        z = forward(x, Ws, bs)
        for a in (x, z):
            a.setflags(write=False)
        _models[key] = (Ws, bs, x, z)
    return _models[key]


# ----------------------------------------------------------------------------------------------------------------------
# device calls
class Net:
    """A network on the device, freed with `dev`."""

    def __init__(self, h, dev, Ws, bs, out_act=0):
        self.widths = [Ws[0].shape[1]] + [w.shape[0] for w in Ws]
        self.d_w = [dev.put(w) for w in Ws]
        self.d_b = None if bs is None else [None if b is None else dev.put(b) for b in bs]
        self.mlp = h.mlp_struct(self.widths, self.d_w, self.d_b, out_act)


def device_forward(h, Ws, bs, x, out_act=0, in_pad=0, out_pad=0, in_shift=0, out_shift=0):
    """pmg_mlp_forward_device on canary-framed buffers -> out [B, width[L]].  in_pad / out_pad: floats between rows (poison on
    the input side, sentinel bytes that must survive on the output side); *_shift: floats off the 16-byte boundary."""
    B, K = x.shape
    A = Ws[-1].shape[0]
    with Dev(h) as dev:
        net = Net(h, dev, Ws, bs, out_act)
        xin = np.full((B, K + in_pad), POISON, np.float32)
        xin[:, :K] = x
        d_in = dev.alloc(xin.nbytes + 32)
        d_in += (-d_in) % 16 + 4 * in_shift
        h.upload(d_in, xin)
        stride = A + out_pad
        off, nbytes = CANARY_BYTES + 4 * out_shift, 4 * B * stride
        base = dev.put(np.full(off + nbytes + CANARY_BYTES, SENTINEL, np.uint8))
        assert base % 16 == 0
        h.mlp_forward_device(net.mlp, d_in, K + in_pad, B, base + off, stride)
        raw = dev.get(base, off + nbytes + CANARY_BYTES, np.uint8)
    assert (raw[:off] == SENTINEL).all() and (raw[off + nbytes:] == SENTINEL).all(), 'bytes around d_out were written'
    rows = raw[off:off + nbytes].reshape(B, 4 * stride)
    assert (rows[:, 4 * A:] == SENTINEL).all(), 'the padding between output rows was written'
    return np.ascontiguousarray(rows[:, :4 * A]).view(np.float32)


def check_z(got, want, label):
    assert got.shape == want.shape and np.array_equal(got, want), (label, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])


def device_act(h, net, kind, explore=None, preact=True, rc=0):
    """pmg_act_env_device into canary-framed buffers -> actions [N, A], z [N, A] (or None)"""
    N, A = h.N, h.dims.action_dim
    nbytes = 4 * N * A
    with Dev(h) as dev:
        bufs = [dev.put(np.full(CANARY_BYTES + nbytes + CANARY_BYTES, SENTINEL, np.uint8)) for _ in range(2)]
        ex = None if explore is None else h.explore_struct(**explore)
        got = h.L.lib.pmg_act_env_device(h.h, C.byref(net.mlp), C.c_int(kind), C.byref(ex) if ex is not None else None,
                                         C.c_void_p(bufs[0] + CANARY_BYTES), C.c_void_p(bufs[1] + CANARY_BYTES) if preact else None)
        assert got == rc, (got, h.L.error(h.h))
        out = []
        for k, b in enumerate(bufs):
            raw = dev.get(b, CANARY_BYTES + nbytes + CANARY_BYTES, np.uint8)
            assert (raw[:CANARY_BYTES] == SENTINEL).all() and (raw[CANARY_BYTES + nbytes:] == SENTINEL).all(), 'bytes around an output were written'
            if rc != 0 or (k == 1 and not preact):
                assert (raw == SENTINEL).all(), 'an output was written although it was NULL or the call was refused'
                out.append(None)
            else:
                out.append(raw[CANARY_BYTES:CANARY_BYTES + nbytes].copy().view(np.float32).reshape(N, A))
    return out


def policy_rows(h, kind):
    """what pmg_policy_input_env_device writes for the current rows"""
    W = h.norm_width(kind) + h.dims.goal_dim
    with Dev(h) as dev:
        d = dev.alloc(4 * h.N * W)
        h.policy_input_env_device(kind, d)
        return dev.get(d, (h.N, W), np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# 0. the model alone
def test_model_fmaf_is_libm():
    libm = C.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    rs = np.random.RandomState(5)
    n = 20000
    a = (rs.uniform(-1, 1, n) * 2.0 ** rs.randint(-20, 20, n)).astype(np.float32)
    b = (rs.uniform(-1, 1, n) * 2.0 ** rs.randint(-20, 20, n)).astype(np.float32)
    sets = [(a, b, (rs.uniform(-1, 1, n) * 2.0 ** rs.randint(-30, 30, n)).astype(np.float32)),      # random
            (a, b, -(a * b) * (1 + rs.randint(-2, 3, n) * np.float32(2.0 ** -23))),                   # cancelling: c = -fl(a b) (1 + few ulp)
            (a, b, (rs.uniform(-1, 1, n) * 2.0 ** 40).astype(np.float32)),                            # large c: the product is below its ulp
            ((a * np.float32(1e-25)), (b * np.float32(1e-15)), (rs.uniform(-1, 1, n) * 1e-42).astype(np.float32))]   # subnormal
    for k, (x, y, c) in enumerate(sets):
        x, y, c = (np.asarray(v, np.float32) for v in (x, y, c))
        want = np.array([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(x, y, c)], np.float32)
        got = fmaf(x, y, c)
        assert np.array_equal(bits(got), bits(want)), (k, np.argwhere(bits(got) != bits(want))[:4])
    # chains: the model against libm in ascending order; another order of the same float32 sum differs on most
    differ = 0
    for i in range(200):
        h, w = rs.uniform(-1, 1, 256).astype(np.float32), rs.uniform(-1, 1, 256).astype(np.float32)
        acc = 0.0
        for p, q in zip(h, w):
            acc = libm.fmaf(float(p), float(q), acc)
        assert forward(h[None], [w[None]], None)[0, 0] == np.float32(acc)
        differ += np.float32(acc) != forward(h[None, ::-1], [w[None, ::-1]], None)[0, 0]
    assert differ > 100


def test_model_pinned_draws():
    p = PINNED
    u1, u2, v, rnd = explore_draws(p['seed'], p['counter'], p['g'], p['A'], p['random_eps'])
    assert ((u1 > 0) & (u1 <= 1)).all() and ((u2 >= 0) & (u2 < 1)).all() and ((v >= -1) & (v < 1)).all()
    for a in (u1, u2):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)          # exact in float32
    assert [int(x) for x in np.round(u1[:, 0] * 2 ** 24)] == PINNED_U1 and [int(x) for x in np.round(u2[:, 1] * 2 ** 24)] == PINNED_U2
    assert [int(x) for x in np.round((v[:, 2].astype(np.float64) + 1) * 2 ** 23)] == PINNED_V and list(rnd) == PINNED_RANDOM


PINNED_U1 = [779735, 3650373, 10881295, 14671045]
PINNED_U2 = [2576538, 5169368, 2412667, 3804]
PINNED_V = [10025707, 16710172, 13394977, 15641867]
PINNED_RANDOM = [True, True, True, False]


def test_model_statistics():
    """the draws on the model alone, 16384 envs x 4 columns: the Gaussian's mean and variance, the random share and the uniform v
    within 5 standard deviations; every bound of the specification"""
    n, A = 16384, 4
    for seed, counter in ((0, 0), (1, 0), (0, 1), (12345, 7), (2 ** 63 + 5, 2 ** 40)):
        u1, u2, v, rnd = explore_draws(seed, counter, np.arange(n) + 32, A, 0.3)
        assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1 and v.min() >= -1 and v.max() < 1
        gauss = (np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)).ravel()
        m = gauss.size
        share = np.asarray(rnd, bool).mean()
        print('seed %d counter %d: gauss mean %.4f var %.4f, random share %.4f, v mean %.4f' % (seed, counter, gauss.mean(), gauss.var(), share, v.mean()))
        assert abs(gauss.mean()) < 5 / np.sqrt(m) and abs(gauss.var() - 1) < 5 * np.sqrt(2.0 / m)
        assert abs(share - 0.3) < 5 * np.sqrt(0.3 * 0.7 / n)
        assert abs(v.mean()) < 5 / np.sqrt(3 * m) and abs(v.var() - 1 / 3) < 5 * np.sqrt(4 / 45 / m)
    assert not np.asarray(explore_draws(1, 2, np.arange(64), 3, 0.0)[3], bool).any()
    assert np.asarray(explore_draws(1, 2, np.arange(64), 3, 1.0)[3], bool).all()


# ----------------------------------------------------------------------------------------------------------------------
# 1. one layer: every K x every width, the batches in turn
def case_one_layer(library, ks=KS):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        n, negative = 0, False
        for K in ks:
            for Nn in OUTS:
                B, bias = BATCHES[n % len(BATCHES)], bool(n % 2)
                n += 1
                Ws, bs, x, z = random_case(7 * K + Nn, (K, Nn), bias, B)
                negative |= bool((z < 0).any())
                check_z(device_forward(h, Ws, bs, x), z, (K, Nn, B, bias))
        assert negative                                   # ReLU would matter


# 2. every batch size, padded strides with poison, both alignment shifts
def case_batches_and_strides(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for widths in ((33, 65), (3, 4), (256, 256)):
            for B in BATCHES:
                for bias in (False, True):
                    Ws, bs, x, z = random_case(11, widths, bias, B)
                    got = device_forward(h, Ws, bs, x, in_pad=5, out_pad=3, in_shift=1 if bias else 0, out_shift=0 if bias else 1)
                    check_z(got, z, (widths, B, bias, 'padded'))
        Ws, bs, x, z = random_case(11, (33, 65), True, BATCHES[-1])
        for shift in (1, 2, 3):
            check_z(device_forward(h, Ws, bs, x, in_shift=shift, out_shift=4 - shift, in_pad=shift), z, ('shift', shift))


# 3. two to four layers
DEEP = ((33, 65, 4), (3, 256, 256, 256, 4), (255, 1, 2, 33), (10, 64, 31, 3), (256, 33, 256, 1, 64), (2, 32, 32))


def case_deep(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, widths in enumerate(DEEP):
            for bias in (False, True):
                B = BATCHES[(n + bias) % len(BATCHES)] if widths != DEEP[1] else BATCHES[-1]
                Ws, bs, x, z = random_case(20 + n, widths, bias, B)
                check_z(device_forward(h, Ws, bs, x, in_pad=n % 2, out_pad=n % 3), z, (widths, B, bias))
        # a hidden layer's output by bits: an identity second layer hands ReLU(acc) through (value + 0 products)
        Ws, bs, x, z1 = random_case(31, (33, 65), True, TILE + 1)
        relu = np.maximum(z1, np.float32(0))
        assert (relu == 0).any() and (relu > 0).any()
        got = device_forward(h, [Ws[0], np.eye(65, dtype=np.float32)], [bs[0], None], x)
        assert np.array_equal(bits(got), bits(relu))
        # tanh on the plain forward: the float32 library function on the bit-checked z
        got = device_forward(h, Ws, bs, x, out_act=1)
        assert np.abs(got - np.tanh(z1.astype(np.float64))).max() <= ACTION_TOL


# 4. exact integers and subnormals
def case_exact_integers(library):
    """one-hot rows against W[j][k] = j K + k (asymmetric): z[r][j] = j K + r exactly -- a swapped row / column map or a wrong k
    names itself by the integer it returns"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for K, Nn in ((33, 65), (64, 256), (255, 31)):
            W = (np.arange(Nn)[:, None] * K + np.arange(K)[None, :]).astype(np.float32)
            assert W.max() < 2 ** 24
            x = np.eye(K, dtype=np.float32)
            got = device_forward(h, [W], None, x)
            want = W.T
            assert np.array_equal(got, want), (K, Nn, np.argwhere(got != want)[:4], got[got != want][:4])
        # subnormal products and sums come through un-flushed
        rs = np.random.RandomState(3)
        x = (rs.uniform(-1, 1, (TILE + 1, 33)) * 1e-24).astype(np.float32)
        W = (rs.uniform(-1, 1, (65, 33)) * 1e-17).astype(np.float32)
        z = forward(x, [W], None)
        assert (z != 0).mean() > 0.9 and (np.abs(z) < 1.1754944e-38).all()
        check_z(device_forward(h, [W], None, x), z, 'subnormal')


# ----------------------------------------------------------------------------------------------------------------------
# 5. act on the env's rows
def stepped(library, task, N, **kw):
    env = pmg.make_env(task=task, num_envs=N, seed=3, seed_stride=1, _library=library, **dict(NC.TASKS[task][0], **kw))
    NC.prime(env.handle)
    env.reset()
    return env


def case_act(library, task):
    N = TILE + 5
    worst = 0.0
    for offset in (0, 32):
        env = stepped(library, task, N, env_index_offset=offset)
        h, A = env.handle, env.dims.action_dim
        g = np.arange(N) + offset
        for kind in (OBS, POL):
            W0 = h.norm_width(kind) + h.dims.goal_dim
            Ws, bs = network(50 + kind, (W0, 64, 33, A))
            x = policy_rows(h, kind)
            scale = np.float32(2.0 ** np.floor(np.log2(0.7 / np.abs(forward(x, Ws, bs)).max())))
            Ws[-1], bs[-1] = Ws[-1] * scale, bs[-1] * scale  # |z| <= 0.7: tanh off saturation, the noise and the clip both show
            z_model = forward(x, Ws, bs)
            for out_act in (1, 0):
                with Dev(h) as dev:
                    net = Net(h, dev, Ws, bs, out_act)
                    plain, z = device_act(h, net, kind)
                    check_z(z, z_model, (task, kind, 'z'))
                    quiet, _ = device_act(h, net, kind, dict(noise_eps=0.0, random_eps=0.0, seed=9, counter=9), preact=False)
                    assert np.array_equal(bits(plain), bits(quiet))
                    none = np.zeros(N, bool)
                    worst = max(worst, np.abs(plain - actions64(z, out_act, 0.0, None, None, np.zeros_like(z), none)).max())
                    if out_act == 0:
                        assert np.array_equal(plain, np.clip(z, np.float32(-1), np.float32(1)))
                    ex = dict(noise_eps=NOISE_EPS, random_eps=0.3, seed=2 ** 63 + 7, counter=11)
                    a, z2 = device_act(h, net, kind, ex)
                    again, _ = device_act(h, net, kind, ex)
                    other, _ = device_act(h, net, kind, dict(ex, counter=12))
                    assert np.array_equal(bits(z2), bits(z)) and np.array_equal(bits(a), bits(again)) and not np.array_equal(a, other)
                    u1, u2, v, rnd = explore_draws(ex['seed'], ex['counter'], g, A, ex['random_eps'])
                    rnd = np.asarray(rnd, bool)
                    assert rnd.any() and not rnd.all()
                    assert np.array_equal(bits(a[rnd]), bits(v[rnd])), (task, kind, 'random envs')
                    a64 = actions64(z, out_act, NOISE_EPS, u1, u2, v, rnd)
                    dev_max = np.abs(a - a64).max()
                    worst = max(worst, dev_max)
                    assert (np.abs(a) <= 1).all() and (np.abs(a[~rnd]) < 1).any()
                    assert dev_max <= ACTION_TOL, (task, kind, out_act, dev_max)
                    allr, _ = device_act(h, net, kind, dict(ex, random_eps=1.0))
                    assert np.array_equal(bits(allr), bits(v))
                    nor, _ = device_act(h, net, kind, dict(ex, random_eps=0.0))
                    assert np.abs(nor - actions64(z, out_act, NOISE_EPS, u1, u2, v, none)).max() <= ACTION_TOL
                    assert np.array_equal(bits(nor[~rnd]), bits(a[~rnd]))
        env.close()
    print('%s: largest |a - a64| = %.3g (bar %.3g)' % (task, worst, ACTION_TOL))
    return worst


# 6. the handle is untouched
def case_handle_untouched(library):
    env = stepped(library, 'push', TILE + 5)
    h = env.handle

    def snapshot(dev):
        packed = dev.get(h.device_ptr(PMG_BUF_PACKED), (h.N, h.dims.packed_dim), np.uint32)
        derived = [np.concatenate([v for k, v in sorted(h.norm_read(w).items()) if k in ('mean', 'std', 'inv_std')]) for w in NC.KINDS]
        return NC.all_totals(h) + derived + [packed, h.get_state(), h.get_rng()]
    Ws, bs = network(1, (h.norm_width(POL) + 3, 64, 3))
    Wf, bf, x, z = random_case(11, (33, 65), True, BATCHES[-1])
    with Dev(h) as dev:
        before = snapshot(dev)
        device_act(h, Net(h, dev, Ws, bs, 1), POL, dict(noise_eps=0.2, random_eps=0.5, seed=1, counter=2))
        check_z(device_forward(h, Wf, bf, x), z, 'forward')
        after = snapshot(dev)
    for a, b in zip(before, after):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    env.close()


# 7. with the env: act_env_device -> step_device against step() with the downloaded actions
def case_with_the_env(library, overlap=False):
    N = TILE + 5
    envs = [pmg.make_env(task='reach', num_envs=N, seed=5, seed_stride=1, _library=library) for _ in range(2)]
    dev_env, host_env = envs
    h = dev_env.handle
    if overlap:
        h.comm_overlap(True)
    for e in envs:
        NC.prime(e.handle)
        e.reset()
    Ws, bs = network(2, (h.norm_width(POL) + 3, 64, 64, 3))
    seen = set()
    with Dev(h) as dev:
        net = Net(h, dev, Ws, bs, 1)
        d_act = dev.alloc(4 * N * 3)
        for t in range(3):
            ex = h.explore_struct(0.2, 0.3, 77, t)
            h.act_env_device(net.mlp, POL, d_act, None, ex)
            a = dev.get(d_act, (N, 3), np.float32)
            h.step_device(d_act)
            seen.add(h.device_ptr(PMG_BUF_PACKED))
            host_env.handle.step(a)
            rows = dev.get(h.device_ptr(PMG_BUF_PACKED), (N, h.dims.packed_dim), np.uint32)
            with Dev(host_env.handle) as hd:
                want = hd.get(host_env.handle.device_ptr(PMG_BUF_PACKED), (N, h.dims.packed_dim), np.uint32)
            assert np.array_equal(rows, want), t
            assert t == 0 or not np.array_equal(a, last)
            last = a
    assert len(seen) == (2 if overlap else 1)
    for e in envs:
        e.close()


# 8. invalid calls
def case_invalid_calls(library):
    env = stepped(library, 'push', 8)
    h, d = env.handle, env.handle.dims
    W0, A = h.norm_width(POL) + d.goal_dim, d.action_dim
    Ws, bs = network(4, (W0, 16, A))
    with Dev(h) as dev:
        net = Net(h, dev, Ws, bs, 1)
        d_in = dev.put(np.zeros((8, W0), np.float32))
        outs = [dev.put(np.full(4 * 8 * A, SENTINEL, np.uint8)) for _ in range(3)]
        vp, i64 = C.c_void_p, C.c_int64

        def mlp(**kw):
            m = h.mlp_struct(net.widths, net.d_w, net.d_b, 1)
            for k, v in kw.items():
                if k in ('width', 'd_weight', 'd_bias'):
                    getattr(m, k)[v[0]] = v[1]
                else:
                    setattr(m, k, v)
            return m

        def fwd(m=None, d_in=d_in, in_stride=W0, batch=8, d_out=outs[0], out_stride=A):
            return h.L.lib.pmg_mlp_forward_device(h.h, C.byref(m or mlp()), vp(d_in), i64(in_stride), i64(batch), vp(d_out), i64(out_stride))

        def act(m=None, kind=POL, ex=None, d_actions=outs[1], d_preact=outs[2], **exkw):
            if exkw:
                ex = h.explore_struct(**exkw)
            return h.L.lib.pmg_act_env_device(h.h, C.byref(m or mlp()), C.c_int(kind), C.byref(ex) if ex is not None else None, vp(d_actions), vp(d_preact))
        bad_nets = [mlp(struct_size=C.sizeof(PmgMlp) - 8), mlp(struct_size=0), mlp(num_layers=0), mlp(num_layers=5), mlp(num_layers=-1),
                    mlp(width=(0, 0)), mlp(width=(1, 257)), mlp(width=(2, -3)), mlp(d_weight=(0, None)), mlp(d_weight=(1, None)),
                    mlp(out_activation=2), mlp(d_weight=(0, net.d_w[0] + 2))]
        short = h.explore_struct()
        short.struct_size -= 4
        bad = [lambda m=m: fwd(m) for m in bad_nets] + [lambda m=m: act(m) for m in bad_nets] + [
            lambda: fwd(d_in=None), lambda: fwd(d_out=None), lambda: fwd(in_stride=W0 - 1), lambda: fwd(out_stride=A - 1), lambda: fwd(batch=-1),
            lambda: fwd(d_out=outs[0] + 2),
            lambda: act(kind=GOAL), lambda: act(kind=7), lambda: act(kind=-1), lambda: act(kind=OBS),      # OBS: widths do not match the dims
            lambda: act(mlp(width=(0, W0 + 1))), lambda: act(mlp(width=(2, A + 1))), lambda: act(d_actions=None),
            lambda: act(ex=short), lambda: act(noise_eps=-0.1), lambda: act(noise_eps=float('inf')), lambda: act(noise_eps=float('nan')),
            lambda: act(random_eps=-0.01), lambda: act(random_eps=1.5), lambda: act(random_eps=float('nan'))]
        for k, call in enumerate(bad):
            assert call() == E_INVALID, k
            assert h.L.error(h.h), k
        h.sync()
        for o in outs:
            assert (dev.get(o, 4 * 8 * A, np.uint8) == SENTINEL).all()
        assert fwd(batch=0) == 0 and act(d_preact=None) == 0 and act(d_preact=None, noise_eps=0.0, random_eps=1.0) == 0
        h.sync()
        assert (dev.get(outs[0], 4 * 8 * A, np.uint8) == SENTINEL).all() and (dev.get(outs[2], 4 * 8 * A, np.uint8) == SENTINEL).all()
    env.close()


# 9. host face
def case_host_face(library):
    import pytest
    env = stepped(library, 'push', TILE + 5)
    h = env.handle
    W0 = h.norm_width(POL) + 3
    Ws, bs = network(6, (W0, 64, 3))
    actor = env.actor
    assert actor is env.actor
    with pytest.raises(ValueError):
        actor.forward(np.zeros((2, W0), np.float32))         # nothing loaded
    actor.load(Ws, bs, out_activation='identity')
    x = np.random.RandomState(8).uniform(-2, 2, (5, 7, W0)).astype(np.float32)
    z = forward(x.reshape(35, W0), Ws, bs).reshape(5, 7, 3)
    got = actor.forward(x)
    assert got.shape == (5, 7, 3) and np.array_equal(got, z) and actor.forward(x[:0]).shape == (0, 7, 3)
    zenv = forward(policy_rows(h, POL), Ws, bs)
    assert np.array_equal(actor.act(), np.clip(zenv, np.float32(-1), np.float32(1)))
    actor.load(Ws, [bs[0], None])                            # tanh, and a layer without a bias
    zenv = forward(policy_rows(h, POL), Ws, [bs[0], None])
    u1, u2, v, rnd = explore_draws(5, 6, np.arange(h.N), 3, 0.25)
    a = actor.act(noise_eps=NOISE_EPS, random_eps=0.25, seed=5, counter=6)
    assert np.abs(a - actions64(zenv, 1, NOISE_EPS, u1, u2, v, rnd)).max() <= ACTION_TOL
    assert np.array_equal(bits(a[np.asarray(rnd, bool)]), bits(v[np.asarray(rnd, bool)]))
    d_a = h.device_alloc(4 * h.N * 3)
    actor.act_device(d_a, noise_eps=NOISE_EPS, random_eps=0.25, seed=5, counter=6)
    back = np.empty_like(a)
    h.sync()
    h.download(back, d_a)
    h.device_free(d_a)
    assert np.array_equal(bits(back), bits(a))
    for args, kw in ((([Ws[0][:-1], Ws[1]], [bs[0][:-1], bs[1]]), {}), (([Ws[0], Ws[1][:, :-1]], bs), {}), ((Ws, bs[:1]), {}), ((Ws, [bs[0][:-1], bs[1]]), {}),
                     (([], []), {}), (([Ws[0]] * 5, None), {}), (([np.zeros((257, 3), np.float32)], None), {}), (([Ws[0][0]], None), {}),
                     ((Ws, bs), {'out_activation': 'relu'})):
        with pytest.raises(ValueError):
            actor.load(*args, **kw)
    for kw in ({'kind': 'goal'}, {'noise_eps': -1.0}, {'random_eps': 2.0}):
        with pytest.raises(ValueError):
            actor.act(**kw)
    with pytest.raises(ValueError):
        actor.forward(np.zeros((2, W0 + 1), np.float32))
    with pytest.raises(PmgError):
        actor.act(kind='observation')                        # the network does not take observation rows
    actor.close()
    with pytest.raises(ValueError):
        actor.act()
    env.close()
