"""The cases of the PPO calls (include/pmg.h pmg_gae_device, pmg_adv_stats_device, pmg_adv_apply_device, pmg_ppo_policy_grad_device,
pmg_ppo_stats_device) and their numpy models, shared by four files: tests/test_ppo_emulated.py runs them on the g++ build of the
product sources over the fiber emulator, tests/test_gpu_ppo.py on libpmg_hip.so on the MI355X, tests/test_ppo_host.py covers the models alone,
tests/test_ppo_wave_order.py the rows kernel under permuted wavefront order.  The pieces are those of tests/sac_cases.py (the Gaussian actors,
the sampler), tests/grad_cases.py / tests/grad_chunk_cases.py (the exact fmaf chains of the backward, the device calls) and tests/td_cases.py
(the canaries).

Bit for bit.  GAE, the mean of the normaliser, its apply step given the device's own statistics, the four minibatch statistics and d_clipped
given the call's own rho are held to the numpy models below bit for bit.  z is held to pmg_mlp_forward_device INDIRECTLY -- no output exposes z:
with zo = that call's z and n = 0, g_mu is zero exactly iff the means agree bit for bit, and the log-ratio is +0.0 iff the CLAMPED log-stds
agree; a raw log-std outside the clamp is pinned only through the clamp predicate in g_ls (against the model's) and the bit comparison of
dW / db --, dW / db to pmg_mlp_grad[_chunked]_device of the actor on the call's own
d_ghead (zeros by value).

Bars.  lr, rho, g_mu and g_ls go through the build's expf.  They are held to the numpy float32 model relative to first-order magnitudes of their
summands (computed in head64; with c = isd (|sd_o n| + |zo_mu| + |m|), the weight of the cancellation in u - m on w,
  mag_lr = sum_j (w^2 / 2 + |ls| + n^2 / 2 + |ls_o| + |w| c),                 rho: rho (1 + mag_lr),
  mag_mu = |k| isd (|w| (1 + mag_lr) + c),   mag_ls = |k| ((w^2 + 1) (1 + mag_lr) + 2 |w| c) + |escale|);
the whole gradient is held to float64 autograd of the textbook loss, relative to the largest |entry| of each tensor, the worst tensor; 1 / (std + eps)
of the normaliser to its float64 model, relative.  Each bar is 4 x the error MEASURED on the numpy model alone against float64 (measure_*
below, run by tests/test_ppo_host.py), the headroom the project gives library functions that differ by an ulp or two between numpy and a
build.  None of them comes from a device's output.

Margins (asserted by tests/test_ppo_host.py on the float64 model, every row of every case): every rho is at least RHO_MARGIN (relative) away
from clip_lo and clip_hi, every raw log-std of the new and of the old policy at least LS_MARGIN away from ls_lo and ls_hi, every |adv| at least
ADV_MARGIN: no clip or clamp predicate is at a tie or within rounding of one."""
import ctypes as C
from fractions import Fraction

import numpy as np

import actor_cases as AC
import grad_cases as GC
import grad_chunk_cases as GCC
import sac_cases as SC
import td_cases as TC
from actor_cases import POISON, Net, bits, fmaf, forward, network
from grad_cases import Params, eq_val, read_rows, rows_out
from normalizer_cases import SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PmgAdvStats, PmgGae, PmgMlp, PmgPpoPolicyGrad, PmgPpoStats
from td_cases import Out, eq_bits, put_rows

E_INVALID = -1
F32, F64 = np.float32, np.float64
TILE = AC.TILE
INF = float('inf')
NAN_WORD = 0x7FC00000 | 0x1234
PAIRS = SC.PAIRS
BATCHES = TC.BATCHES
RHO_MARGIN = 1e-3              # relative distance of every float64 rho from either end of the clip: float32 rho is within 1e-5 of it (measured below)
LS_MARGIN = 1e-3               # of every raw log-std from either end of the clamp: the raw log-stds are bit-defined, any positive margin does
ADV_MARGIN = 0.05              # of every |adv| from 0: the advantages are inputs, any positive margin does
CLIP_EPS = 0.2
CLIP_LO, CLIP_HI = float(F32(1) - F32(CLIP_EPS)), float(F32(1) + F32(CLIP_EPS))
ENT_COEF = 0.01
# measured by measure_head_bars() over every input of CASES (numpy float32 restatement of the head against float64; x86-64 glibc / numpy)
PPO_LR_MEASURED = 4.7e-8       # 4.636e-8
PPO_RHO_MEASURED = 4.1e-8      # 4.017e-8
PPO_MU_MEASURED = 3.4e-8       # 3.345e-8
PPO_LS_MEASURED = 4.7e-8       # 4.623e-8
PPO_LR_TOL, PPO_RHO_TOL, PPO_MU_TOL, PPO_LS_TOL = 4 * PPO_LR_MEASURED, 4 * PPO_RHO_MEASURED, 4 * PPO_MU_MEASURED, 4 * PPO_LS_MEASURED
# measured by measure_model_bar() (the numpy float32 model of steps 1-7 against float64 autograd, MODEL_NETS)
PPO_MEASURED = 2.5e-6          # 2.489e-6
PPO_TOL = 4 * PPO_MEASURED
# measured by measure_inv_bar() (the float32 value of the double model of 1 / (std + eps), S * mean fused or not, against float64, STATS_M)
ADV_INV_MEASURED = 5.8e-8      # 5.747e-8
ADV_INV_TOL = 4 * ADV_INV_MEASURED
# (Dx, A, actor hidden, bias, B, chunk_rows): every pair of sac_cases.PAIRS, the hidden shapes mixed, every batch, every chunk regime at B = 101
CASES = ((6, 3, (33,), True, 101, None),
         (6, 3, (), False, 33, None),
         (1, 1, (33,), True, 1, None),
         (2, 5, (256, 256, 256), True, 31, None),
         (3, 12, (33,), True, 101, 2),
         (29, 4, (256, 256, 256), False, 32, None),
         (1, 20, (), True, 101, 32),
         (5, 9, (33,), True, 101, 128))


# ----------------------------------------------------------------------------------------------------------------------
# generalised advantage estimation
GAE_T = (1, 2, 7)
GAE_N = (1, 63, 64, 65, 257)
PACK = 7                        # floats per row of the packed-like table; reward in column 2, cut in column 5
PACK_R, PACK_C = 2, 5


def gae_model(reward, value, value_next, gamma, lam, cut=None, terminal=None):
    """the normative chain in float32 -> adv, ret [T, N]"""
    r, v, vn = (np.asarray(a, F32) for a in (reward, value, value_next))
    T, N = r.shape
    g, gl = F32(gamma), F32(F32(gamma) * F32(lam))
    adv, ret = np.zeros((T, N), F32), np.zeros((T, N), F32)
    run = np.zeros(N, F32)
    with np.errstate(over='ignore', invalid='ignore'):
        for t in range(T - 1, -1, -1):
            nv = vn[t] if terminal is None else np.where(np.asarray(terminal[t]) != 0, F32(0), vn[t])
            delta = fmaf(np.full(N, g, F32), nv, r[t]).reshape(N) - v[t]
            chained = fmaf(np.full(N, gl, F32), run, delta).reshape(N)
            stop = np.ones(N, bool) if t == T - 1 else (np.zeros(N, bool) if cut is None else np.asarray(cut[t]) != 0)
            run = np.where(stop, delta, chained).astype(F32)
            adv[t], ret[t] = run, run + v[t]
    return adv, ret


def gae_inputs(T, N, seed=0):
    """rewards, a [T + 1, N] value table, a successor table of its own, cuts (at t = 0, mid-rollout and t = T - 1 among them) and terminals
    (with and without a cut)"""
    def make():
        rs = np.random.RandomState(4000 + 31 * T + N + seed)
        r = rs.uniform(-1, 1, (T, N)).astype(F32)
        vtab = rs.standard_normal((T + 1, N)).astype(F32)
        succ = rs.standard_normal((T, N)).astype(F32)
        cut = (rs.uniform(0, 1, (T, N)) < 0.3).astype(F32) * rs.choice([1.0, 0.5, -2.0], (T, N)).astype(F32)      # any non-zero value is a cut
        term = (rs.uniform(0, 1, (T, N)) < 0.25).astype(F32)
        for k, t in enumerate((0, T // 2, T - 1)):
            i = k % N
            cut[t, i] = 1.0
            term[t, i] = float(k & 1)
            term[t, (i + 1) % N], cut[t, (i + 1) % N] = (1.0, 0.0) if N > 1 else (term[t, i], cut[t, i])
        return {'r': r, 'vtab': vtab, 'succ': succ, 'cut': cut, 'term': term}
    return TC.cached(('gae', T, N, seed), make)


def _strides(T, N, layout):
    """-> time stride, env stride, floats of the buffer"""
    if layout == 'time':
        return N + 3, 1, T * (N + 3)
    if layout == 'tight':
        return N, 1, T * N
    if layout == 'env':
        return 1, T + 2, N * (T + 2)
    if layout == 'packed':
        return N * PACK, PACK, T * N * PACK
    raise ValueError(layout)


def _index(T, N, ts, es):
    return (np.arange(T)[:, None] * ts + np.arange(N)[None, :] * es).astype(np.int64)


class _OutTable:
    """a canary-framed, sentinel-filled output table of GAE; reverse: time runs backwards from the last block (a negative time stride)"""

    def __init__(self, dev, T, N, layout, shift, reverse=False):
        ts, es, size = _strides(T, N, layout)
        self.out = Out(dev, 4 * size, 4 * shift)
        self.idx, self.size = _index(T, N, ts, es), size
        self.tab = (self.out.ptr, ts, es)
        if reverse:
            self.idx = self.idx[::-1]
            self.tab = (self.out.ptr + 4 * (T - 1) * ts, -ts, es)

    def read(self, written=True):
        raw = self.out.read(np.uint8, written)
        if raw is None:
            return None
        words = raw.view(np.uint32)
        rest = np.ones(self.size, bool)
        rest[self.idx.ravel()] = False
        assert (words[rest] == int(np.array([SENTINEL] * 4, np.uint8).view(np.uint32)[0])).all(), 'floats between the elements of an output table were written'
        return words[self.idx].view(F32)


def _put_table(h, dev, arr, layout, shift=0):
    T, N = arr.shape
    ts, es, size = _strides(T, N, layout)
    buf = np.full(size, POISON, F32)
    buf[_index(T, N, ts, es)] = arr
    p, _ = put_rows(h, dev, buf[None, :], 0, shift)
    return p, ts, es


def device_gae(h, c, gamma, lam, layout='time', succ='own', cut=True, term=True, ret=True, shift=0, reverse=False, T=None):
    """pmg_gae_device on case c -> adv, ret (None when not asked for).  layout: 'time' (rows of N + 3 floats), 'tight', 'env' (columns of T + 2
    floats) for every table, or 'packed': reward and cut are columns of ONE table of rows of PACK floats, the rest time-major.  succ: 'own' (the
    successor table) or 'shift' (d_value_next = d_value + one step of the [T + 1, N] value table)."""
    r = c['r'] if T is None else c['r'][:T]
    T, N = r.shape
    inner = 'time' if layout == 'packed' else layout
    with Dev(h) as dev:
        if layout == 'packed':
            rows = np.full((T, N, PACK), POISON, F32)
            rows[:, :, PACK_R], rows[:, :, PACK_C] = r, c['cut'][:T]
            p, _ = put_rows(h, dev, rows.reshape(1, -1), 0, shift)
            t_r, t_c = (p + 4 * PACK_R, N * PACK, PACK), (p + 4 * PACK_C, N * PACK, PACK)
        else:
            t_r, t_c = _put_table(h, dev, r, layout, shift), _put_table(h, dev, c['cut'][:T], layout, (shift + 1) & 3)
        if succ == 'shift':
            p, ts, es = _put_table(h, dev, c['vtab'][:T + 1], inner, (shift + 2) & 3)
            t_v, t_vn = (p, ts, es), (p + 4 * ts, ts, es)
        else:
            t_v, t_vn = _put_table(h, dev, c['vtab'][:T], inner, (shift + 2) & 3), _put_table(h, dev, c['succ'][:T], inner, (shift + 3) & 3)
        t_t = _put_table(h, dev, c['term'][:T], inner, shift) if term else None
        o_adv, o_ret = _OutTable(dev, T, N, inner, (shift + 1) & 3, reverse), _OutTable(dev, T, N, 'env' if inner == 'time' else 'time', (shift + 2) & 3)
        g = h.gae_struct(T, N, gamma, lam, t_r, t_v, t_vn, o_adv.tab, t_c if cut else None, t_t, o_ret.tab if ret else None)
        h.gae_device(g)
        h.sync()
        return o_adv.read(), o_ret.read(written=ret)


def gae_want(c, gamma, lam, succ='own', cut=True, term=True, T=None):
    T = c['r'].shape[0] if T is None else T
    vn = c['succ'][:T] if succ == 'own' else c['vtab'][1:T + 1]
    return gae_model(c['r'][:T], c['vtab'][:T], vn, gamma, lam, c['cut'][:T] if cut else None, c['term'][:T] if term else None)


def case_gae(library, shapes=None):
    """bit for bit against the fmaf model: every T x N, the layouts, both ways of passing the successor's value, the optional tables, the ends of
    gamma and lambda; guarded outputs; a column does not depend on the others"""
    shapes = shapes or [(T, N) for T in GAE_T for N in GAE_N]
    seen = set()
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for k, (T, N) in enumerate(shapes):
            c = gae_inputs(T, N)
            seen |= {name for name, hit in (('cut at 0', c['cut'][0] != 0), ('cut mid', c['cut'][T // 2] != 0), ('cut at the end', c['cut'][T - 1] != 0),
                                            ('terminal with a cut', (c['term'] != 0) & (c['cut'] != 0)), ('terminal without', (c['term'] != 0) & (c['cut'] == 0)))
                     if np.any(hit)}
            runs = [dict(layout=('time', 'env', 'packed', 'tight')[k % 4], succ=('own', 'shift')[k & 1], shift=k % 4, reverse=k % 3 == 0),
                    dict(layout=('env', 'packed', 'tight', 'time')[k % 4], succ=('shift', 'own')[k & 1], shift=(k + 1) % 4)]
            if k % 5 == 0:
                runs += [dict(cut=False, term=False, ret=False), dict(gamma=0.0), dict(lam=0.0), dict(lam=1.0, gamma=1.0), dict(term=False, layout='packed')]
            for kw in runs:
                kw = dict(kw)
                gamma, lam = kw.pop('gamma', 0.98), kw.pop('lam', 0.95)
                adv, ret = device_gae(h, c, gamma, lam, **kw)
                want = gae_want(c, gamma, lam, kw.get('succ', 'own'), kw.get('cut', True), kw.get('term', True))
                eq_bits(adv, want[0], ('gae adv', T, N, kw))
                if ret is not None:
                    eq_bits(ret, want[1], ('gae ret', T, N, kw))
            if N > 1:                                              # other columns change, this one does not
                i0 = N // 2
                other = {key: np.array(v) for key, v in c.items()}
                rs = np.random.RandomState(k)
                for key in other:
                    keep = other[key][:, i0].copy()
                    other[key] = rs.permutation(other[key].ravel()).reshape(other[key].shape).astype(F32)
                    other[key][:, i0] = keep
                a0, r0 = device_gae(h, c, 0.98, 0.95)
                a1, r1 = device_gae(h, other, 0.98, 0.95)
                eq_bits(a1[:, i0], a0[:, i0], ('gae column', T, N))
                eq_bits(r1[:, i0], r0[:, i0], ('gae column', T, N))
                assert N < 3 or not np.array_equal(bits(a1), bits(a0))
    if len(shapes) == len(GAE_T) * len(GAE_N):
        assert seen == GAE_COVERAGE, seen
    return seen


GAE_COVERAGE = {'cut at 0', 'cut mid', 'cut at the end', 'terminal with a cut', 'terminal without'}


def reset_store_case():
    """One env, T = 5, an episode that ends behind step 2, a store filled the way a textbook loop fills it after an automatic reset: vtab[t] is
    the value of the state acted on at step t, so vtab[3] belongs to the NEW episode's first state; succ[2] is the value of the finished
    episode's last observation.  -> the inputs and the float64 reference of two separate episodes, each bootstrapped from its own last state"""
    r = np.array([[0.5], [-0.25], [1.0], [0.125], [-0.5]], F32)
    vtab = np.array([[0.3], [0.6], [-0.2], [2.0], [1.5], [0.9]], F32)           # vtab[3]: first state of episode 2
    succ = np.array([[0.6], [-0.2], [-0.7], [1.5], [0.9]], F32)                 # succ[2] = -0.7: the last observation of episode 1, not vtab[3]
    cut = np.array([[0], [0], [1], [0], [0]], F32)
    gamma, lam = 0.9, 0.8
    want = np.zeros(5)
    for lo, hi in ((0, 3), (3, 5)):                                              # the textbook recursion per episode, in float64
        run = 0.0
        for t in range(hi - 1, lo - 1, -1):
            delta = float(r[t, 0]) + gamma * float(succ[t, 0]) - float(vtab[t, 0])
            run = delta + (gamma * lam * run if t < hi - 1 else 0.0)
            want[t] = run
    return r, vtab, succ, cut, gamma, lam, want


# ----------------------------------------------------------------------------------------------------------------------
# the advantage normaliser
STATS_M = (1, 2, 255, 256, 257, 1025)


def stats_rows(M, seed=0):
    return TC.cached(('adv rows', M, seed), lambda: {'x': (np.random.RandomState(4200 + M + seed).standard_normal(M) * 3 + 1.5).astype(F32)})['x']


def chain256(x, dtype):
    """thread k: the elements b = k (mod 256) ascending from +0; then the 256 partial sums ascending from +0 -> total"""
    x = np.asarray(x, dtype)
    part = np.zeros(256, dtype)
    for lo in range(0, x.size, 256):
        blk = x[lo:lo + 256]
        part[:blk.size] = part[:blk.size] + blk
    total = dtype(0)
    for p in part:
        total = dtype(total + p)
    return total


def stats_model(x, eps=1e-8, ddof=0, fused=False):
    """-> mean (float32, bit-defined), 1 / (std + eps) as float32, the same in float64.  fused: S * mean enters the subtraction unrounded, as a
    build that contracts the expression forms it"""
    x = np.asarray(x, F32).astype(F64)
    M = x.size
    S, Q = chain256(x, F64), chain256(x * x, F64)                 # x * x is exact in double
    mean = S / M
    num = float(Fraction(float(Q)) - Fraction(float(S)) * Fraction(float(mean))) if fused else Q - S * mean
    var = max(num / (M - ddof), 0.0)
    with np.errstate(divide='ignore'):
        inv = np.float64(1.0) / (np.sqrt(var) + float(F32(eps)))
    return F32(mean), F32(inv), float(inv)


def apply_model(x, mean, inv):
    with np.errstate(over='ignore', invalid='ignore'):
        return ((np.asarray(x, F32) - F32(mean)) * F32(inv)).astype(F32)


def measure_inv_bar():
    """-> the largest relative distance of the float32 value of either build of the double model (S * mean fused or not) from the float64
    value of the other, over STATS_M and both ddof"""
    worst = 0.0
    for M in STATS_M:
        for ddof in (0, 1):
            if M - ddof < 1 or M == 1:
                continue
            a, b = stats_model(stats_rows(M), 1e-8, ddof), stats_model(stats_rows(M), 1e-8, ddof, fused=True)
            worst = max(worst, abs(float(a[1]) - b[2]) / b[2], abs(float(b[1]) - a[2]) / a[2])
    return worst


def device_adv(h, x, eps=1e-8, ddof=0, inplace=True, shift=0):
    """pmg_adv_stats_device, then pmg_adv_apply_device with the statistics left in device memory -> stats [2], y [M], x as it is afterwards"""
    M = x.size
    with Dev(h) as dev:
        o_x, o_y, o_s = Out(dev, 4 * M, 4 * shift), Out(dev, 4 * M, 4 * ((shift + 1) & 3)), Out(dev, 8, 4 * ((shift + 2) & 3))
        h.upload(o_x.ptr, np.asarray(x, F32))
        h.adv_stats_device(h.adv_stats_struct(M, o_x.ptr, o_s.ptr, eps, ddof))
        h.adv_apply_device(o_x.ptr, M, o_s.ptr, o_x.ptr if inplace else o_y.ptr)
        h.sync()
        return o_s.read(), o_x.read() if inplace else o_y.read(written=True), o_x.read()


def case_adv(library):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for k, M in enumerate(STATS_M):
            for ddof in (0, 1):
                if M - ddof < 1:
                    continue
                x = stats_rows(M)
                for inplace in (True, False):
                    stats, y, x_after = device_adv(h, x, 1e-8, ddof, inplace, shift=(k + ddof) % 4)
                    mean, inv, inv64 = stats_model(x, 1e-8, ddof)
                    eq_bits(stats[:1], np.array([mean], F32), ('mean', M, ddof))
                    if M == 1:                                    # var = 0: 1 / eps, through one double division
                        assert stats[1] == F32(1.0 / float(F32(1e-8))), stats
                    else:
                        err = abs(float(stats[1]) - inv64) / inv64
                        worst = max(worst, err)
                        assert err <= ADV_INV_TOL, ('1 / (std + eps)', M, ddof, err)
                    eq_bits(y, apply_model(x, stats[0], stats[1]), ('apply from the device\'s own statistics', M, ddof, inplace))
                    if not inplace:
                        eq_bits(x_after, x, 'the input of an out-of-place apply')
        # a constant input whose sums are exact: var is 0 exactly, the statistics are 1.5 and 1 / eps, the result +0.0
        for M in (2, 257, 1025):
            stats, y, _ = device_adv(h, np.full(M, 1.5, F32), 1e-5, 1)
            assert stats[0] == F32(1.5) and stats[1] == F32(1.0 / float(F32(1e-5))) and (bits(y) == 0).all(), (M, stats)
    print('1 / (std + eps) against float64: %.3g (bar %.3g)' % (worst, ADV_INV_TOL))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# the clipped-surrogate head: the numpy models
def _clamp32(v, lo, hi):
    return np.minimum(np.maximum(v, F32(lo)), F32(hi))


def head32(z, zo, n, adv, pscale, escale, clip_lo, clip_hi, lo, hi):
    """steps 1 - 6 in float32, the normative expression order, numpy's exp standing in for the build's -> dict(lr, rho, clipped, k, g_mu, g_ls,
    ghead, inr, w, isd, ls, lso, sdn)"""
    z, zo, n, adv = (np.asarray(v, F32) for v in (z, zo, n, adv))
    A = n.shape[1]
    with np.errstate(over='ignore', invalid='ignore'):
        m, raw = z[:, :A], z[:, A:]
        ls, inr = _clamp32(raw, lo, hi), (raw >= F32(lo)) & (raw <= F32(hi))
        lso = _clamp32(zo[:, A:], lo, hi)
        sdo = np.exp(lso)
        u = fmaf(sdo, n, zo[:, :A]).reshape(n.shape)
        lo_j = fmaf(F32(-0.5) * n, n, -lso).reshape(n.shape)
        isd = np.exp(-ls)
        w = (u - m) * isd
        ln_j = fmaf(F32(-0.5) * w, w, -ls).reshape(n.shape)
        d = ln_j - lo_j
        lr = np.zeros(n.shape[0], F32)
        for j in range(A):
            lr = lr + d[:, j]
        rho = np.exp(lr)
        res = head_tail(rho, adv, w, isd, inr, pscale, escale, clip_lo, clip_hi)
    res.update(lr=lr, rho=rho, inr=inr, w=w, isd=isd, ls=ls, lso=lso, sdn=sdo * n)
    return res


def head_tail(rho, adv, w, isd, inr, pscale, escale, clip_lo, clip_hi):
    """steps 5 and 6 from a given rho (the model's, or a device's own)"""
    with np.errstate(over='ignore', invalid='ignore'):
        clipped = ((adv > 0) & (rho > F32(clip_hi))) | ((adv < 0) & (rho < F32(clip_lo)))
        k = np.where(clipped, F32(0), (F32(pscale) * adv) * rho).astype(F32)
        kk = np.broadcast_to(k[:, None], w.shape)
        g_mu = kk * (w * isd)
        g_ls = np.where(inr, fmaf(kk, fmaf(w, w, -np.ones(w.shape, F32)).reshape(w.shape), np.full(w.shape, escale, F32)).reshape(w.shape), F32(0))
    return {'clipped': clipped, 'k': k, 'g_mu': g_mu.astype(F32), 'g_ls': g_ls.astype(F32), 'ghead': np.concatenate([g_mu, g_ls], 1).astype(F32)}


def head64(z, zo, n, adv, pscale, escale, clip_lo, clip_hi, lo, hi):
    """the float64 model from the same float32 inputs -> dict(lr, rho, clipped, g_mu, g_ls, inr, mag_lr, mag_mu, mag_ls)"""
    z, zo, n, adv = (np.asarray(v, F32).astype(F64) for v in (z, zo, n, adv))
    A = n.shape[1]
    lo, hi, clip_lo, clip_hi, pscale, escale = (float(F32(v)) for v in (lo, hi, clip_lo, clip_hi, pscale, escale))
    with np.errstate(over='ignore', invalid='ignore'):
        m, raw = z[:, :A], z[:, A:]
        ls, inr = np.clip(raw, lo, hi), (raw >= lo) & (raw <= hi)
        lso = np.clip(zo[:, A:], lo, hi)
        sdn = np.exp(lso) * n
        u = sdn + zo[:, :A]
        isd = np.exp(-ls)
        w = (u - m) * isd
        lr = ((-0.5 * w * w - ls) - (-0.5 * n * n - lso)).sum(1)
        rho = np.exp(lr)
        clipped = ((adv > 0) & (rho > clip_hi)) | ((adv < 0) & (rho < clip_lo))
        k = np.where(clipped, 0.0, pscale * adv * rho)[:, None]
        g_mu = k * w * isd
        g_ls = np.where(inr, k * (w * w - 1.0) + escale, 0.0)
        # first-order magnitudes: c = the weight of the cancellation in u - m on w
        c = isd * (np.abs(sdn) + np.abs(zo[:, :A]) + np.abs(m))
        mag_lr = (0.5 * w * w + np.abs(ls) + 0.5 * n * n + np.abs(lso) + np.abs(w) * c).sum(1)
        ak, one = np.abs(k), (1.0 + mag_lr)[:, None]
        mag_mu = ak * isd * (np.abs(w) * one + c)
        mag_ls = ak * ((w * w + 1.0) * one + 2.0 * np.abs(w) * c) + abs(escale)
    return {'lr': lr, 'rho': rho, 'clipped': clipped, 'g_mu': g_mu, 'g_ls': g_ls, 'inr': inr, 'mag_lr': mag_lr, 'mag_mu': mag_mu, 'mag_ls': mag_ls, 'raw': raw,
            'raw_old': zo[:, A:]}


def _rel(got, want, mag):
    """largest |got - want| / mag; where mag is 0 the two must be equal"""
    got, want, mag = np.asarray(got, F64), np.asarray(want, F64), np.asarray(mag, F64)
    assert np.array_equal(got[mag == 0], want[mag == 0])
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.where(mag > 0, np.abs(got - want) / mag, 0.0)
    return float(err.max()) if err.size else 0.0


def head_errors(got, w64):
    """the four relative errors of lr, rho, g_mu, g_ls (dict or model) against the float64 model"""
    A = w64['g_mu'].shape[1]
    g_mu, g_ls = (got['ghead'][:, :A], got['ghead'][:, A:]) if got.get('ghead') is not None else (w64['g_mu'], w64['g_ls'])
    return (_rel(got['lr'], w64['lr'], w64['mag_lr']), _rel(got['rho'], w64['rho'], w64['rho'] * (1.0 + w64['mag_lr'])),
            _rel(g_mu, w64['g_mu'], w64['mag_mu']), _rel(np.where(w64['inr'], g_ls, 0.0), w64['g_ls'], np.where(w64['inr'], w64['mag_ls'], 0.0)))


def clamp_of(k):
    """the clamp case k starts from: two narrow ones that the raw log-stds of every case leave on both sides"""
    return (-2.0, 0.5) if k % 2 == 0 else (-4.0, 1.0)


def margins_ok(w64, adv, lo, hi, clip_lo=CLIP_LO, clip_hi=CLIP_HI):
    """-> (rows whose rho is too close to an end of the clip, any raw log-std too close to an end of the clamp, any |adv| too small)"""
    near = (np.abs(w64['rho'] - clip_lo) < RHO_MARGIN * clip_lo) | (np.abs(w64['rho'] - clip_hi) < RHO_MARGIN * clip_hi) | ~np.isfinite(w64['rho'])
    raws = np.concatenate([w64['raw'].ravel(), w64['raw_old'].ravel()])
    tight = bool((np.minimum(np.abs(raws - float(F32(lo))), np.abs(raws - float(F32(hi)))) < LS_MARGIN).any())
    return near, tight, bool((np.abs(np.asarray(adv, F64)) < ADV_MARGIN).any())


def old_policy(z, A, rs, lo, hi, B, scales=(0.02, 0.1, 0.3, 0.8)):
    """the recorded side of a case: n, adv and a zo near z -- per row a scale of the distance, so that ratios far from 1 and close to it both
    occur; rows whose rho falls within the margin of the clip are moved closer to z, a clamp within the margin of a log-std is widened"""
    n = rs.standard_normal((B, A)).astype(F32)
    adv = (rs.choice([-1.0, 1.0], B) * (ADV_MARGIN + np.abs(rs.standard_normal(B)))).astype(F32)
    scale = rs.choice(scales, B) / np.sqrt(A)
    dmu, dls = rs.uniform(-1, 1, (B, A)), rs.uniform(-1, 1, (B, A))
    for _ in range(200):
        lo, hi = float(F32(lo)), float(F32(hi))
        sd = np.exp(np.clip(z[:, A:].astype(F64), lo, hi))
        zo = np.concatenate([z[:, :A] + scale[:, None] * dmu * sd, z[:, A:] + 0.3 * scale[:, None] * dls], 1).astype(F32)
        w64 = head64(z, zo, n, adv, -1.0 / B, -ENT_COEF / B, CLIP_LO, CLIP_HI, lo, hi)
        near, tight, small = margins_ok(w64, adv, lo, hi)
        assert not small
        if tight:
            lo, hi = lo - 0.0137, hi + 0.0071
        elif near.any():
            scale[near] *= 0.8
        else:
            return zo, n, adv, lo, hi
    raise AssertionError('no margins found')


def ppo_case(k):
    """case k of CASES: sac_cases' actor for (Dx, A, hidden) (without its biases where bias is False), its rows and the chain model's z, and the
    recorded side"""
    Dx, A, hidden, bias, B, R = CASES[k]

    def make():
        m = SC.sample_case(Dx, A, hidden)
        Ws, bs = [w.copy() for w in m['Ws']], ([b.copy() for b in m['bs']] if bias else None)
        if not bias:                                              # keep the log-stds spread over the clamp
            Ws[-1][A:] = Ws[-1][A:] * F32(0.25)
        x = m['x'][:B]
        z = forward(x, Ws, bs)
        zo, n, adv, lo, hi = old_policy(z, A, np.random.RandomState(3100 + k), *clamp_of(k), B)
        return {'Ws': Ws, 'bs': bs, 'x': x, 'z': z, 'zo': zo, 'n': n, 'adv': adv, 'lo': lo, 'hi': hi, 'pscale': float(F32(-1.0 / B)),
                'escale': float(F32(-ENT_COEF / B))}
    return TC.cached(('ppo', k), make)


def head_args(c):
    return (c['zo'], c['n'], c['adv'], c['pscale'], c['escale'], CLIP_LO, CLIP_HI, c['lo'], c['hi'])


def measure_head_bars(cases=range(len(CASES))):
    """-> the largest relative errors of lr, rho, g_mu, g_ls of head32 against head64 over the cases' own inputs, having asserted that both
    took the same branches"""
    worst = [0.0] * 4
    for k in cases:
        c = ppo_case(k)
        m, w = head32(c['z'], *head_args(c)), head64(c['z'], *head_args(c))
        assert np.array_equal(m['clipped'], w['clipped']) and np.array_equal(m['inr'], w['inr'])
        worst = [max(a, b) for a, b in zip(worst, head_errors(m, w))]
    return worst


COVERAGE = {'clipped high', 'clipped low', 'unclipped below 1', 'unclipped above 1', 'new below', 'new inside', 'new above', 'old below', 'old inside',
            'old above'}


def coverage_of(rho, clipped, adv, raw, raw_old, lo, hi):
    hits = (('clipped high', clipped & (adv > 0) & (rho > CLIP_HI)), ('clipped low', clipped & (adv < 0) & (rho < CLIP_LO)),
            ('unclipped below 1', ~clipped & (rho < 1)), ('unclipped above 1', ~clipped & (rho > 1)),
            ('new below', raw < lo), ('new inside', (raw > lo) & (raw < hi)), ('new above', raw > hi),
            ('old below', raw_old < lo), ('old inside', (raw_old > lo) & (raw_old < hi)), ('old above', raw_old > hi))
    return {name for name, hit in hits if np.any(hit)}


def model_coverage(cases=range(len(CASES))):
    seen = set()
    for k in cases:
        c = ppo_case(k)
        w = head64(c['z'], *head_args(c))
        seen |= coverage_of(w['rho'], w['clipped'], c['adv'], w['raw'], w['raw_old'], c['lo'], c['hi'])
    return seen


# ----------------------------------------------------------------------------------------------------------------------
# float64 autograd and the float32 model of steps 1 - 7 (CPU only: tests/test_ppo_host.py; the device is then held to the same bar)
MODEL_NETS = ((6, 256, 256, 256, 6), (5, 33, 8))
MODEL_B = 33


def model_case(k):
    def make():
        widths = MODEL_NETS[k]
        A = widths[-1] // 2
        Ws, bs = GC.net(3300 + k, widths)
        bs[-1][A:] = bs[-1][A:] - F32(1)
        Ws[-1][A:] = Ws[-1][A:] * F32(16 if len(widths) > 3 else 4)   # raw log-stds on both sides of the clamp
        x = np.random.RandomState(330 + k).uniform(-2, 2, (MODEL_B, widths[0])).astype(F32)
        z = forward(x, Ws, bs)
        zo, n, adv, lo, hi = old_policy(z, A, np.random.RandomState(3310 + k), -2.0, 0.5, MODEL_B, (0.1, 0.5, 1.0))
        return {'Ws': Ws, 'bs': bs, 'x': x, 'z': z, 'zo': zo, 'n': n, 'adv': adv, 'lo': lo, 'hi': hi, 'pscale': float(F32(-1.0 / MODEL_B)),
                'escale': float(F32(-ENT_COEF / MODEL_B))}
    return TC.cached(('ppo model', k), make)


def autograd64(Ws, bs, x, zo, n, adv, pscale, escale, clip_lo, clip_hi, lo, hi):
    """float64 torch autograd of the textbook loss pscale sum min(rho A, clamp(rho) A) + escale sum ls -> dict(dW, db, masks, inrange, clipped, rho)"""
    import torch
    t64 = lambda v: torch.tensor(np.asarray(v, F32).astype(F64))
    pa = [(t64(W).requires_grad_(), t64(b).requires_grad_()) for W, b in zip(Ws, bs)]
    lo, hi, clip_lo, clip_hi, pscale, escale = (float(F32(v)) for v in (lo, hi, clip_lo, clip_hi, pscale, escale))
    masks = []
    hh = t64(x)
    for l, (W, b) in enumerate(pa):
        hh = hh @ W.T + b
        if l + 1 < len(pa):
            masks.append((hh > 0).numpy())
            hh = torch.relu(hh)
    A = Ws[-1].shape[0] // 2
    raw = hh[:, A:]
    m, ls = hh[:, :A], torch.clamp(raw, lo, hi)
    zo_t, nn, aa = t64(zo), t64(n), t64(adv)
    lso = torch.clamp(zo_t[:, A:], lo, hi)
    u = zo_t[:, :A] + torch.exp(lso) * nn
    w = (u - m) * torch.exp(-ls)
    lr = ((-0.5 * w * w - ls) - (-0.5 * nn * nn - lso)).sum(1)
    rho = torch.exp(lr)
    surrogate = torch.minimum(rho * aa, torch.clamp(rho, clip_lo, clip_hi) * aa)
    (pscale * surrogate.sum() + escale * ls.sum()).backward()
    rho_n = rho.detach().numpy()
    return {'dW': [W.grad.numpy() for W, _ in pa], 'db': [b.grad.numpy() for _, b in pa], 'masks': masks,
            'inrange': ((raw >= lo) & (raw <= hi)).detach().numpy(), 'rho': rho_n,
            'clipped': ((np.asarray(adv) > 0) & (rho_n > clip_hi)) | ((np.asarray(adv) < 0) & (rho_n < clip_lo))}


def model32(Ws, bs, x, zo, n, adv, pscale, escale, clip_lo, clip_hi, lo, hi):
    """the numpy float32 model of steps 1 - 7: the chain, head32, the exact chains of grad_cases for the backward"""
    z = forward(x, Ws, bs)
    hd = head32(z, zo, n, adv, pscale, escale, clip_lo, clip_hi, lo, hi)
    m = GC.model(x, Ws, bs, gout=hd['ghead'])
    return dict(hd, dW=m['dW'], db=m['db'], masks=m['masks'])


def model_args(c):
    return (c['Ws'], c['bs'], c['x']) + head_args(c)


def measure_model_bar():
    """-> the largest error of model32 against autograd64 over MODEL_NETS, having asserted that both took the same branches and that every
    branch occurs"""
    worst = 0.0
    for k in range(len(MODEL_NETS)):
        c = model_case(k)
        w, m = autograd64(*model_args(c)), model32(*model_args(c))
        assert all(np.array_equal(u, v) for u, v in zip(w['masks'], m['masks'])), 'ReLU masks differ'
        assert np.array_equal(w['inrange'], m['inr']) and np.array_equal(w['clipped'], m['clipped'])
        assert w['clipped'].any() and not w['clipped'].all() and w['inrange'].any() and not w['inrange'].all()
        worst = max(worst, SC.recipe_error(m['dW'], m['db'], w['dW'], w['db']))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# device calls
OUTPUTS = ('ratio', 'logratio', 'clipped', 'ghead')


def device_ppo(h, Ws, bs, x, zo, n, adv, pscale, escale, clip_lo=CLIP_LO, clip_hi=CLIP_HI, lo=SC.LS_LO, hi=SC.LS_HI, grads=True, null=(), pad=0, shift=0,
               R=None, twice=False, nan_work=False):
    """pmg_ppo_policy_grad_device on canary-framed, sentinel-filled outputs -> dict(dW, db, ratio, logratio, clipped, ghead) (None for what was
    passed as NULL).  pad: floats of poison behind every input row and of sentinel between output rows; shift: the phase of the first float
    pointer, the others follow in turn.  The workspace is sized EXACTLY pmg_ppo_policy_grad_work_floats and canary-framed; with grads NULL it
    must come back untouched.  nan_work: it starts as NaN bit patterns."""
    B, A = x.shape[0], Ws[-1].shape[0] // 2
    with Dev(h) as dev:
        actor = Net(h, dev, Ws, bs, 0)
        d_x, xs = put_rows(h, dev, x, pad, shift)
        d_zo, zos = put_rows(h, dev, np.asarray(zo, F32), pad, (shift + 1) & 3)
        d_n, ns = put_rows(h, dev, np.asarray(n, F32), pad, (shift + 2) & 3)
        d_adv, _ = put_rows(h, dev, np.asarray(adv, F32)[None, :], 0, (shift + 3) & 3)
        outs = {'ratio': Out(dev, 4 * B, 4 * ((shift + 1) & 3)), 'logratio': Out(dev, 4 * B, 4 * ((shift + 2) & 3)), 'clipped': Out(dev, B, 1 + (shift & 3)),
                'ghead': rows_out(dev, B, 2 * A, pad, (shift + 3) & 3)}
        par = Params(h, dev, Ws, bs, shift)
        work = h.ppo_policy_grad_work_floats(actor.mlp, B, R or 0)
        assert work == (h.mlp_grad_chunked_work_floats(actor.mlp, B, R) if R else h.mlp_grad_work_floats(actor.mlp, B)) and work >= 0
        o_work = Out(dev, 4 * work, 4 * ((shift + 1) & 3))
        if nan_work and work:
            h.upload(o_work.ptr, np.full(work, NAN_WORD, np.uint32))
        ptr = lambda k: None if k in null else outs[k].ptr
        g = h.ppo_policy_grad_struct(B, d_x, xs, d_zo, zos, d_n, ns, d_adv, pscale, escale, clip_lo, clip_hi, lo, hi, par.struct if grads else None,
                                     ptr('ratio'), ptr('logratio'), ptr('clipped'), ptr('ghead'), 2 * A + pad, o_work.ptr, work)
        for _ in range(2 if twice else 1):
            h.ppo_policy_grad_device(actor.mlp, g, R or 0)
        h.sync()
        raw = o_work.read(np.uint32 if work else np.uint8)            # (the canaries around it are checked)
        if not grads and work:
            fill = NAN_WORD if nan_work else int(np.array([SENTINEL] * 4, np.uint8).view(np.uint32)[0])
            assert (raw == fill).all(), 'without grads the workspace was written'
        dW, db = par.read(written=grads)
        res = {'dW': dW, 'db': db, 'ghead': read_rows(outs['ghead'], B, 2 * A, pad, 'ghead' not in null)}
        for k in ('ratio', 'logratio'):
            res[k] = outs[k].read(written=k not in null)
        cl = outs['clipped'].read(np.uint8, written='clipped' not in null)
        assert cl is None or set(cl.tolist()) <= {0, 1}, 'd_clipped holds something else than 0 / 1'
        res['clipped'] = None if cl is None else cl.astype(bool)
        for p, W in zip(actor.d_w, Ws):                                # the actor's weights are not written
            assert np.array_equal(bits(dev.get(p, W.shape, F32)), bits(W)), 'a weight was written'
        return res


def run_case(h, c, R=None, **kw):
    return device_ppo(h, c['Ws'], c['bs'], c['x'], c['zo'], c['n'], c['adv'], c['pscale'], c['escale'], CLIP_LO, CLIP_HI, c['lo'], c['hi'], R=R, **kw)


def actor_grad(h, c, ghead, R=None):
    """the EXISTING call the gradient is defined by: pmg_mlp_grad[_chunked]_device of the actor on a given d_gout"""
    if R is None or R >= c['x'].shape[0]:
        return GC.device_grad(h, c['Ws'], c['bs'], c['x'], None, 0, gout=ghead, null=('gx',))
    return GCC.device_grad_chunked(h, c['Ws'], c['bs'], c['x'], R, None, 0, gout=ghead, null=('gx',))


def check_head(got, c, label):
    """d_clipped from the call's own rho, bit for bit; lr, rho, g_mu, g_ls against the float32 model within the bars -> the four errors"""
    m = head32(c['z'], *head_args(c))
    w = head64(c['z'], *head_args(c))
    own = head_tail(got['ratio'], c['adv'], m['w'], m['isd'], m['inr'], c['pscale'], c['escale'], CLIP_LO, CLIP_HI)
    assert np.array_equal(got['clipped'], own['clipped']), (label, 'd_clipped is not the predicate on the call\'s own rho')
    assert np.array_equal(got['clipped'], m['clipped']), (label, 'the device and the model disagree on a clip despite the margin')
    A = c['n'].shape[1]
    assert (bits(got['ghead'][:, A:][~m['inr']]) == 0).all(), (label, 'g_ls is +0.0 outside the clamp')
    assert (bits(got['ghead'][:, :A][m['clipped']] + F32(0)) == 0).all(), (label, 'g_mu is zero where the clip cut')
    e32 = {'lr': got['logratio'], 'rho': got['ratio'], 'ghead': got['ghead']}
    mags = dict(w, lr=m['lr'].astype(F64), rho=m['rho'].astype(F64), g_mu=m['g_mu'].astype(F64), g_ls=m['g_ls'].astype(F64))   # the float32 model as the reference
    errs = head_errors(e32, mags)
    for name, err, tol in zip(('lr', 'rho', 'g_mu', 'g_ls'), errs, (PPO_LR_TOL, PPO_RHO_TOL, PPO_MU_TOL, PPO_LS_TOL)):
        assert err <= tol, (label, name, err, tol)
    return errs


# 1. against existing calls and the float32 model
def case_sequence(library, cases=range(len(CASES))):
    seen, worst = set(), [0.0] * 4
    cases = list(cases)
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for k in cases:
            Dx, A, hidden, bias, B, R = CASES[k]
            c = ppo_case(k)
            # z: pmg_mlp_forward_device's; recorded as zo with n = 0 the two policies are the same function at the same point
            zf = AC.device_forward(h, c['Ws'], c['bs'], c['x'])
            SC.check_z(zf, c['z'], (k, 'z'))
            same = device_ppo(h, c['Ws'], c['bs'], c['x'], zf, np.zeros((B, A), F32), c['adv'], c['pscale'], 0.0, CLIP_LO, CLIP_HI, c['lo'], c['hi'], grads=False,
                              shift=(k + 1) % 4)
            assert (bits(same['logratio']) == 0).all() and (same['ratio'] == 1).all() and not same['clipped'].any(), (k, 'z is not pmg_mlp_forward_device\'s')
            assert not same['ghead'][:, :A].any(), (k, 'g_mu is not zero at the recorded point')
            got = run_case(h, c, R, pad=k % 3, shift=k % 4, nan_work=bool(k & 1))
            worst = [max(a, b) for a, b in zip(worst, check_head(got, c, k))]
            GC.check(got, actor_grad(h, c, got['ghead'], R), (k, 'dW / db from the own d_ghead'), ('dW', 'db'))
            seen |= coverage_of(got['ratio'], got['clipped'], c['adv'], c['z'][:, A:], c['zo'][:, A:], F32(c['lo']), F32(c['hi']))
    print('head: largest relative errors of lr, rho, g_mu, g_ls against the float32 model = %.3g %.3g %.3g %.3g (bars %.3g %.3g %.3g %.3g)'
          % (tuple(worst) + (PPO_LR_TOL, PPO_RHO_TOL, PPO_MU_TOL, PPO_LS_TOL)))
    if len(cases) == len(CASES):
        assert seen == COVERAGE, seen
    return worst, seen


# 2. the device against float64 autograd
def case_autograd(library):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for k in range(len(MODEL_NETS)):
            c = model_case(k)
            got = run_case(h, c)
            w = autograd64(*model_args(c))
            assert np.array_equal(w['clipped'], got['clipped']), 'the device clipped other rows than float64'
            worst = max(worst, SC.recipe_error(got['dW'], got['db'], w['dW'], w['db']))
    print('the fused PPO actor gradient against float64 autograd: %.3g (bar %.3g)' % (worst, PPO_TOL))
    assert worst <= PPO_TOL, worst
    return worst


# 3. the sampler's own records on the same weights: the ratio is 1
def case_same_weights(library, pairs=PAIRS):
    """lr is 0 and rho is 1 within their own bars, each against its own magnitude as in check_head (the float64 model is 0 to 1e-16: with
    zo == z, u - m is sd n exactly), and nothing is clipped"""
    worst = [0.0, 0.0]
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for i, (Dx, A) in enumerate(pairs):
            m = SC.sample_case(Dx, A, SC.HIDDEN[i % 3])
            B = BATCHES[(i + 2) % len(BATCHES)]
            x, z = m['x'][:B], m['z'][:B]
            lo, hi = -4.0, 1.0
            s = SC.device_sample(h, m['Ws'], m['bs'], x, lo, hi, 1, 11 + i, 5, 2 * i)
            adv = (np.random.RandomState(i).choice([-1.0, 1.0], B) * 1.5).astype(F32)
            got = device_ppo(h, m['Ws'], m['bs'], x, s['z'], s['n'], adv, -1.0 / B, -ENT_COEF / B, CLIP_LO, CLIP_HI, lo, hi, grads=False, pad=1, shift=i % 4)
            w = head64(z, s['z'], s['n'], adv, -1.0 / B, -ENT_COEF / B, CLIP_LO, CLIP_HI, lo, hi)
            assert np.abs(w['lr']).max() <= 1e-12 * w['mag_lr'].max(), 'the float64 model of the same policy twice is not 0'
            e_lr, e_rho = _rel(got['logratio'], 0.0 * w['lr'], w['mag_lr']), _rel(got['ratio'], 1.0 + 0.0 * w['lr'], 1.0 + w['mag_lr'])
            worst = [max(a, b) for a, b in zip(worst, (e_lr, e_rho))]
            assert e_lr <= PPO_LR_TOL, ((Dx, A), 'lr is not 0 on the same weights', e_lr)
            assert e_rho <= PPO_RHO_TOL, ((Dx, A), 'rho is not 1 on the same weights', e_rho)
            assert not got['clipped'].any(), ((Dx, A), 'a row was clipped on the same weights')
    print('the same weights: largest |lr| / magnitude = %.3g (bar %.3g), |rho - 1| / magnitude = %.3g (bar %.3g)' % (worst[0], PPO_LR_TOL, worst[1], PPO_RHO_TOL))
    return worst


# 4. edges
def case_edges(library):
    nan = float('nan')
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        # a NaN advantage: the row is not clipped, rho and lr are what they were, g is NaN where the formulas say and +0.0 outside the clamp
        c = ppo_case(0)
        A, B = c['n'].shape[1], c['x'].shape[0]
        base = run_case(h, c, grads=False)
        rows = np.array([0, 31, 32, 100])
        adv = c['adv'].copy()
        adv[rows] = nan
        got = run_case(h, dict(c, adv=adv), grads=False, shift=1)
        m = head32(c['z'], c['zo'], c['n'], adv, *head_args(c)[3:])
        for key in ('ratio', 'logratio'):
            eq_bits(got[key], base[key], ('NaN adv', key))
        assert not got['clipped'][rows].any() and np.array_equal(np.delete(got['clipped'], rows), np.delete(base['clipped'], rows))
        assert np.isnan(got['ghead'][rows][:, :A]).all() and np.array_equal(np.isnan(got['ghead'][rows][:, A:]), m['inr'][rows])
        assert (bits(got['ghead'][rows][:, A:][~m['inr'][rows]]) == 0).all()
        eq_bits(np.delete(got['ghead'], rows, 0), np.delete(base['ghead'], rows, 0), 'NaN adv: the other rows')
        # a NaN z: a linear actor passes the NaN of an input on.  lr and rho are NaN, nothing is clipped, g_mu is NaN, g_ls +0.0 (NaN is outside)
        c = ppo_case(6)
        A, B = c['n'].shape[1], c['x'].shape[0]
        base = run_case(h, c, grads=False)
        x = c['x'].copy()
        x[rows, 0] = nan
        with np.errstate(invalid='ignore'):
            got = run_case(h, dict(c, x=x), grads=False, shift=2)
        assert np.isnan(got['ratio'][rows]).all() and np.isnan(got['logratio'][rows]).all() and not got['clipped'][rows].any()
        assert np.isnan(got['ghead'][rows][:, :A]).all() and (bits(got['ghead'][rows][:, A:]) == 0).all()
        for key in OUTPUTS:
            eq_bits(np.delete(got[key], rows, 0).astype(F32), np.delete(base[key], rows, 0).astype(F32), ('NaN z: the other rows', key))
        # an open clip (0, +inf): nothing is clipped; a clip that is one point: every row whose rho is not exactly there is cut on one side
        wide = device_ppo(h, c['Ws'], c['bs'], c['x'], c['zo'], c['n'], c['adv'], c['pscale'], c['escale'], 0.0, INF, c['lo'], c['hi'], grads=False)
        assert not wide['clipped'].any()
        eq_bits(wide['ratio'], base['ratio'], 'the clip does not enter rho')
        point = device_ppo(h, c['Ws'], c['bs'], c['x'], c['zo'], c['n'], c['adv'], c['pscale'], c['escale'], 1.0, 1.0, c['lo'], c['hi'], grads=False)
        m = head32(c['z'], c['zo'], c['n'], c['adv'], c['pscale'], c['escale'], 1.0, 1.0, c['lo'], c['hi'])
        assert np.array_equal(point['clipped'], head_tail(point['ratio'], c['adv'], m['w'], m['isd'], m['inr'], c['pscale'], c['escale'], 1.0, 1.0)['clipped'])
        assert point['clipped'].any() and not point['clipped'].all()
        # escale alone (pscale = 0): g_mu is zero, g_ls is escale inside the clamp, and dW / db are the chain's on that head
        ent = device_ppo(h, c['Ws'], c['bs'], c['x'], c['zo'], c['n'], c['adv'], 0.0, -0.125, CLIP_LO, CLIP_HI, c['lo'], c['hi'])
        inr = (c['z'][:, A:] >= F32(c['lo'])) & (c['z'][:, A:] <= F32(c['hi']))
        assert not ent['ghead'][:, :A].any()
        eq_val(ent['ghead'][:, A:], np.where(inr, F32(-0.125), F32(0)), 'the entropy term alone')
        GC.check(ent, GC.model(c['x'], c['Ws'], c['bs'], gout=ent['ghead']), 'the entropy term alone', ('dW', 'db'))


# 5. stale tile
def case_stale_tile(library):
    """sac_cases.stale_actor: a hidden layer leaves 1e31 / inf in column 33 of the tile, beyond the 2 A = 8 columns of the head; B = 33, so the
    second tile has one row of the batch and 31 past it.  Every output against the model; row 32 alone gives the bits it has in the batch"""
    B = TILE + 1
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for regime in ('huge', 'inf'):
            s = SC.stale_actor(regime, B, 'actor')
            A = s['Ws'][-1].shape[0] // 2
            zo, n, adv, lo, hi = old_policy(s['z'], A, np.random.RandomState(3400), -2.0, 0.5, B)
            c = {'Ws': s['Ws'], 'bs': s['bs'], 'x': s['x'], 'z': s['z'], 'zo': zo, 'n': n, 'adv': adv, 'lo': lo, 'hi': hi, 'pscale': float(F32(-1.0 / B)),
                 'escale': float(F32(-ENT_COEF / B))}
            grads = regime == 'huge'                               # (with inf activations dW is inf or NaN by its definition)
            with np.errstate(over='ignore', invalid='ignore'):
                got = run_case(h, c, grads=grads, pad=1, nan_work=True)
                check_head(got, c, ('stale', regime))
                assert np.isfinite(got['ghead']).all() and np.isfinite(got['ratio']).all(), regime
                if grads:
                    GC.check(got, GC.model(c['x'], c['Ws'], c['bs'], gout=got['ghead']), ('stale', regime), ('dW', 'db'))
                one = device_ppo(h, c['Ws'], c['bs'], c['x'][TILE:], zo[TILE:], n[TILE:], adv[TILE:], c['pscale'], c['escale'], CLIP_LO, CLIP_HI, lo, hi, grads=False)
            for key in OUTPUTS:
                eq_bits(one[key].astype(F32), got[key][TILE:].astype(F32), (regime, 'row 32 alone', key))


# 6. properties
def case_properties(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for k in (0, 6):
            Dx, A, hidden, bias, B, R = CASES[k]
            c = ppo_case(k)
            big = run_case(h, c, pad=1, shift=1)
            # a row alone, in a tile of its own and inside its batch
            for lo_, hi_ in ((0, 1), (32, 33), (100, 101), (0, 33), (40, 101)):
                sub = device_ppo(h, c['Ws'], c['bs'], c['x'][lo_:hi_], c['zo'][lo_:hi_], c['n'][lo_:hi_], c['adv'][lo_:hi_], c['pscale'], c['escale'], CLIP_LO,
                                 CLIP_HI, c['lo'], c['hi'], grads=False, shift=2)
                for key in OUTPUTS:
                    assert np.array_equal(bits(sub[key].astype(F32)), bits(big[key][lo_:hi_].astype(F32))), (key, lo_, 'a row depends on its batch')
            again = run_case(h, c, pad=1, shift=1, twice=True)
            for key in OUTPUTS:
                eq_bits(again[key].astype(F32), big[key].astype(F32), (key, 'two calls differ'))
            for u, v in zip(big['dW'] + [t for t in big['db'] if t is not None], again['dW'] + [t for t in again['db'] if t is not None]):
                eq_bits(u, v, 'two calls differ in dW / db')
            # a permutation of the rows
            perm = np.random.RandomState(5).permutation(B)
            cp = dict(c, x=np.ascontiguousarray(c['x'][perm]), zo=np.ascontiguousarray(c['zo'][perm]), n=np.ascontiguousarray(c['n'][perm]),
                      adv=np.ascontiguousarray(c['adv'][perm]))
            rev = run_case(h, cp)
            for key in OUTPUTS:
                assert np.array_equal(bits(rev[key].astype(F32)), bits(big[key][perm].astype(F32))), (key, 'a row depends on its place')
            GC.check(rev, GC.model(cp['x'], c['Ws'], c['bs'], gout=rev['ghead']), 'permuted', ('dW', 'db'))
            GC.check(big, GC.model(c['x'], c['Ws'], c['bs'], gout=big['ghead']), 'in order', ('dW', 'db'))
            assert any(not np.array_equal(bits(u), bits(v)) for u, v in zip(rev['dW'], big['dW']))
            # chunks: another chain, the model's
            for R_ in (2, 32, 128):
                ch = run_case(h, c, R_, nan_work=True)
                for key in OUTPUTS:
                    eq_bits(ch[key].astype(F32), big[key].astype(F32), (key, R_))
                w = GCC.chunk_model(c['x'], c['Ws'], c['bs'], R_, gout=ch['ghead']) if R_ < B else GC.model(c['x'], c['Ws'], c['bs'], gout=ch['ghead'])
                GC.check(ch, w, ('chunks', R_), ('dW', 'db'))
            # every optional output NULL in turn (and all of them) with grads; grads NULL with each output alone and with all
            for null in (('ratio',), ('logratio',), ('clipped',), ('ghead',), OUTPUTS):
                got = run_case(h, c, null=null, shift=3)
                for key in OUTPUTS:
                    assert (got[key] is None) == (key in null)
                    if got[key] is not None:
                        eq_bits(got[key].astype(F32), big[key].astype(F32), ('NULL', null, key))
                GC.check(got, big, ('NULL', null), ('dW', 'db'))
            for keep in (('ratio',), ('logratio',), ('clipped',), ('ghead',), OUTPUTS):
                got = run_case(h, c, grads=False, null=tuple(o for o in OUTPUTS if o not in keep), pad=2, nan_work=bool(len(keep) & 1))
                assert got['dW'] is None and got['db'] is None
                for key in keep:
                    eq_bits(got[key].astype(F32), big[key].astype(F32), ('grads NULL', keep, key))


# 7. the statistics of a minibatch
STAT_BATCHES = (1, 255, 256, 257)


def ppo_stats_model(rho, lr, clipped, adv, clip_lo=CLIP_LO, clip_hi=CLIP_HI):
    rho, lr, adv = (np.asarray(v, F32) for v in (rho, lr, adv))
    B = F32(len(rho))
    cr = np.minimum(np.maximum(rho, F32(clip_lo)), F32(clip_hi))
    terms = ((rho - F32(1)) - lr, np.where(np.asarray(clipped) != 0, F32(1), F32(0)), np.minimum(rho * adv, cr * adv), lr)
    return np.array([F32(F64(chain256(t.astype(F32), F32)) / F64(B)) for t in terms], F32)


def stats_inputs(B):
    def make():
        rs = np.random.RandomState(4400 + B)
        lr = (rs.standard_normal(B) * 0.3).astype(F32)
        rho = np.exp(lr).astype(F32)
        adv = rs.standard_normal(B).astype(F32)
        clipped = ((adv > 0) & (rho > F32(CLIP_HI))) | ((adv < 0) & (rho < F32(CLIP_LO)))
        return {'rho': rho, 'lr': lr, 'adv': adv, 'clipped': clipped.astype(np.uint8) * rs.choice([1, 7, 255], B).astype(np.uint8)}   # any non-zero byte counts
    return TC.cached(('ppo stats', B), make)


def device_ppo_stats(h, s, clip_lo=CLIP_LO, clip_hi=CLIP_HI, shift=0):
    B = len(s['rho'])
    with Dev(h) as dev:
        ptrs = [put_rows(h, dev, np.asarray(s[k], F32)[None, :], 0, (shift + i) & 3)[0] for i, k in enumerate(('rho', 'lr', 'adv'))]
        d_cl = dev.put(np.concatenate([np.zeros(3, np.uint8), s['clipped']])) + 3              # bytes: any alignment
        out = Out(dev, 16, 4 * ((shift + 1) & 3))
        h.ppo_stats_device(h.ppo_stats_struct(B, ptrs[0], ptrs[1], d_cl, ptrs[2], out.ptr, clip_lo, clip_hi))
        h.sync()
        return out.read()


def case_stats(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for k, B in enumerate(STAT_BATCHES):
            s = stats_inputs(B)
            eq_bits(device_ppo_stats(h, s, shift=k % 4), ppo_stats_model(s['rho'], s['lr'], s['clipped'], s['adv']), ('ppo stats', B))
        # from the rows kernel's own outputs
        c = ppo_case(0)
        got = run_case(h, c, grads=False)
        s = {'rho': got['ratio'], 'lr': got['logratio'], 'adv': c['adv'], 'clipped': got['clipped'].astype(np.uint8)}
        st = device_ppo_stats(h, s)
        eq_bits(st, ppo_stats_model(s['rho'], s['lr'], s['clipped'], s['adv']), 'ppo stats of a minibatch')
        assert st[0] > 0 and 0 < st[1] < 1                      # rho - 1 - log rho is positive; some rows are clipped, not all


# 8. the faces
def case_host_face(library):
    import pytest
    env = AC.stepped(library, 'reach', 8)
    ppo, pi = env.ppo, env.gaussian_actor
    assert ppo is env.ppo
    # GAE and the normaliser round-trip the cases
    c = gae_inputs(7, 65)
    adv, ret = ppo.gae(c['r'], c['vtab'][:7], c['succ'], 0.98, 0.95, c['cut'], c['term'])
    want = gae_model(c['r'], c['vtab'][:7], c['succ'], 0.98, 0.95, c['cut'], c['term'])
    eq_bits(adv, want[0], 'gae face')
    eq_bits(ret, want[1], 'gae face')
    adv2, _ = ppo.gae(c['r'], c['vtab'][:7], c['vtab'][1:8], 0.98, 0.95)
    eq_bits(adv2, gae_model(c['r'], c['vtab'][:7], c['vtab'][1:8], 0.98, 0.95)[0], 'gae face without the optional tables')
    assert ppo.gae(c['r'][:0], c['vtab'][:0], c['succ'][:0], 0.98, 0.95)[0].shape == (0, 65)
    y, stats = ppo.normalize_advantages(adv, 1e-8, 1)
    mean, inv, inv64 = stats_model(adv.ravel(), 1e-8, 1)
    assert stats[0] == mean and abs(float(stats[1]) - inv64) <= ADV_INV_TOL * inv64
    eq_bits(y, apply_model(adv, stats[0], stats[1]), 'normalize face')
    assert abs(float(y.mean())) < 1e-5 and abs(float(y.std(ddof=1)) - 1) < 1e-5
    # the gradient and the statistics
    k = 0
    Dx, A, hidden, bias, B, R = CASES[k]
    c = ppo_case(k)
    with pytest.raises(ValueError):
        ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'])    # nothing loaded
    pi.load(c['Ws'], c['bs'])
    assert ppo.policy_grad_work_floats(pi, B) == pi.grad_work_floats(B) and ppo.policy_grad_work_floats(pi, B, 32) == pi.grad_work_floats(B, 32)
    res = ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'], CLIP_EPS, ENT_COEF, ls_lo=c['lo'], ls_hi=c['hi'])
    h = env.handle
    ref = run_case(h, c)
    for key, name in (('ratio', 'ratio'), ('logratio', 'logratio'), ('clipped', 'clipped'), ('ghead', 'ghead')):
        eq_bits(res[key].astype(F32), ref[name].astype(F32), ('face', key))
    GC.check(res, ref, 'face', ('dW', 'db'))
    GC.check(ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'], (CLIP_LO, CLIP_HI), ENT_COEF, ls_lo=c['lo'], ls_hi=c['hi'], chunk_rows=32),
             run_case(h, c, 32), 'face, chunked', ('dW', 'db'))
    only = ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'], CLIP_EPS, ENT_COEF, grads=False, ls_lo=c['lo'], ls_hi=c['hi'])
    assert only['dW'] is None
    eq_bits(only['ghead'], ref['ghead'], 'face without grads')
    assert ppo.policy_grad(pi, c['x'][:0], c['zo'][:0], c['n'][:0], c['adv'][:0])['ghead'].shape == (0, 2 * A)
    st = ppo.stats(res['ratio'], res['logratio'], res['clipped'], c['adv'], CLIP_EPS)
    want = ppo_stats_model(res['ratio'], res['logratio'], res['clipped'], c['adv'])
    eq_bits(np.array([st['approx_kl'], st['clip_fraction'], st['surrogate'], st['mean_logratio']], F32), want, 'stats face')
    # policy_grad_device + adam_step_device move the weights as the call-by-call sequence does
    sa = pi.adam_state()
    work = ppo.policy_grad_work_floats(pi, B)
    with Dev(h) as dev:
        d = [dev.put(np.ascontiguousarray(c[key])) for key in ('x', 'zo', 'n', 'adv')]
        ppo.policy_grad_device(pi, B, d[0], d[1], d[2], d[3], dev.alloc(4 * work), work, CLIP_EPS, ENT_COEF, grads=sa.g, ls_lo=c['lo'], ls_hi=c['hi'])
        pi.adam_step_device(sa.g, sa, 1e-3)
        h.sync()
        fused = pi.parameters()
    pi.load(c['Ws'], c['bs'])
    sa = pi.adam_state()
    with Dev(h) as dev:
        d_x, d_g = dev.put(c['x']), dev.put(ref['ghead'])
        pi.grad_device(B, d_x, Dx, dev.alloc(4 * work), work, d_gout=d_g, grads=sa.g)
        pi.adam_step_device(sa.g, sa, 1e-3)
        h.sync()
        stepwise = pi.parameters()
    for u, v in zip(fused[0] + fused[1], stepwise[0] + stepwise[1]):
        eq_val(u, v, 'the weights after Adam')
    assert any(not np.array_equal(u, v) for u, v in zip(fused[0], c['Ws']))
    # refused arguments
    for call in (lambda: ppo.policy_grad(pi, c['x'][:, :-1], c['zo'], c['n'], c['adv']), lambda: ppo.policy_grad(pi, c['x'], c['zo'][:, :-1], c['n'], c['adv']),
                 lambda: ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'][:-1]), lambda: ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'], clip=1.5),
                 lambda: ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'], ls_lo=1.0, ls_hi=0.0),
                 lambda: ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'], chunk_rows=3), lambda: ppo.policy_grad(env.actor, c['x'], c['zo'], c['n'], c['adv']),
                 lambda: ppo.policy_grad(pi, c['x'], c['zo'], c['n'], c['adv'], pscale=INF), lambda: ppo.gae(c['x'], c['x'], c['x'], 1.5, 0.9),
                 lambda: ppo.gae(c['x'], c['x'][:-1], c['x'], 0.9, 0.9), lambda: ppo.normalize_advantages(c['adv'][:1], ddof=1),
                 lambda: ppo.normalize_advantages(c['adv'], eps=-1.0), lambda: ppo.stats(res['ratio'], res['logratio'][:-1], res['clipped'], c['adv'])):
        with pytest.raises(ValueError):
            call()
    pi.close()
    env.close()


# 9. invalid calls
def case_invalid_calls(library):
    """one invalid call per item of the validation lists of include/pmg.h, nothing written"""
    nan = float('nan')
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B, T, N = 6, 3, 8, 4, 6
        with Dev(h) as dev:
            actor = Net(h, dev, *network(81, (Dx, 16, 2 * A)))
            odd, nobias = Net(h, dev, *network(88, (Dx, 16, 2 * A + 1))), Net(h, dev, network(85, (Dx, 16, 2 * A))[0], None)
            d_in = dev.put(np.zeros(64 * 16, F32))
            size = 4 * B * 2 * A + 4 * T * N * 2
            outs = [dev.put(np.full(size, SENTINEL, np.uint8)) for _ in range(4)]
            need = h.ppo_policy_grad_work_floats(actor.mlp, B, 2)
            wsize = 4 * (need + 8)
            d_work = dev.put(np.full(wsize, SENTINEL, np.uint8))
            par = Params(h, dev, *network(81, (Dx, 16, 2 * A)))
            par_nb = Params(h, dev, network(85, (Dx, 16, 2 * A))[0], None)

            def mlp(net, **kw):
                m = h.mlp_struct(net.widths, net.d_w, net.d_b, 0)
                for k, v in kw.items():
                    if k in ('width', 'd_weight', 'd_bias'):
                        getattr(m, k)[v[0]] = v[1]
                    else:
                        setattr(m, k, v)
                return m

            def pg(am=None, null_g=False, chunk=0, grads='par', **kw):
                a = dict(batch=B, d_x=d_in, x_stride=Dx, d_preact_old=d_in, preact_old_stride=2 * A, d_noise=d_in, noise_stride=A, d_adv=d_in, pscale=-1.0 / B,
                         escale=-0.01 / B, clip_lo=CLIP_LO, clip_hi=CLIP_HI, ls_lo=-2.0, ls_hi=0.5, grads=par.struct if grads == 'par' else grads, d_ratio=outs[0],
                         d_logratio=outs[1], d_clipped=outs[2], d_ghead=outs[3], ghead_stride=2 * A, d_work=d_work, work_floats=need + 8)
                size_ = kw.pop('struct_size', None)
                a.update(kw)
                s = h.ppo_policy_grad_struct(**a)
                if size_ is not None:
                    s.struct_size = size_
                return h.L.lib.pmg_ppo_policy_grad_device(h.h, C.byref(am or mlp(actor)), None if null_g else C.byref(s), C.c_int64(chunk))

            tab = lambda p, ts=N, es=1: (p, ts, es)

            def gae(null_g=False, **kw):
                a = dict(steps=T, envs=N, gamma=0.98, lam=0.95, reward=tab(d_in), value=tab(d_in), value_next=tab(d_in + 4 * N), adv=tab(outs[0]), cut=tab(d_in),
                         terminal=tab(d_in), ret=tab(outs[1]))
                size_ = kw.pop('struct_size', None)
                a.update(kw)
                s = h.gae_struct(**a)
                if size_ is not None:
                    s.struct_size = size_
                return h.L.lib.pmg_gae_device(h.h, None if null_g else C.byref(s))

            def ast(null_s=False, **kw):
                a = dict(count=B, d_x=d_in, d_stats=outs[0], eps=1e-8, ddof=0)
                size_ = kw.pop('struct_size', None)
                a.update(kw)
                s = h.adv_stats_struct(**a)
                if size_ is not None:
                    s.struct_size = size_
                return h.L.lib.pmg_adv_stats_device(h.h, None if null_s else C.byref(s))

            def app(d_x=d_in, count=B, d_stats=d_in, d_y=outs[0]):
                return h.L.lib.pmg_adv_apply_device(h.h, C.c_void_p(d_x), C.c_int64(count), C.c_void_p(d_stats), C.c_void_p(d_y))

            def pst(null_s=False, **kw):
                a = dict(batch=B, d_ratio=d_in, d_logratio=d_in, d_clipped=d_in, d_adv=d_in, d_stats=outs[0], clip_lo=CLIP_LO, clip_hi=CLIP_HI)
                size_ = kw.pop('struct_size', None)
                a.update(kw)
                s = h.ppo_stats_struct(**a)
                if size_ is not None:
                    s.struct_size = size_
                return h.L.lib.pmg_ppo_stats_device(h.h, None if null_s else C.byref(s))
            none = dict(d_ratio=None, d_logratio=None, d_clipped=None, d_ghead=None)
            missing_b = h.params_struct(list(par.struct.d_weight)[:2], [par.struct.d_bias[0], None])
            missing_w = h.params_struct([par.struct.d_weight[0], None], list(par.struct.d_bias)[:2])
            off_w = h.params_struct([par.struct.d_weight[0] + 2, par.struct.d_weight[1]], list(par.struct.d_bias)[:2])
            bad_nets = [mlp(actor, **kw) for kw in (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                                     dict(width=(1, 0)), dict(d_weight=(0, None)), dict(out_activation=2), dict(d_weight=(1, actor.d_w[1] + 2)),
                                                     dict(out_activation=1))] + [mlp(odd)]
            bad = [lambda m=m: pg(am=m) for m in bad_nets] + [
                # the gradient call
                lambda: pg(ls_lo=1.0, ls_hi=0.0), lambda: pg(ls_lo=nan), lambda: pg(ls_hi=INF), lambda: pg(pscale=INF), lambda: pg(pscale=nan), lambda: pg(escale=-INF),
                lambda: pg(escale=nan), lambda: pg(clip_lo=nan), lambda: pg(clip_hi=nan), lambda: pg(clip_lo=-0.1), lambda: pg(clip_lo=1.3, clip_hi=1.2),
                lambda: pg(batch=-1), lambda: pg(d_x=None), lambda: pg(d_preact_old=None), lambda: pg(d_noise=None), lambda: pg(d_adv=None),
                lambda: pg(grads=None, **none), lambda: pg(grads=missing_b), lambda: pg(grads=missing_w), lambda: pg(grads=off_w),
                lambda: pg(am=mlp(nobias), grads=par.struct), lambda: pg(x_stride=Dx - 1), lambda: pg(preact_old_stride=2 * A - 1), lambda: pg(noise_stride=A - 1),
                lambda: pg(ghead_stride=2 * A - 1), lambda: pg(d_x=d_in + 2), lambda: pg(d_preact_old=d_in + 1), lambda: pg(d_noise=d_in + 3), lambda: pg(d_adv=d_in + 2),
                lambda: pg(d_ratio=outs[0] + 1), lambda: pg(d_logratio=outs[1] + 2), lambda: pg(d_ghead=outs[3] + 3), lambda: pg(d_work=d_work + 1),
                lambda: pg(chunk=-2), lambda: pg(chunk=1), lambda: pg(chunk=3), lambda: pg(batch=2 * 65535 + 1, chunk=2), lambda: pg(d_work=None),
                lambda: pg(work_floats=h.ppo_policy_grad_work_floats(actor.mlp, B, 0) - 1), lambda: pg(chunk=2, work_floats=need - 1), lambda: pg(null_g=True),
                lambda: pg(struct_size=C.sizeof(PmgPpoPolicyGrad) - 8),
                # GAE
                lambda: gae(null_g=True), lambda: gae(struct_size=C.sizeof(PmgGae) - 8), lambda: gae(gamma=1.5), lambda: gae(gamma=-0.1), lambda: gae(gamma=nan),
                lambda: gae(lam=1.01), lambda: gae(lam=-1.0), lambda: gae(lam=nan), lambda: gae(steps=-1), lambda: gae(envs=-1), lambda: gae(steps=2 ** 16, envs=2 ** 15),
                lambda: gae(steps=2 ** 31, envs=1), lambda: gae(reward=None), lambda: gae(value=None), lambda: gae(value_next=None), lambda: gae(adv=None),
                lambda: gae(reward=tab(d_in + 2)), lambda: gae(cut=tab(d_in + 1)), lambda: gae(terminal=tab(d_in + 3)), lambda: gae(adv=tab(outs[0] + 2)),
                lambda: gae(ret=tab(outs[1] + 1)),
                # strides that put two (t, i) of an output on one element
                lambda: gae(adv=tab(outs[0], N - 1, 1)), lambda: gae(adv=tab(outs[0], 1, T - 1)), lambda: gae(adv=tab(outs[0], 0, 1)), lambda: gae(adv=tab(outs[0], N, 0)),
                lambda: gae(ret=tab(outs[1], N - 1, 1)), lambda: gae(ret=tab(outs[1], 2, 3)), lambda: gae(adv=tab(outs[0], -(N - 1), 1)),
                # the normaliser
                lambda: ast(null_s=True), lambda: ast(struct_size=C.sizeof(PmgAdvStats) - 8), lambda: ast(count=-1), lambda: ast(ddof=2), lambda: ast(ddof=-1),
                lambda: ast(count=1, ddof=1), lambda: ast(eps=-1e-8), lambda: ast(eps=nan), lambda: ast(eps=INF), lambda: ast(d_x=None), lambda: ast(d_stats=None),
                lambda: ast(d_x=d_in + 2), lambda: ast(d_stats=outs[0] + 1), lambda: app(count=-1), lambda: app(d_x=None), lambda: app(d_stats=None),
                lambda: app(d_y=None), lambda: app(d_x=d_in + 1), lambda: app(d_stats=d_in + 2), lambda: app(d_y=outs[0] + 3),
                # the statistics
                lambda: pst(null_s=True), lambda: pst(struct_size=C.sizeof(PmgPpoStats) - 8), lambda: pst(batch=0), lambda: pst(batch=-1), lambda: pst(clip_lo=nan),
                lambda: pst(clip_lo=1.3, clip_hi=1.2), lambda: pst(clip_lo=-1.0), lambda: pst(d_ratio=None), lambda: pst(d_logratio=None), lambda: pst(d_clipped=None),
                lambda: pst(d_adv=None), lambda: pst(d_stats=None), lambda: pst(d_ratio=d_in + 2), lambda: pst(d_logratio=d_in + 1), lambda: pst(d_adv=d_in + 3),
                lambda: pst(d_stats=outs[0] + 2)]
            g0 = h.ppo_policy_grad_struct(B, d_in, Dx, d_in, 2 * A, d_in, A, d_in, -1.0 / B, 0.0, CLIP_LO, CLIP_HI, d_ratio=outs[0])
            assert h.L.lib.pmg_ppo_policy_grad_device(h.h, None, C.byref(g0), C.c_int64(0)) == E_INVALID

            def untouched():
                h.sync()
                for o in outs:
                    assert (dev.get(o, size, np.uint8) == SENTINEL).all()
                assert (dev.get(d_work, wsize, np.uint8) == SENTINEL).all()
                par.read(written=False)
            for k, call in enumerate(bad):
                assert call() == E_INVALID, k
                assert h.L.error(h.h), k
            untouched()
            assert pg(batch=0) == 0 and pg(batch=0, chunk=2) == 0 and pg(batch=0, grads=None) == 0 and gae(steps=0) == 0 and gae(envs=0) == 0
            assert gae(steps=0, adv=tab(outs[0], 0, 0)) == 0 and ast(count=0) == 0 and app(count=0) == 0
            untouched()
            # the workspace figure
            base = h.mlp_grad_work_floats(actor.mlp, B)
            assert h.ppo_policy_grad_work_floats(actor.mlp, B, 0) == base and h.ppo_policy_grad_work_floats(actor.mlp, B, 2) == h.mlp_grad_chunked_work_floats(actor.mlp, B, 2)
            assert h.ppo_policy_grad_work_floats(actor.mlp, -1, 0) < 0 and h.ppo_policy_grad_work_floats(mlp(odd), B, 0) < 0
            assert h.ppo_policy_grad_work_floats(actor.mlp, B, 3) < 0 and h.ppo_policy_grad_work_floats(mlp(actor, num_layers=0), B, 0) < 0
            # what is allowed
            assert pg() == 0 and pg(chunk=2) == 0 and pg(clip_lo=0.0, clip_hi=INF) == 0 and pg(clip_lo=1.0, clip_hi=1.0) == 0
            assert pg(grads=None, d_work=None, work_floats=0) == 0 and pg(grads=None, **dict(none, d_clipped=outs[2])) == 0 and pg(am=mlp(nobias), grads=par_nb.struct) == 0
            assert pg(pscale=0.0, escale=0.0) == 0 and pg(d_clipped=outs[2] + 1) == 0
            assert gae() == 0 and gae(cut=None, terminal=None, ret=None) == 0 and gae(gamma=0.0, lam=1.0) == 0 and gae(adv=tab(outs[0], 1, T), ret=tab(outs[1], N + 5, 1)) == 0
            assert gae(reward=tab(d_in, 0, 0)) == 0 and gae(adv=tab(outs[0] + 4 * (T - 1) * N, -N, 1)) == 0 and gae(steps=1, adv=tab(outs[0], 0, 1)) == 0
            assert gae(envs=1, adv=tab(outs[0], 1, 0)) == 0
            assert ast() == 0 and ast(ddof=1) == 0 and ast(eps=0.0) == 0 and app() == 0 and app(d_x=outs[0]) == 0 and pst() == 0 and pst(batch=1) == 0
            h.sync()


# 10. what tests/test_ppo_wave_order.py runs under every wavefront order
def wave_order_run(library):
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for name, k in (('wide', 3), ('far', 6), ('small', 0)):
            c = ppo_case(k)
            B = min(c['x'].shape[0], 33)
            cc = dict(c, x=c['x'][:B], zo=c['zo'][:B], n=c['n'][:B], adv=c['adv'][:B])
            for tag, kw in (('', dict()), ('g', dict(grads=False)), ('c', dict(R=2))):
                got = run_case(h, cc, pad=1, shift=1, **kw)
                for key in OUTPUTS:
                    res[name + tag + key] = got[key].astype(F32)
                if got['dW'] is not None:
                    for l, (w, b) in enumerate(zip(got['dW'], got['db'])):
                        res['%s%sdW%d' % (name, tag, l)] = w
                        if b is not None:
                            res['%s%sdb%d' % (name, tag, l)] = b
    return res
