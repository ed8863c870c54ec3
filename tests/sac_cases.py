"""The cases of the SAC tests (include/pmg.h pmg_sac_sample_device, pmg_sac_act_env_device, pmg_sac_target_device) and their
numpy model, shared by four files: tests/test_sac_emulated.py runs them on the g++ build of the product sources over the fiber emulator,
tests/test_gpu_sac.py on libpmg_hip.so on the MI355X, tests/test_sac_host.py covers the model alone and the numpy face,
tests/test_sac_wave_order.py the kernels under permuted wavefront order.  The pieces are those of tests/actor_cases.py, tests/td_cases.py and
tests/td3_cases.py: the exact float32 fmaf chain, the integer draws, the critic's model, the epilogue, the canaries, the stale regimes.

Bars.  z is bit-defined (compared by value with the chain model).  n, a and logp go through the build's logf / sqrtf / cosf / expf / tanhf /
log1pf: they are held to the float64 model -- n from the integer draws, a and logp from the device's own n and the bit-checked z.  The three
bars were MEASURED on this model alone (measure_bars below, run by tests/test_sac_host.py): the largest error of the numpy float32
restatement of the head (same expression order, same n) against the float64 model over every input of SAMPLE_CASES; each bar is 4 x that
error, the headroom the project gives library functions that differ by an ulp or two between numpy and a build (actor_cases.ACTION_TOL,
grad_cases.MODEL_TOL).  None of them comes from a device's output.
  SAC_N_TOL     |n - n64|, absolute.
  SAC_A_TOL     |a - a64|, absolute (no scaling by |u| was needed: tanh's slope falls faster than u's rounding error grows).
  SAC_LOGP_TOL  |logp - logp64| relative to the sum over j of the magnitudes of the summands of l_j (n^2 / 2, |ls|, log(2 pi) / 2,
                2 (log 2 + |u| + softplus(-2 u))): the condition of the sum.
q1, q2, q_min and y of the target are bit-equal to pmg_q_device and the numpy epilogue on the call's OWN a' and logp (DESIGN.md 3.10's rule)."""
import ctypes as C

import numpy as np

import actor_cases as AC
import td3_cases as T3
import td_cases as TC
from actor_cases import Net, bits, check_z, explore_draws, fmaf, forward, network
from normalizer_cases import POL, SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PmgMlp, PmgSacSample, PmgSacTarget
from td_cases import BATCHES, INF, Out, eq_bits, eq_y, put_rows, q_model

E_INVALID, E_STATE = -1, -4
F32, F64 = np.float32, np.float64
TILE = AC.TILE
LS_LO, LS_HI = -20.0, 2.0
PAIRS = ((6, 3), (1, 1), (2, 5), (3, 12), (29, 4), (1, 20), (5, 9))          # the last two: Dx < A, the hand-over hazard of DESIGN.md 3.15
HIDDEN = ((), (33,), (256, 256, 256))
LOG2_32, HALF_LOG_2PI_32, TWO_PI_32 = F32(0.69314718055994530942), F32(0.91893853320467274178), F32(6.28318530717958647692)
LOG2, HALF_LOG_2PI = 0.69314718055994530942, 0.91893853320467274178
# measured by measure_bars() (numpy float32 restatement against the float64 model, every input of SAMPLE_CASES; x86-64 glibc / numpy):
SAC_N_MEASURED = 1.36e-6          # 1.355e-6; bar 5.44e-6; observed maxima: emulator 1.36e-6, MI355X 1.36e-6
SAC_A_MEASURED = 1.49e-7          # 1.488e-7; bar 5.96e-7; observed: emulator 1.04e-7, MI355X 1.06e-7
SAC_LOGP_MEASURED = 9.6e-8        # 9.55e-8 = 1.6 units of 2^-24, relative to the magnitude sum; bar 3.84e-7; observed: emulator 8.0e-8, MI355X 7.9e-8
SAC_N_TOL, SAC_A_TOL, SAC_LOGP_TOL = 4 * SAC_N_MEASURED, 4 * SAC_A_MEASURED, 4 * SAC_LOGP_MEASURED
OUTPUTS = ('y', 'qmin', 'q1', 'q2', 'a', 'logp')


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def draws(seed, counter, row_offset, B, A):
    """u1, u2 [B, A] float64 (exact float32 values): sample index (row_offset + b) * A + j"""
    u1, u2, _, _ = explore_draws(seed, counter, np.arange(B, dtype=np.uint64) + np.uint64(row_offset), A, 0.0)
    return u1, u2


def n64_of(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def n32_of(u1, u2):
    u1, u2 = u1.astype(F32), u2.astype(F32)
    return np.sqrt(F32(-2) * np.log(u1)) * np.cos(TWO_PI_32 * u2)


def head64(z, n, lo=LS_LO, hi=LS_HI):
    """the float64 model of the head from pre-activations z [B, 2 A] and the noise n [B, A] -> a, logp, mag (the sum of the summands'
    magnitudes), u, ls"""
    z, n = np.asarray(z, F32).astype(F64), np.asarray(n).astype(F64)
    A = z.shape[1] // 2
    m, ls = z[:, :A], np.clip(z[:, A:], float(F32(lo)), float(F32(hi)))
    u = np.exp(ls) * n + m
    w = -2.0 * u
    sp = np.maximum(w, 0.0) + np.log1p(np.exp(-np.abs(w)))
    l = (-0.5 * n * n - ls - HALF_LOG_2PI) - 2.0 * ((LOG2 - u) - sp)
    mag = 0.5 * n * n + np.abs(ls) + HALF_LOG_2PI + 2.0 * (LOG2 + np.abs(u) + sp)
    return np.tanh(u), l.sum(1), mag.sum(1), u, ls


def head32(z, n, lo=LS_LO, hi=LS_HI):
    """the float32 restatement, the normative expression order, numpy's float32 functions standing in for the build's -> a, logp"""
    z, n = np.asarray(z, F32), np.asarray(n, F32)
    A = z.shape[1] // 2
    m, ls = z[:, :A], np.minimum(np.maximum(z[:, A:], F32(lo)), F32(hi))
    u = fmaf(np.exp(ls), n, m).reshape(m.shape)
    w = F32(-2) * u
    sp = np.maximum(w, F32(0)) + np.log1p(np.exp(-np.abs(w)))
    c2 = (LOG2_32 - u) - sp
    l = fmaf(np.full(m.shape, -2, F32), c2, fmaf(F32(-0.5) * n, n, -ls).reshape(m.shape) - HALF_LOG_2PI_32).reshape(m.shape)
    acc = np.zeros(m.shape[0], F32)
    for j in range(A):
        acc = acc + l[:, j]
    return np.tanh(u), acc


def soft_epilogue(qmin, logp, r, gamma, alpha, lo=-INF, hi=INF, term=None):
    """t = terminal ? r : fmaf(gamma, fmaf(-alpha, logp, qmin), r); y = clip(t) -> t, y"""
    with np.errstate(invalid='ignore', over='ignore'):
        soft = fmaf(np.full(qmin.shape, -F32(alpha), F32), logp, qmin).reshape(qmin.shape)
    return TC.epilogue(soft, r, gamma, lo, hi, term)


def sample_case(Dx, A, hidden, B=BATCHES[-1]):
    """a Gaussian actor Dx -> hidden -> 2 A, rows and the chain model's z: means up to about 4 in magnitude, raw log-stds spread over about
    [-23, 17] -- below LS_LO, inside the range and above LS_HI all occur over the cases (asserted by their users)"""
    def make():
        Ws, bs = network(1500 + 13 * Dx + A + len(hidden), (Dx,) + tuple(hidden) + (2 * A,))
        rs = np.random.RandomState(Dx * 23 + A + 7 * len(hidden))
        x = rs.uniform(-2, 2, (B, Dx)).astype(F32)
        z = forward(x, Ws, bs)
        sm = F32(2.0 ** np.floor(np.log2(4.0 / max(np.abs(z[:, :A]).max(), 1e-30))))
        Ws[-1][:A], bs[-1][:A] = Ws[-1][:A] * sm, bs[-1][:A] * sm
        zl = z[:, A:]
        sl = F32(2.0 ** np.floor(np.log2(20.0 / max(np.abs(zl - zl.mean()).max(), 1e-30))))
        Ws[-1][A:] = Ws[-1][A:] * sl
        bs[-1][A:] = (bs[-1][A:] * sl - F32(zl.mean()) * sl - F32(3)).astype(F32)
        return {'Ws': Ws, 'bs': bs, 'x': x, 'z': forward(x, Ws, bs)}
    return TC.cached(('sac actor', Dx, A, tuple(hidden), B), make)


SAMPLE_CASES = tuple((Dx, A, hidden) for Dx, A in PAIRS for hidden in HIDDEN)
SEEDS = lambda k: (17 + k, 2 ** 40 + 3 * k, (0, 5, 2 ** 33, 1)[k % 4])          # seed, counter, row_offset of case k


def measure_bars(cases=SAMPLE_CASES):
    """-> the largest |n32 - n64|, |a32 - a64| and |logp32 - logp64| / mag of the numpy float32 restatement against the float64 model, both
    given the same (float32) n, over every input of the cases"""
    worst = [0.0, 0.0, 0.0]
    for k, (Dx, A, hidden) in enumerate(cases):
        m = sample_case(Dx, A, hidden)
        u1, u2 = draws(*SEEDS(k), m['x'].shape[0], A)
        n32 = n32_of(u1, u2)
        a32, lp32 = head32(m['z'], n32)
        a64, lp64, mag, _, _ = head64(m['z'], n32)
        for i, e in enumerate((np.abs(n32 - n64_of(u1, u2)).max(), np.abs(a32 - a64).max(), (np.abs(lp32 - lp64) / mag).max())):
            worst[i] = max(worst[i], float(e))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# device calls
def device_sample(h, Ws, bs, x, lo=LS_LO, hi=LS_HI, sample=1, seed=0, counter=0, row_offset=0, x_pad=0, shift=0, pads=(0, 0, 0), null=()):
    """pmg_sac_sample_device on canary-framed buffers -> dict(a, logp, n, z) (None for an output passed as NULL); pads: floats between the rows
    of a, n and z (sentinel bytes that must survive); shift: floats off the 16-byte boundary"""
    B, A = x.shape[0], Ws[-1].shape[0] // 2
    widths = {'a': A, 'logp': 1, 'n': A, 'z': 2 * A}
    strides = {'a': A + pads[0], 'logp': 1, 'n': A + pads[1], 'z': 2 * A + pads[2]}
    with Dev(h) as dev:
        net = Net(h, dev, Ws, bs, 0)
        d_x, xs = put_rows(h, dev, x, x_pad, shift)
        outs = {k: Out(dev, 4 * B * strides[k], 4 * ((shift + i) & 3)) for i, k in enumerate(('a', 'logp', 'n', 'z'))}
        ptr = lambda k: None if k in null else outs[k].ptr
        s = h.sac_sample_struct(B, d_x, xs, ptr('a'), strides['a'], ptr('logp'), ptr('n'), strides['n'], ptr('z'), strides['z'], lo, hi, sample, seed, counter,
                                row_offset)
        h.sac_sample_device(net.mlp, s)
        res = {}
        for k, o in outs.items():
            raw = o.read(np.uint8, written=k not in null)
            if raw is None:
                res[k] = None
                continue
            rows = raw.reshape(B, 4 * strides[k])
            assert (rows[:, 4 * widths[k]:] == SENTINEL).all(), 'the padding between output rows was written'
            res[k] = np.ascontiguousarray(rows[:, :4 * widths[k]]).view(F32)
    res['logp'] = None if res['logp'] is None else res['logp'][:, 0]
    return res


def device_sac_target(h, Wa, ba, W1, b1, W2=None, b2=None, x=None, r=None, gamma=0.98, lo=-INF, hi=INF, term=None, alpha=0.2, ls_lo=LS_LO, ls_hi=LS_HI,
                      sample=1, seed=0, counter=0, row_offset=0, d_alpha=None, c1_out=0, c2_out=0, x_pad=0, shift=0, null=()):
    """pmg_sac_target_device on canary-framed buffers -> dict(y, qmin, q1, q2, a, logp) (None for an output passed as NULL).  The workspace is
    canary-framed and sized exactly pmg_sac_target_work_floats (NULL where that is 0).  d_alpha: a value put into device memory and passed as
    d_alpha (the struct's alpha is then 0)."""
    B, A = x.shape[0], Wa[-1].shape[0] // 2
    with Dev(h) as dev:
        actor, c1 = Net(h, dev, Wa, ba, 0), Net(h, dev, W1, b1, c1_out)
        c2 = Net(h, dev, W2, b2, c2_out) if W2 is not None else None
        d_x, xs = put_rows(h, dev, x, x_pad, shift)
        d_r, _ = put_rows(h, dev, np.asarray(r, F32)[None, :], 0, (shift + 1) & 3)
        d_t = None
        if term is not None:
            d_t = dev.alloc(B + 32)
            d_t += (-d_t) % 16 + 1
            h.upload(d_t, np.ascontiguousarray(term, np.uint8))
        d_al = None
        if d_alpha is not None:
            d_al, _ = put_rows(h, dev, np.array([[d_alpha]], F32), 0, (shift + 2) & 3)
        outs = {k: Out(dev, 4 * B * (A if k == 'a' else 1), 4 * ((shift + n) & 3)) for n, k in enumerate(OUTPUTS)}
        ptr = lambda k: None if k in null else outs[k].ptr
        need = h.sac_target_work_floats(actor.mlp, 'a' not in null, B)
        assert need == (B * A if 'a' in null else 0)
        work = Out(dev, 4 * need, 4 * ((shift + 1) & 3)) if need else None
        td = h.sac_target_struct(B, d_x, xs, d_r, outs['y'].ptr, gamma, lo, hi, 0.0 if d_alpha is not None else alpha, ls_lo, ls_hi, sample, seed, counter,
                                 row_offset, d_al, d_t, ptr('qmin'), ptr('q1'), ptr('q2'), ptr('a'), ptr('logp'), work.ptr if work else None, need)
        h.sac_target_device(actor.mlp, c1.mlp, c2.mlp if c2 is not None else None, td)
        res = {k: o.read(written=k not in null and not (k == 'q2' and c2 is None)) for k, o in outs.items()}
        if work:
            work.read()
    if res['a'] is not None:
        res['a'] = res['a'].reshape(B, A)
    return res


def check_head(got, z, u1, u2, lo, hi, label, sample=1):
    """n against the draws, a and logp against the float64 model from the device's own n -> the three errors"""
    if sample:
        en = float(np.abs(got['n'] - n64_of(u1, u2)).max())
        assert en <= SAC_N_TOL, (label, 'n', en)
    else:
        en = 0.0
        assert (bits(got['n']) == 0).all(), (label, 'n is +0.0 without sampling')
    a64, lp64, mag, _, _ = head64(z, got['n'], lo, hi)
    ea, el = float(np.abs(got['a'] - a64).max()), float((np.abs(got['logp'] - lp64) / mag).max())
    assert ea <= SAC_A_TOL, (label, 'a', ea)
    assert np.isfinite(got['logp']).all() and el <= SAC_LOGP_TOL, (label, 'logp', el)
    return en, ea, el


# ----------------------------------------------------------------------------------------------------------------------
# 2. sample
def case_sample(library, cases=SAMPLE_CASES):
    worst = np.zeros(3)
    seen = set()
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for Dx, A, hidden in cases:
            k = SAMPLE_CASES.index((Dx, A, hidden))
            m = sample_case(Dx, A, hidden)
            seed, counter, off = SEEDS(k)
            for B in (BATCHES if (Dx, A) == (6, 3) else (BATCHES[k % len(BATCHES)], BATCHES[-1])):
                x, z = m['x'][:B], m['z'][:B]
                got = device_sample(h, m['Ws'], m['bs'], x, seed=seed, counter=counter, row_offset=off, x_pad=(k + B) % 3, shift=(k + B) % 4,
                                    pads=((k + B) % 2, (k + 1) % 3, k % 2))
                check_z(got['z'], z, (Dx, A, hidden, B, 'z'))
                u1, u2 = draws(seed, counter, off, B, A)
                worst = np.maximum(worst, check_head(got, z, u1, u2, LS_LO, LS_HI, (Dx, A, hidden, B)))
                raw = z[:, A:]
                seen |= {s for s, hit in (('below', raw < F32(LS_LO)), ('inside', (raw > F32(LS_LO)) & (raw < F32(LS_HI))), ('above', raw > F32(LS_HI)),
                                          ('saturated', np.abs(got['a']) == 1)) if hit.any()}
                if (np.abs(got['a']) == 1).any():
                    assert np.isfinite(got['logp'][(np.abs(got['a']) == 1).any(1)]).all()
    print('sample: largest |n - n64| = %.3g (bar %.3g), |a - a64| = %.3g (bar %.3g), |logp - logp64| / magnitude = %.3g (bar %.3g)' % (
        worst[0], SAC_N_TOL, worst[1], SAC_A_TOL, worst[2], SAC_LOGP_TOL))
    if len(cases) == len(SAMPLE_CASES):
        assert seen == {'below', 'inside', 'above', 'saturated'}, seen
    return worst


def case_sample_properties(library):
    """sample == 0, row_offset, counter, determinism, every output NULL in turn, another clamp"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for Dx, A, hidden in ((6, 3, (33,)), (1, 20, ())):
            m = sample_case(Dx, A, hidden)
            Ws, bs, x, z = m['Ws'], m['bs'], m['x'], m['z']
            mode = device_sample(h, Ws, bs, x, sample=0, seed=1, counter=2, row_offset=3)
            other = device_sample(h, Ws, bs, x, sample=0, seed=9, counter=8, row_offset=7, shift=1)
            check_head(mode, z, None, None, LS_LO, LS_HI, 'mode', sample=0)
            for k in ('a', 'logp', 'n', 'z'):
                eq_bits(other[k], mode[k], ('sample == 0 under another seed', k))
            whole = device_sample(h, Ws, bs, x, seed=7, counter=8)
            part = device_sample(h, Ws, bs, x[40:], seed=7, counter=8, row_offset=40, x_pad=1, shift=1)
            again = device_sample(h, Ws, bs, x, seed=7, counter=8, shift=2, pads=(1, 2, 3))
            for k in ('a', 'logp', 'n', 'z'):
                eq_bits(part[k], whole[k][40:], ('row_offset', k))
                eq_bits(again[k], whole[k], ('twice', k))
            moved = device_sample(h, Ws, bs, x, seed=7, counter=9)
            assert (moved['a'] != whole['a']).mean() > 0.5 and (moved['n'] != whole['n']).mean() > 0.9
            for null in (('a',), ('logp',), ('n',), ('z',), ('a', 'n', 'z'), ('logp', 'n', 'z')):
                got = device_sample(h, Ws, bs, x[:33], seed=7, counter=8, null=null, shift=3)
                for k in ('a', 'logp', 'n', 'z'):
                    if got[k] is not None:
                        eq_bits(got[k], whole[k][:33], (null, k))
            # a narrow clamp: every raw log-std is outside it on one side or the other
            got = device_sample(h, Ws, bs, x, -1.0, -0.5, seed=7, counter=8)
            u1, u2 = draws(7, 8, 0, x.shape[0], A)
            check_head(got, z, u1, u2, -1.0, -0.5, 'narrow clamp')
            eq_bits(got['n'], whole['n'], 'the clamp does not move the draws')


# 3. env acting
def case_env(library, task='push'):
    N = TILE + 5
    per_offset = {}
    for offset in (0, 32):
        env = AC.stepped(library, task, N, env_index_offset=offset)
        h, A = env.handle, env.dims.action_dim
        W0 = h.norm_width(POL) + h.dims.goal_dim
        Ws, bs = network(1600, (W0, 64, 33, 2 * A))
        bs[-1][A:] = bs[-1][A:] - F32(1)
        x = AC.policy_rows(h, POL)
        z_model = forward(x, Ws, bs)
        with Dev(h) as dev:
            net = Net(h, dev, Ws, bs, 0)
            outs = {k: Out(dev, 4 * N * w, 4 * i) for i, (k, w) in enumerate((('a', A), ('logp', 1), ('n', A), ('z', 2 * A)))}
            s = h.sac_sample_struct(0, None, 0, outs['a'].ptr, A, outs['logp'].ptr, outs['n'].ptr, A, outs['z'].ptr, 2 * A, LS_LO, LS_HI, 1, 21, 22, 12345)
            h.sac_act_env_device(net.mlp, POL, s)
            got = {k: o.read().reshape(N, -1) for k, o in outs.items()}
            got['logp'] = got['logp'][:, 0]
            only = Out(dev, 4 * N * A)
            h.sac_act_env_device(net.mlp, POL, h.sac_sample_struct(0, None, 0, only.ptr, A, None, None, 0, None, 0, LS_LO, LS_HI, 1, 21, 22, 0))
            eq_bits(only.read().reshape(N, A), got['a'], (task, offset, 'actions alone'))
        check_z(got['z'], z_model, (task, offset, 'z'))              # the rows layer 0 saw are those of pmg_policy_input_env_device
        want = device_sample(h, Ws, bs, x, seed=21, counter=22, row_offset=offset)
        for k in ('a', 'logp', 'n', 'z'):
            eq_bits(got[k], want[k], (task, offset, k))
        u1, u2 = draws(21, 22, offset, N, A)
        check_head(got, z_model, u1, u2, LS_LO, LS_HI, (task, offset))
        per_offset[offset] = got['n']
        env.close()
    eq_bits(per_offset[0][32:], per_offset[32][:N - 32], 'two handles agree on the global envs they share')


# 4. target
def target_nets(n, Dx, A, h1=(33,), h2=(64, 33)):
    return T3.critics(1700 + 10 * n, Dx, A, h1, h2)


def check_target(h, got, m, nets, x, r, gamma, lo, hi, term, alpha, seeds, label, sample=1, ls=(LS_LO, LS_HI), c1_out=0, c2_out=0):
    """a', logp: the bits of pmg_sac_sample_device; q1, q2: the bits of pmg_q_device on the call's own a'; qmin, y: the numpy epilogue"""
    seed, counter, off = seeds
    ref = device_sample(h, m['Ws'], m['bs'], x, ls[0], ls[1], sample, seed, counter, off, null=('n', 'z'))
    eq_bits(got['a'], ref['a'], (label, 'a'))
    eq_bits(got['logp'], ref['logp'], (label, 'logp'))
    q1, q2 = T3.device_qs(h, *nets, x, got['a'], c1_out, c2_out)
    eq_bits(got['q1'], q1, (label, 'q1'))
    if q2 is not None:
        eq_bits(got['q2'], q2, (label, 'q2'))
    qmin = np.minimum(q1, q2) if q2 is not None else q1
    eq_bits(got['qmin'] + F32(0), qmin + F32(0), (label, 'qmin'))
    eq_y(got['y'], soft_epilogue(qmin, got['logp'], r, gamma, alpha, lo, hi, term)[1], (label, 'y'))


def case_target(library, pairs=PAIRS):
    relations = set()
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for Dx, A in pairs:
            n = PAIRS.index((Dx, A))
            hidden, h1, h2 = (((33,), (33,), (64, 33)), ((256, 256, 256), (256,), (33, 255, 31)), ((), (256, 256, 256), ()))[n % 3]
            B = BATCHES[(n + 1) % len(BATCHES)] if n else BATCHES[-1]
            m = sample_case(Dx, A, hidden)
            x = m['x'][:B]
            rs = np.random.RandomState(40 + n)
            r = -rs.randint(0, 2, B).astype(F32)
            term = (rs.uniform(0, 1, B) < 0.3).astype(np.uint8) * rs.randint(1, 256, B).astype(np.uint8)
            nets = target_nets(n, Dx, A, h1, h2)
            gamma, lo, hi, alpha = 0.98, -50.0, 0.0, 0.2
            seeds = SEEDS(n)
            kw = dict(x=x, r=r, gamma=gamma, lo=lo, hi=hi, term=term, alpha=alpha, seed=seeds[0], counter=seeds[1], row_offset=seeds[2])
            nulls = [(), ('a',), ('qmin',), ('q1',), ('q2',), ('logp',), ('qmin', 'q1', 'q2', 'a', 'logp')] if n < 2 or Dx < A else [(), ('a',)]
            full = None
            for k, null in enumerate(nulls):
                got = device_sac_target(h, m['Ws'], m['bs'], *nets, x_pad=(n + k) % 3, shift=(n + k) % 4, null=null, **kw)
                if full is None:
                    full = got
                    check_target(h, got, m, nets, x, r, gamma, lo, hi, term, alpha, seeds, (Dx, A))
                    relations |= {s for s, hit in (('<', got['q1'] < got['q2']), ('>', got['q1'] > got['q2'])) if hit.any()}
                else:
                    for key in OUTPUTS:
                        if got[key] is not None:
                            eq_bits(got[key], full[key], (Dx, A, null, key))
            # d_alpha given equals the same value passed as alpha; one critic sees the same action
            got = device_sac_target(h, m['Ws'], m['bs'], *nets, d_alpha=alpha, shift=1, **kw)
            for key in OUTPUTS:
                eq_bits(got[key], full[key], (Dx, A, 'd_alpha', key))
            one = device_sac_target(h, m['Ws'], m['bs'], nets[0], nets[1], None, None, **kw)
            assert one['q2'] is None
            for key, src in (('a', 'a'), ('logp', 'logp'), ('q1', 'q1'), ('qmin', 'q1')):
                eq_bits(one[key], full[src], (Dx, A, 'one critic', key))
            eq_y(one['y'], soft_epilogue(full['q1'], full['logp'], r, gamma, alpha, lo, hi, term)[1], (Dx, A, 'one critic', 'y'))
    if len(pairs) == len(PAIRS):
        assert relations == {'<', '>'}, relations


def case_target_is_td3(library, pairs=PAIRS):
    """sample == 0, alpha == 0: y, q1, q2, a' of pmg_td3_target_device with sigma = 0 on the tanh actor whose last layer is the mean half"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for Dx, A in pairs:
            n = PAIRS.index((Dx, A))
            m = sample_case(Dx, A, HIDDEN[(n + 1) % 3])
            B = BATCHES[n % len(BATCHES)]
            x = m['x'][:B]
            r = -np.random.RandomState(60 + n).randint(0, 2, B).astype(F32)
            nets = target_nets(20 + n, Dx, A)
            got = device_sac_target(h, m['Ws'], m['bs'], *nets, x=x, r=r, gamma=0.98, lo=-50.0, hi=0.0, alpha=0.0, sample=0, x_pad=1, shift=n % 4)
            assert np.isfinite(got['logp']).all()
            Wm, bm = m['Ws'][:-1] + [m['Ws'][-1][:A]], m['bs'][:-1] + [m['bs'][-1][:A]]
            old = T3.device_td3(h, Wm, bm, *nets, x, r, 0.98, -50.0, 0.0, act_out=1)
            for key in ('q1', 'q2', 'a'):
                eq_bits(got[key] + F32(0), old[key] + F32(0), (Dx, A, 'td3', key))
            eq_y(got['y'], old['y'], (Dx, A, 'td3', 'y'))


def case_epilogue(library):
    """terminal rows, both clips, no clip, gamma = 0, alpha = 0 and a large alpha"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B = 6, 3, 101
        m = sample_case(Dx, A, (33,))
        rs = np.random.RandomState(63)
        r = -rs.randint(0, 2, B).astype(F32)
        term = (rs.uniform(0, 1, B) < 0.3).astype(np.uint8)
        nets = target_nets(40, Dx, A)
        for W, b in ((nets[0], nets[1]), (nets[2], nets[3])):
            W[-1], b[-1] = W[-1] * F32(8), b[-1] * F32(8)               # |q| of some tens: t on both sides of both clips of [-50, 0]
        seeds = (5, 6, 7)
        base = dict(x=m['x'], r=r, seed=5, counter=6, row_offset=7)
        sides = set()
        for n, (gamma, lo, hi, tm, alpha) in enumerate(((0.98, -INF, INF, None, 0.2), (0.98, -50.0, 0.0, None, 0.2), (0.98, -50.0, 0.0, term, 1.5),
                                                        (0.98, -0.5, -0.25, term, 0.0), (0.0, -INF, INF, None, 0.2))):
            got = device_sac_target(h, m['Ws'], m['bs'], *nets, gamma=gamma, lo=lo, hi=hi, term=tm, alpha=alpha, shift=n % 4, **base)
            check_target(h, got, m, nets, m['x'], r, gamma, lo, hi, tm, alpha, seeds, n)
            t = soft_epilogue(got['qmin'], got['logp'], r, gamma, alpha, term=tm)[0]
            if gamma == 0.0:
                assert np.array_equal(got['y'], r)
            if tm is not None:
                assert np.array_equal(t[tm != 0], r[tm != 0])
            if n == 1:
                sides |= {s for s, hit in (('lo', t < F32(lo)), ('hi', t > F32(hi)), ('in', (t > F32(lo)) & (t < F32(hi)))) if hit.any()}
        assert sides == {'lo', 'hi', 'in'}, sides


# 5. stale tile
def stale_actor(regime, B, between):
    """td_cases.stale_case / td3_cases.stale_critics with a Gaussian actor: the means are their actor's outputs, the log-stds further outputs of
    the same kind.  between = 'actor': the ACTOR's hidden layer leaves column 33 huge or inf in front of an ordinary critic 1 (td_cases' critic,
    a second one behind); 'critics': critic 1's hidden layer leaves it so in front of critic 2 (td3_cases' pair)."""
    def make():
        m = T3.stale_critics(regime, B)
        rs = np.random.RandomState(290 + B)
        last = m['Wa'][-1]
        extra = (rs.uniform(0.5, 1, last.shape) * 1e-38 if regime == 'huge' else rs.uniform(-1, 1, last.shape)).astype(F32)
        Ws = list(m['Wa'][:-1]) + [np.concatenate([last, extra], 0)]
        bs = list(m['ba'][:-1]) + [np.concatenate([m['ba'][-1], rs.uniform(-1.5, 0.5, last.shape[0]).astype(F32)])]
        with np.errstate(over='ignore', invalid='ignore'):
            z = forward(m['x'], Ws, bs)
        assert np.isfinite(z).all()
        if between == 'actor':
            c = TC.stale_case(regime, B)
            assert np.array_equal(c['x'], m['x'])
            W2, b2 = network(196, (33, 64, 1))
            W2[0] = (W2[0] * (1.0 if regime == 'huge' else 1e-9)).astype(F32)
            nets = (c['Wc'], c['bc'], W2, b2)
        else:
            nets = (m['W1'], m['b1'], m['W2'], m['b2'])
        return {'Ws': Ws, 'bs': bs, 'z': z, 'x': m['x'], 'r': m['r'], 'nets': nets}
    return TC.cached(('sac stale', regime, B, between), make)


def case_stale_tile(library):
    """td_cases' and td3_cases' `huge` and `inf` regimes in front of critic 1 and of critic 2, B = 33, Dx + A = 33 (odd): every output against
    the MODEL -- a' against float64 from the chain model's z, q1 / q2 against the numpy chain on the call's own a' (a finite wrong answer shows:
    a stale inf that meets the stand-in zero of the padding column becomes a NaN, and ReLU turns that into a finite 0)"""
    B = TILE + 1
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for regime in ('huge', 'inf'):
            for between in ('actor', 'critics'):
                m = stale_actor(regime, B, between)
                x, r, nets = m['x'], m['r'], m['nets']
                whole = None
                for null in ((), ('a',)):
                    got = device_sac_target(h, m['Ws'], m['bs'], *nets, x=x, r=r, gamma=0.98, alpha=0.2, seed=3, counter=4, row_offset=5, x_pad=1, null=null)
                    if whole is None:
                        whole = got
                        u1, u2 = draws(3, 4, 5, B, 4)
                        a64 = head64(m['z'], n32_of(u1, u2))[0]
                        assert np.abs(got['a'] - a64).max() <= SAC_A_TOL + SAC_N_TOL * np.exp(0.5), (regime, between)   # the model's n: its error rides on sd <= e^0.5
                        with np.errstate(over='ignore', invalid='ignore'):
                            q1, q2 = q_model(x, got['a'], nets[0], nets[1]), q_model(x, got['a'], nets[2], nets[3])
                        assert np.isfinite(q1).all() and np.isfinite(q2).all() and len(set(q2.tolist())) > B // 2
                        assert between == 'actor' or ((q1 < q2).any() and (q2 < q1).any())
                        eq_bits(got['q1'], q1, (regime, between, 'q1 against the model'))
                        eq_bits(got['q2'], q2, (regime, between, 'q2 against the model'))
                        eq_y(got['y'], soft_epilogue(np.minimum(q1, q2), got['logp'], r, 0.98, 0.2)[1], (regime, between, 'y'))
                    else:
                        for k in ('y', 'qmin', 'q1', 'q2', 'logp'):
                            eq_bits(got[k], whole[k], (regime, between, 'workspace path', k))
                one = device_sac_target(h, m['Ws'], m['bs'], *nets, x=x[TILE:], r=r[TILE:], gamma=0.98, alpha=0.2, seed=3, counter=4, row_offset=5 + TILE)
                for k in OUTPUTS:
                    eq_bits(one[k], whole[k][TILE:], (regime, between, 'row 32 alone', k))


# 6. invalid calls
def case_invalid_calls(library):
    env = AC.stepped(library, 'push', 8)
    h, d = env.handle, env.handle.dims
    Dx, A, B = 6, 3, 8
    W0, Ae = h.norm_width(POL) + d.goal_dim, d.action_dim
    nan = float('nan')
    with Dev(h) as dev:
        actor, c1, c2 = Net(h, dev, *network(81, (Dx, 16, 2 * A))), Net(h, dev, *network(82, (Dx + A, 16, 1))), Net(h, dev, *network(87, (Dx + A, 8, 8, 1)))
        odd, wide, two = Net(h, dev, *network(88, (Dx, 16, 2 * A + 1))), Net(h, dev, *network(83, (Dx + A + 1, 16, 1))), Net(h, dev, *network(84, (Dx + A, 16, 2)))
        eactor, ewrong = Net(h, dev, *network(89, (W0, 16, 2 * Ae))), Net(h, dev, *network(90, (W0, 16, Ae)))
        d_x, d_r = dev.put(np.zeros((B, 16), F32)), dev.put(np.zeros(B, F32))
        d_t, d_al = dev.put(np.zeros(B + 1, np.uint8)), dev.put(np.full(2, 0.2, F32))
        size = 4 * B * 2 * max(A, Ae)
        outs = [dev.put(np.full(size, SENTINEL, np.uint8)) for _ in range(7)]

        def mlp(net, **kw):
            m = h.mlp_struct(net.widths, net.d_w, net.d_b, 0)
            for k, v in kw.items():
                if k in ('width', 'd_weight', 'd_bias'):
                    getattr(m, k)[v[0]] = v[1]
                else:
                    setattr(m, k, v)
            return m

        def bad_nets(net):
            return [mlp(net, **kw) for kw in (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                              dict(width=(1, 0)), dict(d_weight=(0, None)), dict(out_activation=2), dict(d_weight=(1, net.d_w[1] + 2)))]

        def sample_args(A_, **kw):
            a = dict(batch=B, d_x=d_x, x_stride=Dx, d_action=outs[0], action_stride=A_, d_logp=outs[1], d_noise=outs[2], noise_stride=A_, d_preact=outs[3],
                     preact_stride=2 * A_, ls_lo=LS_LO, ls_hi=LS_HI, sample=1, seed=1, counter=2, row_offset=3)
            size_ = kw.pop('struct_size', None)
            a.update(kw)
            s = h.sac_sample_struct(**a)
            if size_ is not None:
                s.struct_size = size_
            return s

        def smp(am=None, null_s=False, **kw):
            return h.L.lib.pmg_sac_sample_device(h.h, C.byref(am or mlp(actor)), None if null_s else C.byref(sample_args(A, **kw)))

        def act(am=None, kind=POL, null_s=False, **kw):
            return h.L.lib.pmg_sac_act_env_device(h.h, C.byref(am or mlp(eactor)), C.c_int(kind), None if null_s else C.byref(sample_args(Ae, **kw)))

        def td(am=None, m1=None, m2='c2', null_td=False, **kw):
            a = dict(batch=B, d_x_next=d_x, x_stride=Dx, d_reward=d_r, d_y=outs[0], gamma=0.98, clip_lo=-50.0, clip_hi=0.0, alpha=0.2, ls_lo=LS_LO, ls_hi=LS_HI,
                     sample=1, seed=1, counter=2, row_offset=3, d_alpha=None, d_terminal=d_t + 1, d_q_min=outs[1], d_q1=outs[2], d_q2=outs[3], d_next_action=outs[4],
                     d_logp=outs[5], d_work=outs[6], work_floats=B * A)
            size_ = kw.pop('struct_size', None)
            a.update(kw)
            s = h.sac_target_struct(**a)
            if size_ is not None:
                s.struct_size = size_
            m2 = mlp(c2) if isinstance(m2, str) else m2
            return h.L.lib.pmg_sac_target_device(h.h, C.byref(am or mlp(actor)), C.byref(m1 or mlp(c1)), C.byref(m2) if m2 is not None else None,
                                                 None if null_td else C.byref(s))
        common = (dict(ls_lo=1.0, ls_hi=0.0), dict(ls_lo=nan), dict(ls_hi=nan), dict(ls_lo=-INF), dict(ls_hi=INF), dict(struct_size=0))
        bad = [lambda m=m: smp(am=m) for m in bad_nets(actor)] + [lambda m=m: td(am=m) for m in bad_nets(actor)] + [lambda m=m: td(m1=m) for m in bad_nets(c1)] + \
              [lambda m=m: td(m2=m) for m in bad_nets(c2)] + [lambda m=m: act(am=m) for m in bad_nets(eactor)] + \
              [lambda k=k: smp(**k) for k in common] + [lambda k=k: act(**k) for k in common] + [lambda k=k: td(**k) for k in common] + [
            # an odd width[L], a tanh output
            lambda: smp(am=mlp(odd)), lambda: td(am=mlp(odd)), lambda: smp(am=mlp(actor, out_activation=1)), lambda: td(am=mlp(actor, out_activation=1)),
            lambda: act(am=mlp(eactor, out_activation=1)), lambda: act(am=mlp(ewrong)), lambda: act(kind=7), lambda: act(kind=2),
            # the critics' shapes
            lambda: td(m1=mlp(wide)), lambda: td(m1=mlp(two)), lambda: td(m2=mlp(wide)), lambda: td(m2=mlp(two)),
            # the sample struct
            lambda: smp(null_s=True), lambda: act(null_s=True), lambda: smp(struct_size=C.sizeof(PmgSacSample) - 8), lambda: smp(d_x=None), lambda: smp(d_x=d_x + 2),
            lambda: smp(x_stride=Dx - 1), lambda: smp(batch=-1), lambda: smp(row_offset=-1), lambda: smp(d_action=None, d_logp=None),
            lambda: act(d_action=None, d_logp=None), lambda: smp(d_action=outs[0] + 1), lambda: smp(d_logp=outs[1] + 2), lambda: smp(d_noise=outs[2] + 3),
            lambda: smp(d_preact=outs[3] + 1), lambda: act(d_action=outs[0] + 1), lambda: smp(action_stride=A - 1), lambda: smp(noise_stride=A - 1),
            lambda: smp(preact_stride=2 * A - 1), lambda: act(action_stride=Ae - 1),
            # the target struct
            lambda: td(null_td=True), lambda: td(struct_size=C.sizeof(PmgSacTarget) - 8), lambda: td(d_x_next=None), lambda: td(d_reward=None), lambda: td(d_y=None),
            lambda: td(d_x_next=d_x + 2), lambda: td(d_reward=d_r + 1), lambda: td(d_y=outs[0] + 2), lambda: td(d_q_min=outs[1] + 1), lambda: td(d_q1=outs[2] + 3),
            lambda: td(d_q2=outs[3] + 2), lambda: td(d_next_action=outs[4] + 3), lambda: td(d_logp=outs[5] + 1), lambda: td(d_work=outs[6] + 1),
            lambda: td(d_alpha=d_al + 2), lambda: td(x_stride=Dx - 1), lambda: td(batch=-1), lambda: td(gamma=-0.1), lambda: td(gamma=INF), lambda: td(gamma=nan),
            lambda: td(clip_lo=0.0, clip_hi=-1.0), lambda: td(clip_lo=nan), lambda: td(alpha=-0.1), lambda: td(alpha=INF), lambda: td(alpha=nan),
            lambda: td(row_offset=-1), lambda: td(d_next_action=None, d_work=None), lambda: td(d_next_action=None, work_floats=B * A - 1),
            lambda: td(d_next_action=None, work_floats=0)]
        good = sample_args(A)
        assert h.L.lib.pmg_sac_sample_device(h.h, None, C.byref(good)) == E_INVALID
        assert h.L.lib.pmg_sac_target_device(h.h, None, C.byref(mlp(c1)), None, C.byref(h.sac_target_struct(B, d_x, Dx, d_r, outs[0], 0.98))) == E_INVALID
        for k, call in enumerate(bad):
            assert call() == E_INVALID, k
            assert h.L.error(h.h), k
        h.sync()
        for o in outs:
            assert (dev.get(o, size, np.uint8) == SENTINEL).all()
        assert smp(batch=0) == 0 and td(batch=0) == 0 and td(batch=0, d_next_action=None, d_work=None, work_floats=0) == 0
        h.sync()
        for o in outs:
            assert (dev.get(o, size, np.uint8) == SENTINEL).all()
        # the workspace figure
        assert h.sac_target_work_floats(mlp(actor), 0, B) == B * A and h.sac_target_work_floats(mlp(actor), 1, B) == 0
        assert h.sac_target_work_floats(mlp(actor), 0, -1) < 0 and h.sac_target_work_floats(mlp(odd), 0, B) < 0 and h.sac_target_work_floats(mlp(actor, num_layers=0), 0, B) < 0
        # what is allowed
        assert td(d_work=None, work_floats=0) == 0 and td(m2=None, d_q2=None) == 0 and td(d_alpha=d_al + 4, alpha=0.0, row_offset=2 ** 40) == 0
        assert td(d_next_action=None, d_q_min=None, d_q1=None, d_q2=None, d_logp=None, d_terminal=None, sample=0) == 0
        assert smp(d_action=None, d_noise=None, d_preact=None) == 0 and smp(d_logp=None, sample=0, ls_lo=0.0, ls_hi=0.0) == 0 and act() == 0
        h.sync()
    env.close()
    # before the first reset: PMG_E_STATE
    import pybullet_multigoal_gym_amd as pmg
    import normalizer_cases as NC
    from pybullet_multigoal_gym_amd._lib import PmgHandle
    raw = PmgHandle(library, task=0, num_envs=8, binary_reward=1, max_episode_steps=50, distance_threshold=0.05, seed_stride=1)
    try:
        W0r, Ar = raw.norm_width(POL) + raw.dims.goal_dim, raw.dims.action_dim
        with Dev(raw) as dev:
            net = Net(raw, dev, *network(91, (W0r, 8, 2 * Ar)))
            out = dev.put(np.full(4 * 8 * Ar, SENTINEL, np.uint8))
            s = raw.sac_sample_struct(0, None, 0, out, Ar, None, None, 0, None, 0, LS_LO, LS_HI, 1, 1, 2, 0)
            assert raw.L.lib.pmg_sac_act_env_device(raw.h, C.byref(net.mlp), C.c_int(POL), C.byref(s)) == E_STATE
            assert (dev.get(out, 4 * 8 * Ar, np.uint8) == SENTINEL).all()
    finally:
        raw.close()


# 7. the numpy face and the documented actor step
def recipe_nets(Dx=6, A=3):
    Wa, ba = network(1800, (Dx, 33, 2 * A))
    ba[-1][A:] = ba[-1][A:] - F32(1)
    W1, b1, W2, b2 = T3.critics(1810, Dx, A, (33,), (17, 9))
    x = np.random.RandomState(93).uniform(-2, 2, (37, Dx)).astype(F32)          # the rows of the users: either critic is the smaller on some
    a = np.tanh(forward(x, Wa, ba)[:, :A])
    b2[-1] = b2[-1] + F32(np.median(q_model(x, a, W1, b1) - q_model(x, a, W2, b2)))
    return Wa, ba, W1, b1, W2, b2


def recipe_autograd64(nets, x, n, alpha, lo=LS_LO, hi=LS_HI):
    """float64 torch autograd of mean(alpha logp - min(Q1, Q2)) with respect to the actor's parameters -> dW, db (lists)"""
    import torch
    Wa, ba, W1, b1, W2, b2 = nets
    t64 = lambda v: torch.tensor(np.asarray(v, F64))
    pa = [(t64(W).requires_grad_(), t64(b).requires_grad_()) for W, b in zip(Wa, ba)]

    def net(hh, params):
        for l, (W, b) in enumerate(params):
            hh = hh @ W.T + b
            if l + 1 < len(params):
                hh = torch.relu(hh)
        return hh
    A = Wa[-1].shape[0] // 2
    z = net(t64(x), pa)
    m, ls = z[:, :A], torch.clamp(z[:, A:], lo, hi)
    nn = t64(n)
    u = m + torch.exp(ls) * nn
    a = torch.tanh(u)
    logp = (-0.5 * nn * nn - ls - HALF_LOG_2PI - 2.0 * (LOG2 - u - torch.nn.functional.softplus(-2.0 * u))).sum(1)
    xa = torch.cat([t64(x), a], 1)
    q = torch.minimum(net(xa, [(t64(W), t64(b)) for W, b in zip(W1, b1)])[:, 0], net(xa, [(t64(W), t64(b)) for W, b in zip(W2, b2)])[:, 0])
    (alpha * logp - q).mean().backward()
    return [W.grad.numpy() for W, _ in pa], [b.grad.numpy() for _, b in pa]


def recipe_model32(nets, x, n, alpha, lo=LS_LO, hi=LS_HI):
    """the numpy float32 model of the documented step: the head, the critics' input gradients, the fix-up, the actor's backward (plain float32
    matrix products: the bar's yardstick, not a bit model) -> dW, db"""
    from pybullet_multigoal_gym_amd.sac import actor_head_grad
    Wa, ba, W1, b1, W2, b2 = nets
    B, A = x.shape[0], Wa[-1].shape[0] // 2

    def fwd(hh, Ws, bs):
        hs = [hh]
        for l, (W, b) in enumerate(zip(Ws, bs)):
            hh = hh @ W.T + b
            if l + 1 < len(Ws):
                hh = np.maximum(hh, F32(0))
            hs.append(hh)
        return hs

    def back(hs, Ws, g):
        dW, db = [], []
        for l in range(len(Ws) - 1, -1, -1):
            dW.insert(0, g.T @ hs[l])
            db.insert(0, g.sum(0))
            g = g @ Ws[l]
            if l:
                g = np.where(hs[l] > 0, g, F32(0))
        return dW, db, g
    hs = fwd(x, Wa, ba)
    z = hs[-1]
    a, _ = head32(z, n, lo, hi)
    xa = np.concatenate([x, a], 1)
    gas, qs = [], []
    for W, b in ((W1, b1), (W2, b2)):
        hc = fwd(xa, W, b)
        qs.append(hc[-1][:, 0])
        gas.append(back(hc, W, np.full((B, 1), -1.0 / B, F32))[2][:, x.shape[1]:])
    ga = np.where((qs[0] <= qs[1])[:, None], gas[0], gas[1])
    gout = actor_head_grad(a, n, z, ga, alpha, lo, hi)
    dW, db, _ = back(hs, Wa, gout)
    return dW, db


# measured by test_sac_host.test_recipe_bar (the numpy float32 model of the step against float64 autograd, relative to the largest |entry| of
# each tensor, the worst tensor): 4.16e-7; the bar is 4 x that.  Observed: emulator 3.01e-7, MI355X 3.01e-7
RECIPE_MEASURED = 4.2e-7
RECIPE_TOL = 4 * RECIPE_MEASURED


def recipe_error(got_dW, got_db, want_dW, want_db):
    return max(float(np.abs(np.asarray(g, F64) - w).max() / np.abs(w).max()) for g, w in zip(list(got_dW) + list(got_db), list(want_dW) + list(want_db)))


def case_host_face(library):
    import pytest
    from pybullet_multigoal_gym_amd.critic import Critic
    from pybullet_multigoal_gym_amd.sac import GaussianActor, actor_head_grad
    env = AC.stepped(library, 'reach', 8)
    Dx, A, B = 6, 3, 37
    nets = recipe_nets(Dx, A)
    Wa, ba, W1, b1, W2, b2 = nets
    pi, critic, critic2 = env.gaussian_actor, env.critic, Critic(env)
    assert pi is env.gaussian_actor and isinstance(pi, GaussianActor)
    rs = np.random.RandomState(93)
    x, r = rs.uniform(-2, 2, (B, Dx)).astype(F32), -rs.randint(0, 2, B).astype(F32)
    term = rs.randint(0, 2, B).astype(bool)
    with pytest.raises(ValueError):
        pi.sample(x)                                                 # nothing loaded
    with pytest.raises(ValueError):
        pi.load(Wa[:-1] + [Wa[-1][:-1]], ba[:-1] + [ba[-1][:-1]])    # an odd number of outputs
    pi.load(Wa, ba)
    critic.load(W1, b1)
    critic2.load(W2, b2)
    z_model = forward(x, Wa, ba)
    # sample
    a, logp, n, z = pi.sample(x, seed=4, counter=5, row_offset=6, preact=True)
    check_z(z, z_model, 'z')
    u1, u2 = draws(4, 5, 6, B, A)
    check_head({'a': a, 'logp': logp, 'n': n}, z_model, u1, u2, LS_LO, LS_HI, 'GaussianActor.sample')
    a0, logp0, n0 = pi.sample(x, sample=False)
    assert (bits(n0) == 0).all() and np.abs(a0 - np.tanh(z_model[:, :A].astype(F64))).max() <= SAC_A_TOL
    assert pi.sample(x[:0])[0].shape == (0, A) and pi.sample(x[:0])[1].shape == (0,)
    # the soft target
    assert critic.sac_target_work_floats(pi, B) == B * A and critic.sac_target_work_floats(pi, B, next_action=True) == 0
    for kw in ({}, {'clip_lo': -50.0, 'clip_hi': 0.0, 'terminal': term}):
        y, qm, q1, q2, na, lp = critic.sac_target(pi, critic2, x, r, 0.98, 0.2, seed=4, counter=5, row_offset=6, **kw)
        eq_bits(na, a, 'the target samples what sample() samples')
        eq_bits(lp, logp, 'logp')
        eq_bits(q1, q_model(x, na, W1, b1), 'q1')
        eq_bits(q2, q_model(x, na, W2, b2), 'q2')
        eq_bits(qm + F32(0), np.minimum(q1, q2) + F32(0), 'qmin')
        eq_y(y, soft_epilogue(np.minimum(q1, q2), lp, r, 0.98, 0.2, kw.get('clip_lo', -INF), kw.get('clip_hi', INF), kw.get('terminal'))[1], 'y')
    y1, qm1, q11, q21, na1, lp1 = critic.sac_target(pi, None, x, r, 0.98, 0.2, seed=4, counter=5, row_offset=6)
    assert q21 is None
    eq_bits(q11, q1, 'one critic')
    eq_bits(qm1, q1, 'one critic: qmin')
    assert critic.sac_target(pi, critic2, x[:0], r[:0], 0.98, 0.2)[4].shape == (0, A)
    # env rows
    W0 = env.handle.norm_width(POL) + env.handle.dims.goal_dim
    We, be = network(1820, (W0, 33, 2 * env.dims.action_dim))
    epi = GaussianActor(env)
    epi.load(We, be)
    ea, elp = epi.act(seed=8, counter=9)
    want = device_sample(env.handle, We, be, AC.policy_rows(env.handle, POL), seed=8, counter=9, row_offset=0)
    eq_bits(ea, want['a'], 'act: a')
    eq_bits(elp, want['logp'], 'act: logp')
    with pytest.raises(ValueError):
        epi.act(kind='goal')
    epi.close()
    # the documented actor step, assembled from existing calls, against float64 autograd
    alpha = 0.2
    q1 = critic.q(x, a)
    q2 = critic2.q(x, a)
    ga1 = critic.grad(x, a, gscale=-1.0 / B, grads=False)['ga']
    ga2 = critic2.grad(x, a, gscale=-1.0 / B, grads=False)['ga']
    gout = actor_head_grad(a, n, z, np.where((q1 <= q2)[:, None], ga1, ga2), alpha)
    res = pi.grad(x, gout=gout)
    want_dW, want_db = recipe_autograd64(nets, x, n, alpha)
    err = recipe_error(res['dW'], res['db'], want_dW, want_db)
    print('the SAC actor step against float64 autograd: %.3g (bar %.3g)' % (err, RECIPE_TOL))
    assert (q1 < q2).any() and (q2 < q1).any()
    assert err <= RECIPE_TOL, err
    # refused arguments
    for call in (lambda: pi.sample(x[:, :-1]), lambda: pi.sample(x, ls_lo=1.0, ls_hi=0.0), lambda: pi.sample(x, ls_lo=float('nan')), lambda: pi.sample(x, row_offset=-1),
                 lambda: critic.sac_target(pi, critic2, x, r, 0.98, -0.1), lambda: critic.sac_target(pi, critic2, x, r, 0.98, INF),
                 lambda: critic.sac_target(pi, critic2, x, r[:-1], 0.98, 0.2), lambda: critic.sac_target(env.actor, critic2, x, r, 0.98, 0.2),
                 lambda: critic.sac_target(pi, critic2, x, r, -1.0, 0.2), lambda: critic.sac_target(pi, critic2, x, r, 0.98, 0.2, ls_lo=3.0),
                 lambda: critic.sac_target(pi, critic2, x, r, 0.98, 0.2, row_offset=-1), lambda: critic.sac_target(pi, pi, x, r, 0.98, 0.2)):
        with pytest.raises(ValueError):
            call()
    critic2.close()
    pi.close()
    with pytest.raises(ValueError):
        pi.sample(x)
    env.close()
    return err


# 8. what tests/test_sac_wave_order.py runs under every wavefront order
def wave_order_run(library):
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        shapes = {'wide': (3, 12, (256, 256, 256), (256,), (33, 255), 33), 'far': (1, 20, (33,), (64,), (), 32), 'small': (6, 3, (33,), (33,), (33,), 33)}
        for name, (Dx, A, ah, h1, h2, B) in shapes.items():
            m = sample_case(Dx, A, ah)
            nets = T3.critics(1900 + Dx, Dx, A, h1, h2)
            r = -np.random.RandomState(Dx).randint(0, 2, B).astype(F32)
            for null in ((), ('a',)):
                got = device_sac_target(h, m['Ws'], m['bs'], *nets, x=m['x'][:B], r=r, gamma=0.98, lo=-50.0, hi=0.0, alpha=0.2, seed=3, counter=4, row_offset=5,
                                        x_pad=1, shift=1, null=null)
                for k in OUTPUTS:
                    if got[k] is not None:
                        res[name + k + str(len(null))] = got[k]
            got = device_sample(h, m['Ws'], m['bs'], m['x'][:B], seed=3, counter=4, row_offset=5, shift=1)
            for k, v in got.items():
                res[name + 'sample' + k] = v
    return res
