"""The cases of the fused SAC actor update (include/pmg.h pmg_sac_policy_grad_device, pmg_sac_alpha_device) and their numpy model,
shared by four files: tests/test_sac_pg_emulated.py runs them on the g++ build of the product sources over the fiber emulator,
tests/test_gpu_sac_pg.py on libpmg_hip.so on the MI355X, tests/test_sac_pg_host.py covers the model alone, tests/test_sac_pg_wave_order.py the
kernel under permuted wavefront order.  The pieces are those of tests/sac_cases.py (the head, the draws), tests/policy_grad_cases.py and
tests/grad_cases.py / tests/grad_chunk_cases.py (the exact fmaf chains of the backward, the device calls of the sequence) and tests/td_cases.py /
tests/td3_cases.py (the critics, the stale regimes).

Bars.  a, logp, q1, q2, ga, dW and db are held bit for bit (zeros by value) to EXISTING calls on the same library: pmg_sac_sample_device,
pmg_q_device on the call's own a, the input-only pmg_mlp_grad_device of either critic on x | a, pmg_mlp_grad[_chunked]_device of the actor on
the call's own d_ghead.  g_mu is bit-defined from the call's own a, ga and e.  g_ls goes through the build's expf (sd): it is held to the
float32 model from the call's own a and ga and the sample call's n and z,
  SAC_PG_LS_TOL   |g_ls - model| relative to |e| (|2 a sdn| + 1) + |d sdn|, the magnitudes of the summands;
the whole gradient is held to float64 autograd,
  SAC_PG_TOL      |t - t64| relative to the largest |entry| of each tensor t of dW / db, the worst tensor;
and alpha = expf(log_alpha) to exp in float64,
  SAC_ALPHA_TOL   relative.
Each bar is 4 x the error MEASURED on the numpy float32 model alone (measure_* below, run by tests/test_sac_pg_host.py), the headroom the
project gives library functions that differ by an ulp or two between numpy and a build.  None of them comes from a device's output."""
import ctypes as C

import numpy as np

import actor_cases as AC
import grad_cases as GC
import grad_chunk_cases as GCC
import policy_grad_cases as PG
import sac_cases as SC
import td3_cases as T3
import td_cases as TC
from actor_cases import Net, bits, fmaf, forward, network
from grad_cases import Params, eq_val, read_rows, rows_out
from normalizer_cases import SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PmgMlp, PmgSacAlpha, PmgSacPolicyGrad
from td_cases import Out, eq_bits, put_rows, q_model

E_INVALID = -1
F32, F64 = np.float32, np.float64
TILE = AC.TILE
INF = float('inf')
LS_LO, LS_HI = SC.LS_LO, SC.LS_HI
PAIRS = SC.PAIRS
BATCHES = TC.BATCHES
OUTPUTS = ('a', 'logp', 'q1', 'q2', 'ga', 'ghead')
NAN_WORD = 0x7FC00000 | 0x1234
# measured by measure_ls_bar() over every input of CASES (numpy float32 restatement of g_ls against float64; x86-64 glibc / numpy): 2.361e-7
SAC_PG_LS_MEASURED = 2.4e-7
SAC_PG_LS_TOL = 4 * SAC_PG_LS_MEASURED
# measured by measure_model_bar() (the numpy float32 model of steps 1-6 against float64 autograd, MODEL_NETS): 1.425e-6
SAC_PG_MEASURED = 1.43e-6
SAC_PG_TOL = 4 * SAC_PG_MEASURED
# measured by measure_alpha_bar() (numpy float32 exp against float64 over ALPHA_LOGS): 1.252e-7
SAC_ALPHA_MEASURED = 1.26e-7
SAC_ALPHA_TOL = 4 * SAC_ALPHA_MEASURED
# (Dx, A, actor hidden, critic 1 hidden, critic 2 hidden, bias, B, chunk_rows, critic activations): every pair, the hidden shapes mixed, critic 2's
# depth unlike critic 1's, every batch and every chunk regime at B = 101
CASES = ((6, 3, (33,), (33,), (64, 33), True, 101, None, (0, 0)),
         (6, 3, (), (256, 256, 256), (), False, 33, 2, (0, 1)),
         (1, 1, (33,), (), (33,), True, 1, None, (1, 0)),
         (2, 5, (256, 256, 256), (33,), (), True, 31, None, (0, 0)),
         (3, 12, (33,), (33,), (256, 256, 256), True, 101, 2, (0, 0)),
         (29, 4, (256, 256, 256), (256,), (33, 255, 31), False, 32, None, (0, 0)),
         (1, 20, (), (33,), (64, 33), True, 101, 32, (0, 0)),
         (5, 9, (33,), (256, 256, 256), (33,), True, 101, 128, (0, 0)))


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def head_grad(a, ga, e, n, z, lo=LS_LO, hi=LS_HI):
    """step 5 in float32 from a, ga [B, A], e = lscale * alpha (float32), n [B, A], z [B, 2 A] -> g_mu (bit-defined), g_ls (numpy's exp standing
    in for the build's), inrange, mag (the magnitudes of g_ls's summands)"""
    a, ga, n, z = (np.asarray(v, F32) for v in (a, ga, n, z))
    A, e = a.shape[1], F32(e)
    one = np.ones(a.shape, F32)
    with np.errstate(over='ignore', invalid='ignore'):
        t = fmaf(-a, a, one).reshape(a.shape)
        d = ga * t
        g_mu = fmaf(np.full(a.shape, F32(2) * e, F32), a, d).reshape(a.shape)
        raw = z[:, A:]
        inr = (raw >= F32(lo)) & (raw <= F32(hi))
        sdn = np.exp(np.minimum(np.maximum(raw, F32(lo)), F32(hi))) * n
        inner = fmaf(F32(2) * a, sdn, -one).reshape(a.shape)
        g_ls = np.where(inr, fmaf(np.full(a.shape, e, F32), inner, d * sdn).reshape(a.shape), F32(0))
        mag = np.abs(e) * (np.abs(F32(2) * a * sdn) + 1) + np.abs(d * sdn)
    return g_mu, g_ls, inr, mag


def g_ls64(a, ga, e, n, z, lo=LS_LO, hi=LS_HI):
    a, ga, n, z = (np.asarray(v, F32).astype(F64) for v in (a, ga, n, z))
    A = a.shape[1]
    raw = z[:, A:]
    sdn = np.exp(np.clip(raw, float(F32(lo)), float(F32(hi)))) * n
    d = ga * (1.0 - a * a)
    return np.where((raw >= float(F32(lo))) & (raw <= float(F32(hi))), float(F32(e)) * (2.0 * a * sdn - 1.0) + d * sdn, 0.0)


def spg_case(Dx, A, ah, h1, h2, bias=True, B=101, acts=(0, 0)):
    """sac_cases' actor for (Dx, A, ah) (without its biases where bias is False) and two critics whose outputs cross on its rows"""
    def make():
        m = SC.sample_case(Dx, A, ah)
        Ws, bs = [w.copy() for w in m['Ws']], ([b.copy() for b in m['bs']] if bias else None)
        if not bias:                                              # keep the log-stds spread over the clamp: fold their offset into nothing, rescale
            Ws[-1][A:] = Ws[-1][A:] * F32(0.25)
        x = m['x'][:B]
        W1, b1, W2, b2 = T3.critics(2100 + 31 * Dx + A, Dx, A, h1, h2)
        if not bias:
            b1 = b2 = None
        else:
            a0 = np.tanh(forward(x, Ws, bs)[:, :A])
            with np.errstate(over='ignore'):
                z1, z2 = forward(np.concatenate([x, a0], 1), W1, b1)[:, 0], forward(np.concatenate([x, a0], 1), W2, b2)[:, 0]
            b2[-1] = b2[-1] + F32(np.median(z1 - z2))                   # either critic is the smaller on some rows
        return {'Ws': Ws, 'bs': bs, 'x': x, 'z': forward(x, Ws, bs), 'nets': (W1, b1, W2, b2)}
    return TC.cached(('sac pg', Dx, A, tuple(ah), tuple(h1), tuple(h2), bias, B, acts), make)


def clamp_of(k):
    """the clamp of case k: SAC's usual one, and a narrow one that the raw log-stds of every case leave on both sides"""
    return (LS_LO, LS_HI) if k % 2 == 0 else (-4.0, 1.0)


def measure_ls_bar(cases=CASES):
    """-> the largest |g_ls32 - g_ls64| / mag over the cases' own inputs: a from the float32 head, ga of the model's critics, the draws' n"""
    worst = 0.0
    for k, (Dx, A, ah, h1, h2, bias, B, R, acts) in enumerate(cases):
        c = spg_case(Dx, A, ah, h1, h2, bias, B, acts)
        n = SC.n32_of(*SC.draws(*SC.SEEDS(k), B, A))
        lo, hi = clamp_of(k)
        a = SC.head32(c['z'], n, lo, hi)[0]
        ga = GC.model(c['x'], c['nets'][0], c['nets'][1], acts[0], gscale=-1.0 / B, a=a, weights=False)['ga']
        e = F32(1.0 / B) * F32(0.2)
        _, g32, inr, mag = head_grad(a, ga, e, n, c['z'], lo, hi)
        err = np.abs(g32.astype(F64) - g_ls64(a, ga, e, n, c['z'], lo, hi)) / mag
        worst = max(worst, float(err[inr].max()) if inr.any() else 0.0)
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# float64 autograd and the float32 model of steps 1 - 6 (CPU only: tests/test_sac_pg_host.py; the device is then held to the same bar)
MODEL_NETS = (((6, 256, 256, 256, 6), (256, 256, 256), (33,)), ((5, 33, 8), (33,), (17, 9)))
MODEL_B = 33


def model_case(k):
    def make():
        widths, h1, h2 = MODEL_NETS[k]
        Dx, A = widths[0], widths[-1] // 2
        Wa, ba = GC.net(2300 + k, widths)
        ba[-1][A:] = ba[-1][A:] - F32(1)
        (W1, b1), (W2, b2) = GC.net(2310 + k, (Dx + A,) + tuple(h1) + (1,)), GC.net(2311 + k, (Dx + A,) + tuple(h2) + (1,))
        x = np.random.RandomState(230 + k).uniform(-2, 2, (MODEL_B, Dx)).astype(F32)
        Wa[-1][A:] = Wa[-1][A:] * F32(16 if len(widths) > 3 else 4)   # raw log-stds on both sides of the clamp [-2, 0.5] of the users
        a = np.tanh(forward(x, Wa, ba)[:, :A])
        b2[-1] = b2[-1] + F32(np.median(q_model(x, a, W1, b1) - q_model(x, a, W2, b2)))
        n = SC.n32_of(*SC.draws(7 + k, 8, 9, MODEL_B, A))
        return {'nets': (Wa, ba, W1, b1, W2, b2), 'x': x, 'n': n, 'seeds': (7 + k, 8, 9)}
    return TC.cached(('sac pg model', k), make)


MODEL_LS = (-2.0, 0.5)


def autograd64(nets, x, n, alpha, lscale, gscale, lo, hi):
    """float64 torch autograd of lscale alpha sum logp + gscale sum min(Q1, Q2) -> dict(dW, db, masks (actor), inrange, first (q1 <= q2))"""
    import torch
    Wa, ba, W1, b1, W2, b2 = nets
    t64 = lambda v: torch.tensor(np.asarray(v, F64))
    pa = [(t64(W).requires_grad_(), t64(b).requires_grad_()) for W, b in zip(Wa, ba)]
    masks = []

    def net(hh, params, keep=None):
        for l, (W, b) in enumerate(params):
            hh = hh @ W.T + b
            if l + 1 < len(params):
                if keep is not None:
                    keep.append((hh > 0).numpy())
                hh = torch.relu(hh)
        return hh
    A = Wa[-1].shape[0] // 2
    z = net(t64(x), pa, masks)
    raw = z[:, A:]
    m, ls = z[:, :A], torch.clamp(raw, lo, hi)
    nn = t64(n)
    u = m + torch.exp(ls) * nn
    a = torch.tanh(u)
    logp = (-0.5 * nn * nn - ls - SC.HALF_LOG_2PI - 2.0 * (SC.LOG2 - u - torch.nn.functional.softplus(-2.0 * u))).sum(1)
    xa = torch.cat([t64(x), a], 1)
    q1, q2 = (net(xa, [(t64(W), t64(b)) for W, b in zip(Wc, bc)])[:, 0] for Wc, bc in ((W1, b1), (W2, b2)))
    (lscale * alpha * logp.sum() + gscale * torch.minimum(q1, q2).sum()).backward()
    return {'dW': [W.grad.numpy() for W, _ in pa], 'db': [b.grad.numpy() for _, b in pa], 'masks': masks,
            'inrange': ((raw >= lo) & (raw <= hi)).detach().numpy(), 'first': (q1 <= q2).detach().numpy()}


def model32(nets, x, n, alpha, lscale, gscale, lo, hi):
    """the numpy float32 model of steps 1 - 6: sac_cases' head, the exact chains of grad_cases for the critics' input gradients and the actor's
    backward, head_grad -> dict(dW, db, masks, inrange, first, a, ga, ghead, q1, q2)"""
    Wa, ba, W1, b1, W2, b2 = nets
    A = Wa[-1].shape[0] // 2
    z = forward(x, Wa, ba)
    a = SC.head32(z, n, lo, hi)[0]
    c1 = GC.model(x, W1, b1, gscale=gscale, a=a, weights=False)
    c2 = GC.model(x, W2, b2, gscale=gscale, a=a, weights=False)
    q1, q2 = c1['out'][:, 0], c2['out'][:, 0]
    first = q1 <= q2
    ga = np.where(first[:, None], c1['ga'], c2['ga'])
    g_mu, g_ls, inr, _ = head_grad(a, ga, F32(lscale) * F32(alpha), n, z, lo, hi)
    ghead = np.concatenate([g_mu, g_ls], 1)
    m = GC.model(x, Wa, ba, gout=ghead)
    return {'dW': m['dW'], 'db': m['db'], 'masks': m['masks'], 'inrange': inr, 'first': first, 'a': a, 'ga': ga, 'ghead': ghead, 'q1': q1, 'q2': q2}


def measure_model_bar():
    """-> the largest error of model32 against autograd64 over MODEL_NETS, having asserted that both took the same branches"""
    worst = 0.0
    for k in range(len(MODEL_NETS)):
        c = model_case(k)
        B = c['x'].shape[0]
        args = (c['nets'], c['x'], c['n'], 0.2, 1.0 / B, -1.0 / B) + MODEL_LS
        w, m = autograd64(*args), model32(*args)
        assert all(np.array_equal(u, v) for u, v in zip(w['masks'], m['masks'])), 'ReLU masks differ'
        assert np.array_equal(w['inrange'], m['inrange']) and np.array_equal(w['first'], m['first'])
        assert w['first'].any() and not w['first'].all() and w['inrange'].any() and not w['inrange'].all()
        worst = max(worst, SC.recipe_error(m['dW'], m['db'], w['dW'], w['db']))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# device calls
def device_sac_pg(h, Wa, ba, W1, b1, W2, b2, x, gscale, lscale, alpha=0.2, lo=LS_LO, hi=LS_HI, sample=1, seed=0, counter=0, row_offset=0, d_alpha=None,
                  grads=True, null=(), pad=0, shift=0, R=None, c1_out=0, c2_out=0, twice=False, nan_work=False):
    """pmg_sac_policy_grad_device on canary-framed, sentinel-filled outputs -> dict(dW, db, a, logp, q1, q2, ga, ghead) (None for what was passed
    as NULL).  pad: floats of poison behind every input row and of sentinel between output rows; shift: the phase of the first float pointer,
    the others follow in turn.  The workspace is sized EXACTLY pmg_sac_policy_grad_work_floats and canary-framed; with grads NULL its first
    pmg_mlp_grad_work_floats floats -- the actor's part -- must come back untouched, and all of it when nothing has to be kept.  nan_work: it
    starts as NaN bit patterns.  d_alpha: a value put into device memory and passed as d_alpha (the struct's alpha is then 0)."""
    B, A = x.shape[0], Wa[-1].shape[0] // 2
    twin = W2 is not None
    with Dev(h) as dev:
        actor, c1 = Net(h, dev, Wa, ba, 0), Net(h, dev, W1, b1, c1_out)
        c2 = Net(h, dev, W2, b2, c2_out) if twin else None
        d_x, xs = put_rows(h, dev, x, pad, shift)
        d_al = None
        if d_alpha is not None:
            d_al, _ = put_rows(h, dev, np.array([[d_alpha]], F32), 0, (shift + 2) & 3)
        outs = {'a': rows_out(dev, B, A, pad, (shift + 1) & 3), 'logp': Out(dev, 4 * B, 4 * ((shift + 2) & 3)), 'q1': Out(dev, 4 * B, 4 * ((shift + 3) & 3)),
                'q2': Out(dev, 4 * B, 4 * (shift & 3)), 'ga': rows_out(dev, B, A, pad, (shift + 1) & 3), 'ghead': rows_out(dev, B, 2 * A, pad, (shift + 2) & 3)}
        par = Params(h, dev, Wa, ba, shift)
        work = h.sac_policy_grad_work_floats(actor.mlp, 'a' not in null, twin, B, R or 0)
        base = h.mlp_grad_work_floats(actor.mlp, B)
        mine = h.mlp_grad_chunked_work_floats(actor.mlp, B, R) if R else base
        assert work == mine + (B * A if 'a' in null else 0) + (B * A if twin else 0) and base >= 0
        o_work = Out(dev, 4 * work, 4 * ((shift + 1) & 3))
        if nan_work and work:
            h.upload(o_work.ptr, np.full(work, NAN_WORD, np.uint32))
        ptr = lambda k: None if k in null else outs[k].ptr
        g = h.sac_policy_grad_struct(B, d_x, xs, o_work.ptr, work, gscale, lscale, 0.0 if d_alpha is not None else alpha, lo, hi, sample, seed, counter,
                                     row_offset, d_al, par.struct if grads else None, ptr('a'), A + pad, ptr('logp'), ptr('q1'), ptr('q2'), ptr('ga'), A + pad,
                                     ptr('ghead'), 2 * A + pad)
        for _ in range(2 if twice else 1):
            h.sac_policy_grad_device(actor.mlp, c1.mlp, c2.mlp if twin else None, g, R or 0)
        h.sync()
        raw = o_work.read(np.uint32 if work else np.uint8)            # (the canaries around it are checked)
        if not grads and work:
            back = 'ga' not in null or 'ghead' not in null
            untouched = raw[:base] if ('a' in null or (twin and back)) else raw
            fill = NAN_WORD if nan_work else int(np.array([SENTINEL] * 4, np.uint8).view(np.uint32)[0])
            assert (untouched == fill).all(), "without grads the actor's part of the workspace was written"
        dW, db = par.read(written=grads)
        res = {'dW': dW, 'db': db}
        for k, W in (('a', A), ('ga', A), ('ghead', 2 * A)):
            res[k] = read_rows(outs[k], B, W, pad, k not in null)
        for k in ('logp', 'q1', 'q2'):
            res[k] = outs[k].read(written=k not in null and not (k == 'q2' and not twin))
        for net, Ws in ((actor, Wa), (c1, W1)) + (((c2, W2),) if twin else ()):       # no network's weights are written
            for p, W in zip(net.d_w, Ws):
                assert np.array_equal(bits(dev.get(p, W.shape, F32)), bits(W)), 'a weight was written'
        return res


def device_sequence(h, Wa, ba, W1, b1, W2, b2, x, gscale, own, lo=LS_LO, hi=LS_HI, sample=1, seed=0, counter=0, row_offset=0, R=None, c1_out=0, c2_out=0,
                    grads=True):
    """the existing calls the fused call is defined by, on the fused call's OWN a and d_ghead -> dict(a, logp, n, z, q1, q2, ga, first, dW, db)"""
    s = SC.device_sample(h, Wa, ba, x, lo, hi, sample, seed, counter, row_offset)
    a = own['a'] if own.get('a') is not None else s['a']
    q1, q2 = T3.device_qs(h, W1, b1, W2, b2, x, a, c1_out, c2_out)
    with np.errstate(over='ignore', invalid='ignore'):
        ga1 = GC.device_grad(h, W1, b1, x, a, c1_out, gscale=gscale, grads=False, null=('gx',))['ga']
        ga2 = GC.device_grad(h, W2, b2, x, a, c2_out, gscale=gscale, grads=False, null=('gx',))['ga'] if W2 is not None else None
    first = np.ones(x.shape[0], bool) if W2 is None else q1 <= q2
    res = dict(s, q1=q1, q2=q2, first=first, ga=ga1 if W2 is None else np.where(first[:, None], ga1, ga2), dW=None, db=None)
    if grads and own.get('ghead') is not None:
        p = GC.device_grad(h, Wa, ba, x, None, 0, gout=own['ghead'], null=('gx',)) if R is None or R >= x.shape[0] else \
            GCC.device_grad_chunked(h, Wa, ba, x, R, None, 0, gout=own['ghead'], null=('gx',))
        res.update(dW=p['dW'], db=p['db'])
    return res


def check_sequence(got, seq, label):
    """test 1: bit for bit (zeros by value) against the existing calls"""
    for k in ('a', 'logp', 'q1', 'q2', 'ga'):
        if got.get(k) is not None and seq[k] is not None:
            eq_val(got[k], seq[k], (label, k))
    if got['dW'] is not None and seq['dW'] is not None:
        PG.check(got, seq, label, ('dW', 'db'))


def check_head_grad(got, n, z, e, lo, hi, label):
    """test 2: g_mu exact from the call's own a, ga and e; g_ls against the float32 model -> its largest relative error"""
    A = got['a'].shape[1]
    g_mu, g_ls, inr, mag = head_grad(got['a'], got['ga'], e, n, z, lo, hi)
    eq_val(got['ghead'][:, :A], g_mu, (label, 'g_mu'))
    out = got['ghead'][:, A:]
    assert (bits(out[~inr]) == 0).all(), (label, 'g_ls is +0.0 outside the clamp')
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs(out.astype(F64) - g_ls.astype(F64)) / mag
    worst = float(err[inr].max()) if inr.any() else 0.0
    assert worst <= SAC_PG_LS_TOL, (label, 'g_ls', worst)
    return worst


def run_both(h, c, k, gscale, lscale, alpha, R=None, acts=(0, 0), twin=True, **kw):
    """the fused call and the sequence on case c with the seeds and the clamp of case k -> got, seq"""
    seed, counter, off = SC.SEEDS(k)
    lo, hi = clamp_of(k)
    W1, b1, W2, b2 = c['nets'] if twin else (c['nets'][0], c['nets'][1], None, None)
    got = device_sac_pg(h, c['Ws'], c['bs'], W1, b1, W2, b2, c['x'], gscale, lscale, alpha, lo, hi, seed=seed, counter=counter, row_offset=off, R=R,
                        c1_out=acts[0], c2_out=acts[1], **kw)
    seq = device_sequence(h, c['Ws'], c['bs'], W1, b1, W2, b2, c['x'], gscale, got, lo, hi, seed=seed, counter=counter, row_offset=off, R=R, c1_out=acts[0],
                          c2_out=acts[1], grads=kw.get('grads', True))
    return got, seq


# ----------------------------------------------------------------------------------------------------------------------
# 1 + 2. against existing calls, and the head gradient
def case_sequence(library, cases=CASES):
    seen, worst = set(), 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for case in cases:
            k = CASES.index(case)
            Dx, A, ah, h1, h2, bias, B, R, acts = case
            c = spg_case(Dx, A, ah, h1, h2, bias, B, acts)
            alpha, lscale, gscale = 0.2, 1.0 / B, -1.0 / B
            got, seq = run_both(h, c, k, gscale, lscale, alpha, R, acts, pad=k % 3, shift=k % 4, nan_work=bool(k & 1))
            SC.check_z(seq['z'], c['z'], (case, 'z'))
            check_sequence(got, seq, case)
            lo, hi = clamp_of(k)
            worst = max(worst, check_head_grad(got, seq['n'], seq['z'], F32(lscale) * F32(alpha), lo, hi, case))
            raw = seq['z'][:, A:]
            seen |= {s for s, hit in (('q1 < q2', got['q1'] < got['q2']), ('q2 < q1', got['q2'] < got['q1']), ('below', raw < F32(lo)),
                                      ('inside', (raw > F32(lo)) & (raw < F32(hi))), ('above', raw > F32(hi))) if hit.any()}
            # the workspace path of a (d_action NULL) and one critic give the same rows
            if k % 2 == 0:
                ws = device_sac_pg(h, c['Ws'], c['bs'], *c['nets'], c['x'], gscale, lscale, alpha, lo, hi, seed=SC.SEEDS(k)[0], counter=SC.SEEDS(k)[1],
                                   row_offset=SC.SEEDS(k)[2], R=R, c1_out=acts[0], c2_out=acts[1], null=('a',), shift=(k + 1) % 4)
                for key in ('logp', 'q1', 'q2', 'ga', 'ghead'):
                    eq_bits(ws[key], got[key], (case, 'a in the workspace', key))
                for u, v in zip(ws['dW'] + [t for t in ws['db'] if t is not None], got['dW'] + [t for t in got['db'] if t is not None]):
                    eq_bits(u, v, (case, 'a in the workspace', 'dW / db'))
    print('head gradient: largest |g_ls - model| / magnitude = %.3g (bar %.3g)' % (worst, SAC_PG_LS_TOL))
    if len(cases) == len(CASES):
        assert seen == COVERAGE, seen
    return worst, seen


COVERAGE = {'q1 < q2', 'q2 < q1', 'below', 'inside', 'above'}


def model_coverage(cases=CASES):
    """what the cases cover, from the model alone: both orders of the critics (on the float32 head's a) and the three sides of the clamp"""
    seen = set()
    for k, (Dx, A, ah, h1, h2, bias, B, R, acts) in enumerate(cases):
        c = spg_case(Dx, A, ah, h1, h2, bias, B, acts)
        lo, hi = clamp_of(k)
        a = SC.head32(c['z'], SC.n32_of(*SC.draws(*SC.SEEDS(k), B, A)), lo, hi)[0]
        q1 = GC.model(c['x'], c['nets'][0], c['nets'][1], acts[0], a=a, weights=False)['out'][:, 0]
        q2 = GC.model(c['x'], c['nets'][2], c['nets'][3], acts[1], a=a, weights=False)['out'][:, 0]
        raw = c['z'][:, A:]
        seen |= {s for s, hit in (('q1 < q2', q1 < q2), ('q2 < q1', q2 < q1), ('below', raw < F32(lo)), ('inside', (raw > F32(lo)) & (raw < F32(hi))),
                                  ('above', raw > F32(hi))) if hit.any()}
    return seen


# 3. the device against float64 autograd
def case_autograd(library):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for k in range(len(MODEL_NETS)):
            c = model_case(k)
            Wa, ba, W1, b1, W2, b2 = c['nets']
            B = c['x'].shape[0]
            seed, counter, off = c['seeds']
            got = device_sac_pg(h, Wa, ba, W1, b1, W2, b2, c['x'], -1.0 / B, 1.0 / B, 0.2, MODEL_LS[0], MODEL_LS[1], seed=seed, counter=counter, row_offset=off)
            n = SC.device_sample(h, Wa, ba, c['x'], MODEL_LS[0], MODEL_LS[1], 1, seed, counter, off)['n']
            w = autograd64(c['nets'], c['x'], n, 0.2, 1.0 / B, -1.0 / B, *MODEL_LS)
            assert np.array_equal(w['first'], got['q1'] <= got['q2']), 'the device picked another critic than float64'
            worst = max(worst, SC.recipe_error(got['dW'], got['db'], w['dW'], w['db']))
    print('the fused SAC actor gradient against float64 autograd: %.3g (bar %.3g)' % (worst, SAC_PG_TOL))
    assert worst <= SAC_PG_TOL, worst
    return worst


# 4. the DDPG kernel
def case_is_policy_grad(library, pairs=PAIRS):
    """sample == 0, lscale == 0, one critic: a, q and ga are pmg_policy_grad_device's (l2scale = 0) on the tanh actor whose last layer is the mean
    half; dW / db equal by value on every layer and on the mean rows of the last one, the log-std rows are zero"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A) in enumerate(pairs):
            ah, ch = SC.HIDDEN[(n + 1) % 3], SC.HIDDEN[n % 3]
            m = SC.sample_case(Dx, A, ah)
            B = BATCHES[n % len(BATCHES)]
            x = m['x'][:B]
            Wc, bc = network(2400 + n, (Dx + A,) + tuple(ch) + (1,))
            R = (None, 2, 32)[n % 3]
            got = device_sac_pg(h, m['Ws'], m['bs'], Wc, bc, None, None, x, -1.0 / B, 0.0, 0.2, sample=0, R=R, c1_out=n & 1, pad=1, shift=n % 4)
            Wm, bm = m['Ws'][:-1] + [m['Ws'][-1][:A]], m['bs'][:-1] + [m['bs'][-1][:A]]
            old = PG.device_policy_grad(h, Wm, bm, Wc, bc, x, -1.0 / B, 0.0, 1, n & 1, R=R, shift=(n + 1) % 4)
            for k, o in (('a', 'action'), ('q1', 'q'), ('ga', 'gaction')):
                eq_val(got[k], old[o], ((Dx, A), 'policy_grad', k))
            assert np.isfinite(got['logp']).all()
            L = len(Wm)
            for l in range(L):
                rows = slice(0, A) if l == L - 1 else slice(None)
                eq_val(got['dW'][l][rows], old['dW'][l], ((Dx, A), 'dW', l))
                eq_val(got['db'][l][rows], old['db'][l], ((Dx, A), 'db', l))
            assert not got['dW'][-1][A:].any() and not got['db'][-1][A:].any(), 'the log-std rows are not zero'


# 5. edges
def case_edges(library):
    nan = float('nan')
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B = 6, 3, 33
        c = spg_case(Dx, A, (33,), (33,), (64, 33), True, B)
        x, nets = c['x'], c['nets']
        gscale, lscale, alpha = -1.0 / B, 1.0 / B, 0.2
        e = F32(lscale) * F32(alpha)
        lo, hi = F32(-1.5), F32(0.25)
        # zero last-layer weights: z is the bias in every row; log-std biases at the ends of the clamp, one step beyond each, and NaN
        for ls_bias, inside in (([lo, hi, lo], True), ([np.nextafter(lo, F32(-INF)), np.nextafter(hi, F32(INF)), F32(nan)], False)):
            Ws = c['Ws'][:-1] + [np.zeros_like(c['Ws'][-1])]
            bs = c['bs'][:-1] + [np.concatenate([np.array([0.5, -0.25, 0.0], F32), np.array(ls_bias, F32)])]
            got = device_sac_pg(h, Ws, bs, *nets, x, gscale, lscale, alpha, float(lo), float(hi), seed=3, counter=4)
            z = np.broadcast_to(bs[-1], (B, 2 * A)).copy()
            n = SC.device_sample(h, Ws, bs, x, float(lo), float(hi), 1, 3, 4)['n']
            check_head_grad(got, n, z, e, float(lo), float(hi), ('ends', inside))
            g_ls = got['ghead'][:, A:]
            assert (g_ls != 0).all() if inside else (bits(g_ls) == 0).all(), inside
            w = GC.model(x, Ws, bs, gout=got['ghead'])
            PG.check(got, w, ('ends', inside), ('dW', 'db'))
        # a row driven to |a| == 1: t == 0, g_mu == 2 e a exactly, logp finite
        Ws = c['Ws'][:-1] + [np.zeros_like(c['Ws'][-1])]
        bs = c['bs'][:-1] + [np.array([30.0, -30.0, 0.1, -1.0, -1.0, -1.0], F32)]
        got = device_sac_pg(h, Ws, bs, *nets, x, gscale, lscale, alpha, seed=3, counter=4)
        assert (np.abs(got['a'][:, :2]) == 1).all() and np.isfinite(got['logp']).all()
        eq_val(got['ghead'][:, :2], (F32(2) * e) * got['a'][:, :2], 'g_mu at |a| == 1')
        # critic 2 a copy of critic 1: a tie, every output equals the one-critic call
        kw = dict(seed=5, counter=6, row_offset=7)
        one = device_sac_pg(h, c['Ws'], c['bs'], nets[0], nets[1], None, None, x, gscale, lscale, alpha, **kw)
        tie = device_sac_pg(h, c['Ws'], c['bs'], nets[0], nets[1], nets[0], nets[1], x, gscale, lscale, alpha, shift=1, **kw)
        assert one['q2'] is None
        eq_bits(tie['q2'], tie['q1'], 'the copy')
        for k in ('a', 'logp', 'q1', 'ga', 'ghead'):
            eq_bits(tie[k], one[k], ('tie', k))
        PG.check(tie, one, 'tie', ('dW', 'db'))
        # a critic whose q is NaN on some rows: a LINEAR critic passes the NaN of an input on (behind a hidden layer fmaxf(NaN, 0) = 0 clears it).
        # NaN in q1: q1 <= q2 is false, critic 2 supplies ga; NaN in q2: likewise false, critic 2 supplies ga -- a NaN on either side takes critic 2
        Wl, bl = network(2450, (Dx + A, 1))
        xn = x.copy()
        xn[::3, 0] = nan
        for label, (Wf, bf, Ws_, bs_) in (('NaN q1', (Wl, bl, nets[2], nets[3])), ('NaN q2', (nets[0], nets[1], Wl, bl))):
            with np.errstate(invalid='ignore'):
                got = device_sac_pg(h, c['Ws'], c['bs'], Wf, bf, Ws_, bs_, xn, gscale, lscale, alpha, null=('ghead',), grads=False, **kw)
                ga1 = GC.device_grad(h, Wf, bf, xn, got['a'], 0, gscale=gscale, grads=False, null=('gx',))['ga']
                ga2 = GC.device_grad(h, Ws_, bs_, xn, got['a'], 0, gscale=gscale, grads=False, null=('gx',))['ga']
            qn = got['q1'] if label == 'NaN q1' else got['q2']
            assert np.isnan(qn[::3]).all() and np.isfinite(np.delete(qn, np.s_[::3])).all(), label
            assert np.isfinite(got['q2'] if label == 'NaN q1' else got['q1']).all(), label
            eq_val(got['ga'][::3], ga2[::3], (label, 'NaN rows take critic 2'))
            eq_val(got['ga'], np.where((got['q1'] <= got['q2'])[:, None], ga1, ga2), (label, 'selection'))
        # d_alpha equals alpha
        base = device_sac_pg(h, c['Ws'], c['bs'], *nets, x, gscale, lscale, alpha, **kw)
        dal = device_sac_pg(h, c['Ws'], c['bs'], *nets, x, gscale, lscale, d_alpha=alpha, shift=2, **kw)
        for k in OUTPUTS:
            eq_bits(dal[k], base[k], ('d_alpha', k))
        PG.check(dal, base, 'd_alpha', ('dW', 'db'))


# 6. stale tile, both directions
def stale_forward(regime, between):
    return SC.stale_actor(regime, TILE + 1, between)


def stale_back(regime):
    """Dx = 29, A = 4 (Dx + A = 33): a Gaussian actor 29 -> 33 -> 8 behind critics that leave the tile as large as they can: grad_cases.stale_case's
    critic ('huge', 'inf') as critic 1 and 2 in turn, and the 'gx' regime of policy_grad_cases.back_stale_case: a critic whose layer 0 has 3e38 in
    the column of an input that is 0 in every row, gscale = -100, so that s_0 next to the action columns overflows"""
    def make():
        Dx, A, B = 29, 4, TILE + 1
        Wa, ba = network(2500, (Dx, 33, 2 * A))
        ba[-1][A:] = ba[-1][A:] - F32(1)
        if regime == 'gx':
            W1, b1 = GC.net(2501, (Dx + A, 33, 1))
            W1[0][:, Dx - 1] = 3e38                                   # the input next to the action columns
            W2, b2 = GC.net(2502, (Dx + A, 17, 1))
            W2[0][:, 0] = 3e38
            x = np.random.RandomState(2503).uniform(-2, 2, (B, Dx)).astype(F32)
            x[:, Dx - 1] = 0
            x[:, 0] = 0
            gscale = -100.0
        else:
            s = GC.stale_case(regime, B)
            W1, b1 = s['Ws'], s['bs']
            W2, b2 = network(2504, (Dx + A, 33, 1))
            W2[0] = (W2[0] * (1.0 if regime == 'huge' else 1e-9)).astype(F32)
            x, gscale = s['x'], -1.0 / B
        return {'Ws': Wa, 'bs': ba, 'x': x, 'nets': (W1, b1, W2, b2), 'gscale': gscale, 'z': forward(x, Wa, ba)}
    return TC.cached(('sac pg stale', regime), make)


def check_model(h, got, c, nets, gscale, e, seeds, label, lo=LS_LO, hi=LS_HI, grads=True):
    """every output against the MODEL: a against float64 from the chain model's z, q against the numpy chain on the call's own a, ga against the
    exact backward chains, the head gradient, dW / db against the exact chains from the call's own d_ghead"""
    W1, b1, W2, b2 = nets
    x, B, A = c['x'], c['x'].shape[0], got['a'].shape[1]
    u1, u2 = SC.draws(*seeds, B, A)
    n = SC.n32_of(u1, u2)
    a64, lp64, mag, _, _ = SC.head64(c['z'], n, lo, hi)
    assert np.abs(got['a'] - a64).max() <= SC.SAC_A_TOL + SC.SAC_N_TOL * np.exp(min(hi, 0.5)), (label, 'a')
    assert np.isfinite(got['logp']).all(), (label, 'logp')
    with np.errstate(over='ignore', invalid='ignore'):
        m1 = GC.model(x, W1, b1, gscale=gscale, a=got['a'], weights=False)
        m2 = GC.model(x, W2, b2, gscale=gscale, a=got['a'], weights=False)
    q1, q2 = m1['out'][:, 0], m2['out'][:, 0]
    assert np.isfinite(q1).all() and np.isfinite(q2).all(), label
    eq_bits(got['q1'], q1, (label, 'q1 against the model'))
    eq_bits(got['q2'], q2, (label, 'q2 against the model'))
    ga = np.where((q1 <= q2)[:, None], m1['ga'], m2['ga'])
    eq_val(got['ga'], ga, (label, 'ga against the model'))
    assert np.isfinite(got['ga']).all() and np.isfinite(got['ghead']).all(), (label, 'NaN or inf')
    A_ = got['a'].shape[1]
    g_mu = head_grad(got['a'], got['ga'], e, n, c['z'], lo, hi)[0]
    eq_val(got['ghead'][:, :A_], g_mu, (label, 'g_mu'))
    if grads:
        with np.errstate(over='ignore', invalid='ignore'):
            w = GC.model(x, c['Ws'], c['bs'], gout=got['ghead'])
        assert all(np.isfinite(t).all() for t in got['dW'] + got['db']), (label, 'NaN or inf in dW / db')
        PG.check(got, w, label, ('dW', 'db'))
    return q1, q2


def case_stale_tile(library):
    B = TILE + 1
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        seeds = (3, 4, 5)
        kw = dict(seed=3, counter=4, row_offset=5)
        # forward: the actor's / critic 1's hidden activations of 1e31 / inf under the columns a critic's layer 0 reads (Dx + A = 33 is odd)
        for regime in ('huge', 'inf'):
            for between in ('actor', 'critics'):
                c = stale_forward(regime, between)
                gscale, lscale, alpha = -1.0 / B, 1.0 / B, 0.2
                for null in ((), ('a',)):
                    got = device_sac_pg(h, c['Ws'], c['bs'], *c['nets'], c['x'], gscale, lscale, alpha, grads=False, null=null + ('ga', 'ghead'), pad=1, **kw)
                    with np.errstate(over='ignore', invalid='ignore'):
                        a = got['a'] if got['a'] is not None else whole['a']
                        q1, q2 = q_model(c['x'], a, c['nets'][0], c['nets'][1]), q_model(c['x'], a, c['nets'][2], c['nets'][3])
                    assert np.isfinite(q1).all() and np.isfinite(q2).all() and len(set(q2.tolist())) > B // 2
                    eq_bits(got['q1'], q1, (regime, between, null, 'q1 against the model'))
                    eq_bits(got['q2'], q2, (regime, between, null, 'q2 against the model'))
                    if not null:
                        whole = got
                        a64 = SC.head64(c['z'], SC.n32_of(*SC.draws(*seeds, B, 4)))[0]
                        assert np.abs(got['a'] - a64).max() <= SC.SAC_A_TOL + SC.SAC_N_TOL * np.exp(0.5), (regime, between)
        # backward: the critics' leavings under the columns of the hand-back and of the actor's first transposed chain
        for regime in ('huge', 'inf', 'gx'):
            c = stale_back(regime)
            for swap in (False, True):
                nets = c['nets'] if not swap else c['nets'][2:] + c['nets'][:2]
                for null in ((), ('a',)):
                    got = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'], c['gscale'], 1.0 / B, 0.2, null=null, pad=1, nan_work=True, **kw)
                    if not null:
                        whole = got
                        check_model(h, got, c, nets, c['gscale'], F32(1.0 / B) * F32(0.2), seeds, (regime, swap))
                    else:
                        for k in ('logp', 'q1', 'q2', 'ga', 'ghead'):
                            eq_bits(got[k], whole[k], (regime, swap, 'workspace path', k))
                        PG.check(got, whole, (regime, swap, 'workspace path'), ('dW', 'db'))
                one = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'][TILE:], c['gscale'], 1.0 / B, 0.2, grads=False, seed=3, counter=4, row_offset=5 + TILE)
                for k in OUTPUTS:
                    eq_bits(one[k], whole[k][TILE:], (regime, swap, 'row 32 alone', k))


# 7. properties
def case_properties(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        B = 101
        for Dx, A, ah, h1, h2 in ((6, 3, (33,), (33,), (64, 33)), (1, 20, (), (33,), (64, 33))):
            c = spg_case(Dx, A, ah, h1, h2, True, B)
            nets = c['nets']
            tail = (-1.0 / B, 1.0 / B, 0.2)
            kw = dict(seed=7, counter=8)
            big = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'], *tail, pad=1, shift=1, **kw)
            # a row alone, in a tile of its own and inside its batch
            for lo_, hi_ in ((0, 1), (32, 33), (100, 101), (0, 33), (40, 101)):
                sub = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'][lo_:hi_], *tail, grads=False, shift=2, seed=7, counter=8, row_offset=lo_)
                for k in OUTPUTS:
                    assert np.array_equal(bits(sub[k]), bits(big[k][lo_:hi_])), (k, lo_, 'a row depends on its batch')
            again = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'], *tail, pad=1, shift=1, twice=True, **kw)
            for k in OUTPUTS:
                eq_bits(again[k], big[k], (k, 'two calls differ'))
            for u, v in zip(big['dW'] + big['db'], again['dW'] + again['db']):
                eq_bits(u, v, 'two calls differ in dW / db')
            # a permutation of the rows (without sampling: the draws belong to the place, not to the row)
            mode = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'], *tail, sample=0)
            perm = np.random.RandomState(5).permutation(B)
            xp = np.ascontiguousarray(c['x'][perm])
            rev = device_sac_pg(h, c['Ws'], c['bs'], *nets, xp, *tail, sample=0)
            for k in OUTPUTS:
                assert np.array_equal(bits(rev[k]), bits(mode[k][perm])), (k, 'a row depends on its place')
            PG.check(rev, GC.model(xp, c['Ws'], c['bs'], gout=rev['ghead']), 'permuted', ('dW', 'db'))
            PG.check(mode, GC.model(c['x'], c['Ws'], c['bs'], gout=mode['ghead']), 'in order', ('dW', 'db'))
            assert any(not np.array_equal(bits(u), bits(v)) for u, v in zip(rev['dW'], mode['dW']))
            # chunks: another chain, the model's
            for R in (2, 32, 128):
                ch = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'], *tail, R=R, nan_work=True, **kw)
                for k in OUTPUTS:
                    eq_bits(ch[k], big[k], (k, R))
                w = GCC.chunk_model(c['x'], c['Ws'], c['bs'], R, gout=ch['ghead']) if R < B else GC.model(c['x'], c['Ws'], c['bs'], gout=ch['ghead'])
                PG.check(ch, w, ('chunks', R), ('dW', 'db'))
            # every optional output NULL in turn (and all of them); grads NULL with and without d_ghead / d_gaction
            for null in (('a',), ('logp',), ('q1',), ('q2',), ('ga',), ('ghead',), OUTPUTS):
                got = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'], *tail, null=null, shift=3, **kw)
                for k in OUTPUTS:
                    assert (got[k] is None) == (k in null)
                    if got[k] is not None:
                        eq_bits(got[k], big[k], ('NULL', null, k))
                PG.check(got, big, ('NULL', null), ('dW', 'db'))
            for null in ((), ('ghead',), ('ga', 'ghead'), ('q1', 'q2', 'ga', 'ghead'), ('a', 'ga', 'ghead'), ('a', 'logp', 'q1', 'q2', 'ga'), ('logp', 'q1', 'ga', 'ghead'),
                         ('a', 'q1', 'q2', 'ga', 'ghead')):
                got = device_sac_pg(h, c['Ws'], c['bs'], *nets, c['x'], *tail, grads=False, null=null, pad=2, nan_work=bool(len(null) & 1), **kw)
                assert got['dW'] is None and got['db'] is None
                for k in OUTPUTS:
                    if got[k] is not None:
                        eq_bits(got[k], big[k], ('grads NULL', null, k))


# 8. the temperature
ALPHA_BATCHES = (1, 255, 256, 257, 1000)
ALPHA_LOGS = tuple(np.linspace(-9, 3, 97).astype(np.float32))


def measure_alpha_bar():
    la = np.array(ALPHA_LOGS, F32)
    return float((np.abs(np.exp(la).astype(F64) - np.exp(la.astype(F64))) / np.exp(la.astype(F64))).max())


def alpha_total(logp):
    """the two chains: p_t over the rows b = t (mod 256) ascending from +0.0, then the p_t ascending from +0.0 -> total (float32)"""
    logp = np.asarray(logp, F32)
    part = np.zeros(256, F32)
    for lo in range(0, logp.size, 256):
        blk = logp[lo:lo + 256]
        part[:blk.size] = part[:blk.size] + blk
    total = F32(0)
    for p in part:
        total = F32(total + p)
    return total


def alpha_g(logp, target_entropy):
    return -F32(F32(alpha_total(logp) / F32(len(logp))) + F32(target_entropy))


def device_alpha(h, logp, state, target_entropy, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, shift=0, steps=1):
    """`steps` consecutive pmg_sac_alpha_device calls on canary-framed buffers -> the states after each"""
    B = len(logp)
    out = []
    with Dev(h) as dev:
        d_lp, _ = put_rows(h, dev, np.asarray(logp, F32)[None, :], 0, shift)
        st = Out(dev, 16, 4 * ((shift + 1) & 3))
        h.upload(st.ptr, np.asarray(state, F32))
        for k in range(steps):
            h.sac_alpha_device(h.sac_alpha_struct(B, d_lp, st.ptr, target_entropy, lr, step + k, beta1, beta2, eps))
            out.append(st.read())
    return out


def device_adam_one(h, p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """pmg_mlp_adam_device on a network of one weight -> p, m, v"""
    with Dev(h) as dev:
        ptrs = [dev.put(np.array([[t]], F32)) for t in (p, g, m, v)]
        mlp = h.mlp_struct([1, 1], [ptrs[0]], None, 0)
        ps = [h.params_struct([q]) for q in ptrs]
        h.mlp_adam_device(mlp, ps[0], ps[1], ps[2], ps[3], h.adam_struct(lr, step, beta1, beta2, eps))
        return [dev.get(ptrs[i], 1, F32)[0] for i in (0, 2, 3)]


def case_alpha(library):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, B in enumerate(ALPHA_BATCHES):
            logp = (np.random.RandomState(70 + B).standard_normal(B) * 3 - 2).astype(F32)
            te, lr = -3.0, 3e-2
            g = alpha_g(logp, te)
            # beta1 = 0 (and beta2 = 0): m = g and v = g * g exactly -- the two chains and the quotient, bit for bit
            st = device_alpha(h, logp, [0.5, 9.0, 9.0, 0.0], te, lr, 1, beta1=0.0, beta2=0.0, shift=n % 4)[0]
            eq_bits(st[1:2], np.array([g], F32), (B, 'g (total)'))
            eq_bits(st[2:3], np.array([g * g], F32), (B, 'g * g'))
            # three consecutive steps against pmg_mlp_adam_device on one weight fed the model's g
            state = np.array([np.log(0.2), 0.0, 0.0, 0.2], F32)
            got = device_alpha(h, logp, state, te, lr, 1, shift=(n + 1) % 4, steps=3)
            p, m, v = state[0], state[1], state[2]
            for k, s in enumerate(got):
                p, m, v = device_adam_one(h, p, g, m, v, lr, 1 + k)
                eq_bits(s[:3], np.array([p, m, v], F32), (B, k, 'log_alpha, m, v'))
                err = abs(float(s[3]) - np.exp(float(s[0]))) / np.exp(float(s[0]))
                worst = max(worst, err)
                assert err <= SAC_ALPHA_TOL, (B, k, 'alpha', err)
            assert got[2][0] != state[0]
        # update, then the target reads the new value on the stream: no sync in between
        from pybullet_multigoal_gym_amd.sac import Temperature
        Dx, A, B = 6, 3, 37
        c = spg_case(Dx, A, (33,), (33,), (64, 33), True, B)
        r = np.zeros(B, F32)
        temp = Temperature(env)
        temp.init(0.2)
        assert abs(temp.value() - 0.2) < 1e-7
        with Dev(h) as dev:
            logp = np.full(B, -1.0, F32)
            d_lp = dev.put(logp)
            actor, c1 = Net(h, dev, c['Ws'], c['bs'], 0), Net(h, dev, c['nets'][0], c['nets'][1], 0)
            d_x, d_r, d_y = dev.put(c['x']), dev.put(r), dev.alloc(4 * B)
            d_w = dev.alloc(4 * B * A)
            temp.update_device(d_lp, B, -float(A), 0.05, 1)
            h.sac_target_device(actor.mlp, c1.mlp, None, h.sac_target_struct(B, d_x, Dx, d_r, d_y, 0.98, alpha=0.0, seed=1, counter=2, d_alpha=temp.d_alpha,
                                                                               d_work=d_w, work_floats=B * A))
            y_new = dev.get(d_y, B, F32)
            new = temp.value()
        assert new != F32(0.2)
        want = SC.device_sac_target(h, c['Ws'], c['bs'], c['nets'][0], c['nets'][1], None, None, x=c['x'], r=r, alpha=float(new), seed=1, counter=2)
        eq_bits(y_new, want['y'], 'the target reads the updated temperature')
        temp.close()
    print('alpha = expf(log_alpha) against float64: %.3g (bar %.3g)' % (worst, SAC_ALPHA_TOL))
    return worst


# 9. the faces
def case_host_face(library):
    import pytest
    from pybullet_multigoal_gym_amd.critic import Critic
    from pybullet_multigoal_gym_amd.sac import GaussianActor, Temperature, actor_head_grad
    env = AC.stepped(library, 'reach', 8)
    Dx, A, B = 6, 3, 37
    nets = SC.recipe_nets(Dx, A)
    Wa, ba, W1, b1, W2, b2 = nets
    pi, critic, critic2 = env.gaussian_actor, env.critic, Critic(env)
    x = np.random.RandomState(93).uniform(-2, 2, (B, Dx)).astype(F32)
    with pytest.raises(ValueError):
        pi.policy_grad(x, critic, critic2, 0.2)                  # nothing loaded
    pi.load(Wa, ba)
    critic.load(W1, b1)
    critic2.load(W2, b2)
    alpha = 0.2
    assert pi.policy_grad_work_floats(B, critic2=critic2) == pi.grad_work_floats(B) + 2 * B * A
    assert pi.policy_grad_work_floats(B, action=True) == pi.grad_work_floats(B)
    res = pi.policy_grad(x, critic, critic2, alpha, seed=4, counter=5, row_offset=6)
    # the call-by-call sequence of the old recipe, with actor_head_grad as its reference
    a, logp, n, z = pi.sample(x, seed=4, counter=5, row_offset=6, preact=True)
    eq_bits(res['action'], a, 'a')
    eq_bits(res['logp'], logp, 'logp')
    q1, q2 = critic.q(x, a), critic2.q(x, a)
    eq_bits(res['q1'], q1, 'q1')
    eq_bits(res['q2'], q2, 'q2')
    ga1 = critic.grad(x, a, gscale=-1.0 / B, grads=False)['ga']
    ga2 = critic2.grad(x, a, gscale=-1.0 / B, grads=False)['ga']
    ga = np.where((q1 <= q2)[:, None], ga1, ga2)
    eq_val(res['gaction'], ga, 'ga')
    assert (q1 < q2).any() and (q2 < q1).any()
    old = pi.grad(x, gout=actor_head_grad(a, n, z, ga, alpha))
    err = SC.recipe_error(res['dW'], res['db'], [np.asarray(t, F64) for t in old['dW']], [np.asarray(t, F64) for t in old['db']])
    assert err <= SAC_PG_TOL, ('the fused call against the old recipe', err)
    want_dW, want_db = SC.recipe_autograd64(nets, x, n, alpha)
    err64 = SC.recipe_error(res['dW'], res['db'], want_dW, want_db)
    assert err64 <= SAC_PG_TOL, err64
    new = pi.grad(x, gout=res['ghead'])
    PG.check(res, new, 'dW / db from the own d_ghead', ('dW', 'db'))
    # policy_grad + adam_step_device gives the weights the call-by-call sequence gives
    h = env.handle
    st = pi.adam_state()
    work = pi.policy_grad_work_floats(B, critic2=critic2)
    with Dev(h) as dev:
        d_x, d_work = dev.put(x), dev.alloc(4 * work)
        pi.policy_grad_device(B, d_x, critic, critic2, d_work, work, alpha, grads=st.g, seed=4, counter=5, row_offset=6)
        pi.adam_step_device(st.g, st, 1e-3)
        h.sync()
        fused = pi.parameters()
    pi.load(Wa, ba)
    st = pi.adam_state()
    with Dev(h) as dev:
        d_x, d_work, d_g = dev.put(x), dev.alloc(4 * pi.grad_work_floats(B)), dev.put(res['ghead'])
        pi.grad_device(B, d_x, Dx, d_work, pi.grad_work_floats(B), d_gout=d_g, grads=st.g)
        pi.adam_step_device(st.g, st, 1e-3)
        h.sync()
        stepwise = pi.parameters()
    for u, v in zip(fused[0] + fused[1], stepwise[0] + stepwise[1]):
        eq_val(u, v, 'the weights after Adam')
    assert any(not np.array_equal(u, v) for u, v in zip(fused[0], Wa))
    pi.load(Wa, ba)
    one = pi.policy_grad(x, critic, None, alpha, seed=4, counter=5, row_offset=6, chunk_rows=2)
    assert one['q2'] is None
    eq_bits(one['q1'], q1, 'one critic')
    assert pi.policy_grad(x[:0], critic, critic2, alpha)['action'].shape == (0, A)
    # the temperature
    temp = Temperature(env)
    with pytest.raises(ValueError):
        temp.value()
    for bad in (-1.0, 0.0, float('nan'), INF):
        with pytest.raises(ValueError):
            temp.init(bad)
    temp.init(0.3)
    assert abs(temp.value() - 0.3) < 1e-7 and temp.d_alpha
    with Dev(h) as dev:
        d_lp = dev.put(np.asarray(res['logp'], F32))
        for call in (lambda: temp.update_device(d_lp, 0, -3.0, 1e-3, 1), lambda: temp.update_device(d_lp, B, float('nan'), 1e-3, 1),
                     lambda: temp.update_device(d_lp, B, -3.0, 1e-3, 0), lambda: temp.update_device(None, B, -3.0, 1e-3, 1)):
            with pytest.raises(ValueError):
                call()
        temp.update_device(d_lp, B, -3.0, 1e-2, 1)
        assert temp.value() != F32(0.3)
    # refused arguments
    for call in (lambda: pi.policy_grad(x[:, :-1], critic, critic2, alpha), lambda: pi.policy_grad(x, critic, critic2, -0.1),
                 lambda: pi.policy_grad(x, critic, critic2, alpha, ls_lo=1.0, ls_hi=0.0), lambda: pi.policy_grad(x, critic, critic2, alpha, row_offset=-1),
                 lambda: pi.policy_grad(x, critic, critic2, alpha, chunk_rows=3), lambda: pi.policy_grad(x, pi, critic2, alpha),
                 lambda: pi.policy_grad(x, critic, pi, alpha), lambda: pi.policy_grad(x, critic, critic2, alpha, gscale=INF)):
        with pytest.raises(ValueError):
            call()
    temp.close()
    critic2.close()
    pi.close()
    env.close()
    return err64


def case_invalid_calls(library):
    """one invalid call per item of both validation lists, nothing written"""
    nan = float('nan')
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B = 6, 3, 8
        with Dev(h) as dev:
            actor, c1, c2 = Net(h, dev, *network(81, (Dx, 16, 2 * A))), Net(h, dev, *network(82, (Dx + A, 16, 1))), Net(h, dev, *network(87, (Dx + A, 8, 8, 1)))
            odd, wide, two = Net(h, dev, *network(88, (Dx, 16, 2 * A + 1))), Net(h, dev, *network(83, (Dx + A + 1, 16, 1))), Net(h, dev, *network(84, (Dx + A, 16, 2)))
            nobias = Net(h, dev, network(85, (Dx, 16, 2 * A))[0], None)
            d_x, d_al = dev.put(np.zeros((B, 16), F32)), dev.put(np.full(2, 0.2, F32))
            d_lp, d_st = dev.put(np.zeros(B + 1, F32)), dev.put(np.full(5, SENTINEL * 0 + 0.25, F32))
            size = 4 * B * 2 * A
            outs = [dev.put(np.full(size, SENTINEL, np.uint8)) for _ in range(6)]
            need = h.sac_policy_grad_work_floats(actor.mlp, 1, 1, B, 2)
            wsize = 4 * (need + 2 * B * A)
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

            def bad_nets(net):
                return [mlp(net, **kw) for kw in (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                                  dict(width=(1, 0)), dict(d_weight=(0, None)), dict(out_activation=2), dict(d_weight=(1, net.d_w[1] + 2)))]

            def pg(am=None, m1=None, m2='c2', null_g=False, chunk=0, grads='par', **kw):
                a = dict(batch=B, d_x=d_x, x_stride=Dx, d_work=d_work, work_floats=need + 2 * B * A, gscale=-1.0 / B, lscale=1.0 / B, alpha=0.2, ls_lo=LS_LO, ls_hi=LS_HI,
                         sample=1, seed=1, counter=2, row_offset=3, d_alpha=None, grads=par.struct if grads == 'par' else grads, d_action=outs[0], action_stride=A,
                         d_logp=outs[1], d_q1=outs[2], d_q2=outs[3], d_gaction=outs[4], gaction_stride=A, d_ghead=outs[5], ghead_stride=2 * A)
                size_ = kw.pop('struct_size', None)
                a.update(kw)
                s = h.sac_policy_grad_struct(**a)
                if size_ is not None:
                    s.struct_size = size_
                m2 = mlp(c2) if isinstance(m2, str) else m2
                return h.L.lib.pmg_sac_policy_grad_device(h.h, C.byref(am or mlp(actor)), C.byref(m1 or mlp(c1)), C.byref(m2) if m2 is not None else None,
                                                          None if null_g else C.byref(s), C.c_int64(chunk))

            def al(null_a=False, **kw):
                a = dict(batch=B, d_logp=d_lp, d_state=d_st, target_entropy=-3.0, lr=1e-3, step=1)
                size_ = kw.pop('struct_size', None)
                a.update(kw)
                s = h.sac_alpha_struct(**a)
                if size_ is not None:
                    s.struct_size = size_
                return h.L.lib.pmg_sac_alpha_device(h.h, None if null_a else C.byref(s))
            none = dict(d_action=None, d_logp=None, d_q1=None, d_q2=None, d_gaction=None, d_ghead=None)
            missing_b = h.params_struct(list(par.struct.d_weight)[:2], [par.struct.d_bias[0], None])
            missing_w = h.params_struct([par.struct.d_weight[0], None], list(par.struct.d_bias)[:2])
            off_w = h.params_struct([par.struct.d_weight[0] + 2, par.struct.d_weight[1]], list(par.struct.d_bias)[:2])
            bad = [lambda m=m: pg(am=m) for m in bad_nets(actor)] + [lambda m=m: pg(m1=m) for m in bad_nets(c1)] + [lambda m=m: pg(m2=m) for m in bad_nets(c2)] + [
                # what pmg_sac_target_device rejects in the networks, alpha, d_alpha, the clamp and row_offset
                lambda: pg(am=mlp(odd)), lambda: pg(am=mlp(actor, out_activation=1)), lambda: pg(m1=mlp(wide)), lambda: pg(m1=mlp(two)), lambda: pg(m2=mlp(wide)),
                lambda: pg(m2=mlp(two)), lambda: pg(alpha=-0.1), lambda: pg(alpha=INF), lambda: pg(alpha=nan), lambda: pg(d_alpha=d_al + 2),
                lambda: pg(ls_lo=1.0, ls_hi=0.0), lambda: pg(ls_lo=nan), lambda: pg(ls_hi=nan), lambda: pg(ls_lo=-INF), lambda: pg(ls_hi=INF), lambda: pg(row_offset=-1),
                # what pmg_policy_grad_device rejects in grads, strides, pointers, chunk_rows, d_work and work_floats
                lambda: pg(grads=missing_b), lambda: pg(grads=missing_w), lambda: pg(grads=off_w), lambda: pg(am=mlp(nobias), grads=par.struct),
                lambda: pg(x_stride=Dx - 1), lambda: pg(action_stride=A - 1), lambda: pg(gaction_stride=A - 1), lambda: pg(ghead_stride=2 * A - 1),
                lambda: pg(d_x=None), lambda: pg(d_x=d_x + 2), lambda: pg(d_action=outs[0] + 1), lambda: pg(d_logp=outs[1] + 2), lambda: pg(d_q1=outs[2] + 3),
                lambda: pg(d_q2=outs[3] + 1), lambda: pg(d_gaction=outs[4] + 2), lambda: pg(d_ghead=outs[5] + 3), lambda: pg(d_work=d_work + 1),
                lambda: pg(batch=-1), lambda: pg(chunk=-2), lambda: pg(chunk=1), lambda: pg(chunk=3), lambda: pg(batch=2 * 65535 + 1, chunk=2),
                lambda: pg(d_work=None), lambda: pg(work_floats=h.sac_policy_grad_work_floats(actor.mlp, 1, 1, B, 0) - 1),
                lambda: pg(chunk=2, work_floats=need - 1), lambda: pg(d_action=None, work_floats=h.sac_policy_grad_work_floats(actor.mlp, 0, 1, B, 0) - 1),
                lambda: pg(m2=None, work_floats=h.sac_policy_grad_work_floats(actor.mlp, 1, 0, B, 0) - 1),
                # its own
                lambda: pg(gscale=INF), lambda: pg(gscale=nan), lambda: pg(lscale=-INF), lambda: pg(lscale=nan), lambda: pg(grads=None, **none),
                lambda: pg(m2=None, grads=None, **dict(none, d_q2=outs[3])), lambda: pg(null_g=True), lambda: pg(struct_size=C.sizeof(PmgSacPolicyGrad) - 8),
                # the temperature
                lambda: al(null_a=True), lambda: al(struct_size=C.sizeof(PmgSacAlpha) - 8), lambda: al(batch=0), lambda: al(batch=-1), lambda: al(target_entropy=nan),
                lambda: al(target_entropy=INF), lambda: al(lr=nan), lambda: al(lr=INF), lambda: al(eps=-1e-8), lambda: al(eps=nan), lambda: al(beta1=1.0),
                lambda: al(beta1=-0.1), lambda: al(beta2=1.0), lambda: al(beta2=nan), lambda: al(step=0), lambda: al(d_logp=None), lambda: al(d_state=None),
                lambda: al(d_logp=d_lp + 2), lambda: al(d_state=d_st + 1)]
            g0 = h.sac_policy_grad_struct(B, d_x, Dx, d_work, need, -1.0 / B, 1.0 / B, 0.2, d_logp=outs[1])
            assert h.L.lib.pmg_sac_policy_grad_device(h.h, None, C.byref(mlp(c1)), None, C.byref(g0), C.c_int64(0)) == E_INVALID
            assert h.L.lib.pmg_sac_policy_grad_device(h.h, C.byref(mlp(actor)), None, None, C.byref(g0), C.c_int64(0)) == E_INVALID

            def untouched():
                h.sync()
                for o in outs:
                    assert (dev.get(o, size, np.uint8) == SENTINEL).all()
                assert (dev.get(d_work, wsize, np.uint8) == SENTINEL).all()
                par.read(written=False)
                assert (dev.get(d_st, 5, F32) == F32(0.25)).all()
            for k, call in enumerate(bad):
                assert call() == E_INVALID, k
                assert h.L.error(h.h), k
            untouched()
            assert pg(batch=0) == 0 and pg(batch=0, chunk=2) == 0 and pg(batch=0, grads=None) == 0
            untouched()
            # the workspace figure
            base = h.mlp_grad_work_floats(actor.mlp, B)
            assert h.sac_policy_grad_work_floats(actor.mlp, 1, 0, B, 0) == base and h.sac_policy_grad_work_floats(actor.mlp, 0, 0, B, 0) == base + B * A
            assert h.sac_policy_grad_work_floats(actor.mlp, 0, 1, B, 0) == base + 2 * B * A
            assert h.sac_policy_grad_work_floats(actor.mlp, 1, 1, B, 2) == h.mlp_grad_chunked_work_floats(actor.mlp, B, 2) + B * A
            assert h.sac_policy_grad_work_floats(actor.mlp, 1, 1, -1, 0) < 0 and h.sac_policy_grad_work_floats(mlp(odd), 1, 1, B, 0) < 0
            assert h.sac_policy_grad_work_floats(actor.mlp, 1, 1, B, 3) < 0 and h.sac_policy_grad_work_floats(mlp(actor, num_layers=0), 1, 1, B, 0) < 0
            # what is allowed
            assert pg() == 0 and pg(chunk=2) == 0 and pg(m2=None, d_q2=None) == 0 and pg(d_alpha=d_al + 4, alpha=0.0, row_offset=2 ** 40) == 0
            assert pg(grads=None, **dict(none, d_logp=outs[1])) == 0 and pg(am=mlp(nobias), grads=par_nb.struct) == 0 and pg(lscale=0.0, sample=0) == 0
            assert al() == 0 and al(batch=1, step=2 ** 40) == 0
            h.sync()


# 10. what tests/test_sac_pg_wave_order.py runs under every wavefront order
def wave_order_run(library):
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        shapes = {'wide': (3, 12, (256, 256, 256), (256,), (33, 255), 33), 'far': (1, 20, (33,), (64,), (), 32), 'small': (6, 3, (33,), (33,), (33,), 33)}
        for name, (Dx, A, ah, h1, h2, B) in shapes.items():
            c = spg_case(Dx, A, ah, h1, h2, True, B)
            for tag, null, R in (('', (), None), ('w', ('a',), None), ('c', (), 2)):
                got = device_sac_pg(h, c['Ws'], c['bs'], *c['nets'], c['x'], -1.0 / B, 1.0 / B, 0.2, seed=3, counter=4, row_offset=5, pad=1, shift=1, null=null, R=R)
                for k in OUTPUTS:
                    if got[k] is not None:
                        res[name + tag + k] = got[k]
                for l, (w, b) in enumerate(zip(got['dW'], got['db'])):
                    res['%s%sdW%d' % (name, tag, l)], res['%s%sdb%d' % (name, tag, l)] = w, b
    return res
