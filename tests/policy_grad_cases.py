"""The cases of the policy-gradient tests (include/pmg.h pmg_policy_grad_device) and their numpy model, shared by
tests/test_policy_grad_emulated.py (the g++ build of the product sources over the fiber emulator), tests/test_gpu_policy_grad.py
(libpmg_hip.so on the MI355X), tests/test_policy_grad_host.py (the numpy faces, and the model against torch.autograd) and
tests/test_policy_grad_wave_order.py.  The model is put together from the pieces the earlier tests stand on: actor_cases' exact float32 fmaf
and forward chain, grad_cases' model of a network's backward, grad_chunk_cases' chunked sums.

Bars.  The fused call is DEFINED as a sequence of existing calls (pmg_mlp_forward_device -> clip on the host -> pmg_mlp_grad_device of the
critic with the constant head, input gradients only -> the L2 / clip head on the host with an exact fmaf -> pmg_mlp_grad[_chunked]_device of
the actor from d_gout), so every output is compared bit for bit with that sequence run on the same library (GC.eq_val: zeros by value), and
with the numpy model.  A tanh output goes through the library's tanhf: the model then starts from the call's own out / q, held to the float64
tanh of the model's bit-exact z within actor_cases.ACTION_TOL, as grad_cases and td_cases do."""
import ctypes as C

import numpy as np

import actor_cases as AC
import grad_cases as GC
import grad_chunk_cases as GCC
import td_cases as TC
from actor_cases import ACTION_TOL, Net, fmaf
from grad_cases import Params, eq_val, read_rows, rows_out
from normalizer_cases import SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PmgMlp, PmgPolicyGrad
from td_cases import Out, cached, put_rows

E_INVALID = -1
TILE = AC.TILE
F32 = np.float32
INF = float('inf')
BATCHES = GC.BATCHES
# (Dx, A): the flagship; the smallest; A > Dx in one pass of 8 units; A > Dx in two passes; Dx + A = 33, odd
PAIRS = ((6, 3), (1, 1), (2, 5), (3, 12), (29, 4))
# (the actor's hidden widths, the critic's): L = 1 and L = 4 on both sides
HIDDEN = (((), (33,)), ((33,), ()), ((256, 256, 256), (33,)), ((33,), (256, 256, 256)), ((256, 256, 256), (256, 256, 256)))
OUTPUTS = ('action', 'out', 'q', 'gaction')


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def fclip(o):
    """fminf(fmaxf(o, -1), 1): td_cases.clip1 where o is a number; a NaN o becomes -1, as fmaxf returns its other operand"""
    return np.fmin(np.fmax(np.asarray(o, F32), F32(-1)), F32(1))


def head(o, ga, l2scale):
    """step 4: g = fmaf(l2scale, o, inside ? ga : +0.0) -> g, inside"""
    inside = (o >= F32(-1)) & (o <= F32(1))
    with np.errstate(over='ignore', invalid='ignore'):
        return fmaf(np.full(o.shape, l2scale, F32), o, np.where(inside, ga, F32(0))).reshape(o.shape), inside


def pg_model(x, Wa, ba, Wc, bc, gscale, l2scale=0.0, act_a=0, act_c=0, out=None, q=None, grads=True, R=None):
    """steps 1-5 -> dict(out, action, q, gaction, g, inside, dW, db, masks_a, masks_c).  out / q: the call's own o and q where that network
    has a tanh output (None: numpy's float32 tanh)."""
    with np.errstate(over='ignore', invalid='ignore'):
        z = AC.forward(x, Wa, ba)
        o = z if not act_a else (np.tanh(z).astype(F32) if out is None else np.asarray(out, F32))
        a = fclip(o)
        if not np.isnan(o).any():
            assert np.array_equal(a, TC.clip1(o))
        mc = GC.model(x, Wc, bc, act_c, gscale=gscale, out=None if q is None else np.asarray(q, F32)[:, None], a=a, weights=False)
        g, inside = head(o, mc['ga'], l2scale)
        res = {'z': z, 'out': o, 'action': a, 'q': np.ascontiguousarray(mc['out'][:, 0]), 'zc': mc['z'], 'gaction': mc['ga'], 'g': g, 'inside': inside,
               'dW': None, 'db': None, 'masks_c': mc['masks']}
        if grads:
            ma = GC.model(x, Wa, ba, act_a, gout=g, out=o) if R is None or R >= x.shape[0] else GCC.chunk_model(x, Wa, ba, R, act_a, gout=g, out=o)
            res.update(dW=ma['dW'], db=ma['db'], masks_a=ma['masks'])
    return res


def check(got, want, label, keys=('dW', 'db') + OUTPUTS):
    for k in keys:
        if k in ('dW', 'db'):
            if got[k] is None:
                continue
            for l, (g, w) in enumerate(zip(got[k], want[k])):
                assert (g is None) == (w is None), (label, k, l)
                if g is not None:
                    eq_val(g, w, (label, k, l))
        elif got.get(k) is not None:
            eq_val(got[k], want[k], (label, k))


# ----------------------------------------------------------------------------------------------------------------------
# device calls
def device_policy_grad(h, Wa, ba, Wc, bc, x, gscale, l2scale=0.0, act_a=0, act_c=0, grads=True, null=(), pad=0, shift=0, R=None, twice=False,
                       nan_work=False):
    """pmg_policy_grad_device on canary-framed, sentinel-filled outputs -> dict(dW, db, action, out, q, gaction) (None for what was passed as
    NULL).  pad: floats of poison behind every input row and of sentinel between output rows; shift: the phase of the first float pointer,
    the others follow in turn; the workspace is sized exactly and, with grads NULL, must come back untouched."""
    B, A = x.shape[0], Wa[-1].shape[0]
    with Dev(h) as dev:
        actor, critic = Net(h, dev, Wa, ba, act_a), Net(h, dev, Wc, bc, act_c)
        d_x, xs = put_rows(h, dev, x, pad, shift)
        outs = {'action': rows_out(dev, B, A, pad, (shift + 1) & 3), 'out': rows_out(dev, B, A, pad, (shift + 2) & 3),
                'q': Out(dev, 4 * B, 4 * ((shift + 3) & 3)), 'gaction': rows_out(dev, B, A, pad, shift & 3)}
        par = Params(h, dev, Wa, ba, shift)
        work = h.policy_grad_work_floats(actor.mlp, critic.mlp, B, R or 0)
        assert work >= h.mlp_grad_work_floats(actor.mlp, B) >= 0
        assert work == (h.mlp_grad_chunked_work_floats(actor.mlp, B, R) if R else h.mlp_grad_work_floats(actor.mlp, B))
        o_work = Out(dev, 4 * work, 4 * ((shift + 1) & 3))
        if nan_work and work:
            h.upload(o_work.ptr, np.full(work, 0x7FC00000 | 0x1234, np.uint32))
        ptr = lambda k: None if k in null else outs[k].ptr
        g = h.policy_grad_struct(B, d_x, xs, o_work.ptr, work, gscale, l2scale, par.struct if grads else None, ptr('action'), A + pad, ptr('out'), A + pad,
                                 ptr('q'), ptr('gaction'), A + pad)
        for _ in range(2 if twice else 1):
            h.policy_grad_device(actor.mlp, critic.mlp, g, R or 0)
        h.sync()
        o_work.read(np.uint8, written=bool(grads) or nan_work)
        dW, db = par.read(written=grads)
        res = {'dW': dW, 'db': db}
        for k in ('action', 'out', 'gaction'):
            res[k] = read_rows(outs[k], B, A, pad, k not in null)
        res['q'] = outs['q'].read(written='q' not in null)
        for net in (actor, critic):                                # neither network's weights are written
            for p, W in zip(net.d_w, (Wa if net is actor else Wc)):
                assert np.array_equal(AC.bits(dev.get(p, W.shape, F32)), AC.bits(W)), 'a weight was written'
        return res


def device_sequence(h, Wa, ba, Wc, bc, x, gscale, l2scale=0.0, act_a=0, act_c=0, grads=True, R=None, out=None):
    """the sequence of existing calls the fused call is defined by -> the same dict.  out: start from this o in place of the forward's own."""
    o = AC.device_forward(h, Wa, ba, x, act_a) if out is None else np.asarray(out, F32)
    a = fclip(o)
    with np.errstate(over='ignore', invalid='ignore'):
        c = GC.device_grad(h, Wc, bc, x, a, act_c, gscale=gscale, grads=False, null=('gx',))
        g, _ = head(o, c['ga'], l2scale)
    res = {'dW': None, 'db': None, 'action': a, 'out': o, 'q': np.ascontiguousarray(c['out'][:, 0]), 'gaction': c['ga']}
    if grads:
        p = GC.device_grad(h, Wa, ba, x, None, act_a, gout=g, null=('gx',)) if R is None else GCC.device_grad_chunked(h, Wa, ba, x, R, None, act_a, gout=g, null=('gx',))
        eq_val(p['out'], o, 'the actor gradient call starts from another o than the forward call gave')
        res.update(dW=p['dW'], db=p['db'])
    return res


# ----------------------------------------------------------------------------------------------------------------------
# 1. the model is the gradient (CPU only: tests/test_policy_grad_host.py)
MODEL_NETS = (((6, 256, 256, 256, 3), 1, (256, 256, 256)), ((5, 33, 4), 0, (33,)))
MODEL_SEEDS = (1, 2)
MODEL_B = 33


def scaled_actor(seed, widths, out_act, bias=True):
    """grad_cases.net; an identity actor's last layer is scaled so that roughly half its outputs leave [-1, 1]"""
    Wa, ba = GC.net(seed, widths, bias)
    if not out_act:
        Wa[-1] = (Wa[-1] * 4).astype(F32)
        if ba is not None:
            ba[-1] = (ba[-1] * 4).astype(F32)
    return Wa, ba


def model_vs_autograd(widths, out_act, critic_hidden, B, seed):
    """-> (largest max|g32 - g64| / max|g64| over the actor's dW, db and over gaction and q, masks and clip predicates equal, the share of
    outputs outside [-1, 1]) against float64 autograd of gscale * sum Q(x, clamp(pi(x), -1, 1)) + l2scale / 2 * sum pi(x)^2"""
    import torch
    Dx, A = widths[0], widths[-1]
    Wa, ba = scaled_actor(seed, widths, out_act)
    Wc, bc = GC.net(seed + 50, (Dx + A,) + tuple(critic_hidden) + (1,))
    rs = np.random.RandomState(seed + 77)
    x = rs.uniform(-1, 1, (B, Dx)).astype(F32)
    gscale, l2scale = -1.0 / B, 2.0 / (B * A)
    m = pg_model(x, Wa, ba, Wc, bc, gscale, l2scale, out_act, 0)
    dt = torch.float64
    tW, tb = [torch.tensor(W, dtype=dt, requires_grad=True) for W in Wa], [torch.tensor(b, dtype=dt, requires_grad=True) for b in ba]
    cW, cb = [torch.tensor(W, dtype=dt) for W in Wc], [torch.tensor(b, dtype=dt) for b in bc]
    tx = torch.tensor(x, dtype=dt)

    def mlp(h, Ws, bs, masks):
        for l in range(len(Ws)):
            z = h @ Ws[l].T + bs[l]
            if l + 1 < len(Ws):
                masks.append((z > 0).detach().numpy())
                h = torch.relu(z)
        return z
    masks_a, masks_c = [], []
    z = mlp(tx, tW, tb, masks_a)
    o = torch.tanh(z) if out_act else z
    a = torch.clamp(o, -1.0, 1.0)
    a.retain_grad()
    q = mlp(torch.cat([tx, a], 1), cW, cb, masks_c)
    (float(F32(gscale)) * q.sum() + float(F32(l2scale)) / 2 * (o * o).sum()).backward()
    inside64 = ((o >= -1) & (o <= 1)).detach().numpy()
    same = all(np.array_equal(u, v) for u, v in zip(m['masks_a'] + m['masks_c'], masks_a + masks_c)) and np.array_equal(m['inside'], inside64)
    pairs = list(zip(m['dW'] + m['db'] + [m['gaction'], m['q']], [t.grad.numpy() for t in tW + tb] + [a.grad.numpy(), q.detach().numpy()[:, 0]]))
    worst = max(float(np.abs(np.asarray(u, np.float64) - v).max() / np.abs(v).max()) for u, v in pairs)
    return worst, same, float(1.0 - m['inside'].mean())


# ----------------------------------------------------------------------------------------------------------------------
# 2. bit-equal to the sequence of existing calls
def pg_case(Dx, A, ah, ch, B, bias=True, act_a=0, act_c=0, seed=None):
    """an actor Dx -> ah -> A and a critic Dx + A -> ch -> 1 on B rows (no model: the sequence of device calls is the reference)"""
    def make():
        s = seed if seed is not None else 2000 + 31 * Dx + 7 * A + len(ah) + 3 * len(ch)
        Wa, ba = scaled_actor(s, (Dx,) + tuple(ah) + (A,), act_a, bias)
        Wc, bc = GC.net(s + 1, (Dx + A,) + tuple(ch) + (1,), bias)
        x = np.random.RandomState(s + B).uniform(-2, 2, (B, Dx)).astype(F32)
        return dict(Wa=Wa, ba=ba, Wc=Wc, bc=bc, x=x, act_a=act_a, act_c=act_c)
    return cached(('pg', Dx, A, tuple(ah), tuple(ch), B, bias, act_a, act_c, seed), make)


def run_both(h, c, gscale, l2scale, n=0, R=None, model=False, **kw):
    """the fused call against the sequence of existing calls on the same library (and, asked for, against the numpy model) -> the fused result"""
    args = (c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], gscale, l2scale, c['act_a'], c['act_c'])
    got = device_policy_grad(h, *args, pad=n % 3, shift=n % 4, R=R, **kw)
    grads = kw.get('grads', True)
    check(got, device_sequence(h, *args, grads=grads, R=R), ('the sequence', n))
    if model:
        check(got, pg_model(c['x'], *args[:4], *args[5:], out=got['out'], q=got['q'], grads=grads, R=R), ('the model', n))
    return got


def case_bit_exact(library, hidden):
    """every pair (Dx, A) on one choice of hidden widths, the batches, biases, l2scale and the two output activations in turn"""
    ah, ch = hidden
    big = len(ah) + len(ch) > 2
    clipped = total = 0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A) in enumerate(PAIRS):
            k = n + HIDDEN.index(hidden)
            B = BATCHES[k % (4 if big else 5)]                    # (the largest networks take the batches up to 33: the emulator's cost is B)
            c = pg_case(Dx, A, ah, ch, B, bias=k % 3 != 2, act_a=k % 2, act_c=(k // 2) % 2)
            l2scale = 0.0 if n % 2 else 2.0 / (B * A)
            got = run_both(h, c, -1.0 / B, l2scale, k, model=not big)
            clipped += int((np.abs(got['out']) > 1).sum())
            total += got['out'].size
    assert big or clipped > 0, 'no output of an identity actor left [-1, 1]: the clip was never active'
    return clipped, total


def case_chunks(library):
    """chunk_rows None, 2 and 32 at B = 101, against the chunked sequence and the chunked model"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A, ah, ch) in enumerate(((6, 3, (33,), (33,)), (3, 12, (33,), ()), (29, 4, (), (33,)))):
            c = pg_case(Dx, A, ah, ch, 101, bias=n != 1)
            for R in (None, 2, 32):
                run_both(h, c, -1.0 / 101, 2.0 / (101 * A), n + 1, R=R, model=R != 2, nan_work=R == 32)
            # one chunk is the single chain: the same bits
            one = device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], -1.0 / 101, R=102)
            check(one, device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], -1.0 / 101), 'R >= B')


def case_every_batch(library):
    """every batch size on the flagship shape with small hidden layers, tanh actor, against sequence and model"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, B in enumerate(BATCHES):
            c = pg_case(6, 3, (33,), (33,), B, act_a=1)
            run_both(h, c, -1.0 / B, 2.0 / (B * 3), n, model=True)


def case_tanh(library):
    """o of a tanh actor and q of a tanh critic against the float64 tanh of the model's bit-exact z"""
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A, ah, ch) in enumerate(((6, 3, (33,), (33,)), (2, 5, (256, 256, 256), (33,)), (29, 4, (), ()))):
            c = pg_case(Dx, A, ah, ch, 33, act_a=1, act_c=1)
            got = device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], -1.0 / 33, 0.01, 1, 1, shift=n)
            m = pg_model(c['x'], c['Wa'], c['ba'], c['Wc'], c['bc'], -1.0 / 33, 0.01, 1, 1, out=got['out'], q=got['q'])
            err = max(float(np.abs(got['out'] - np.tanh(m['z'].astype(np.float64))).max()), float(np.abs(got['q'] - np.tanh(m['zc'].astype(np.float64))[:, 0]).max()))
            worst = max(worst, err)
            assert err <= ACTION_TOL, (Dx, A, err)
            check(got, m, ('tanh', n))
    print('tanh outputs: largest |o - tanh64(z)|, |q - tanh64(z_c)| = %.3g (bar %.3g)' % (worst, ACTION_TOL))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# 3. clip edges
def case_clip_edges(library):
    one, up, down = F32(1), np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(-2))
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        B, Dx, A = 33, 3, 4
        Wc, bc = GC.net(301, (Dx + A, 33, 1))
        x = np.random.RandomState(302).uniform(-2, 2, (B, Dx)).astype(F32)
        # an identity actor with zero weights and biases exactly 1, -1, the next float above 1 and the next below -1
        Wa, ba = [np.zeros((A, Dx), F32)], [np.array([one, -one, up, down], F32)]
        for l2scale in (0.0, 0.25):
            got = device_policy_grad(h, Wa, ba, Wc, bc, x, -1.0 / B, l2scale)
            check(got, device_sequence(h, Wa, ba, Wc, bc, x, -1.0 / B, l2scale), ('edges', l2scale))
            check(got, pg_model(x, Wa, ba, Wc, bc, -1.0 / B, l2scale), ('edges: model', l2scale))
            assert np.array_equal(got['out'], np.broadcast_to(ba[0], (B, A))) and np.array_equal(got['action'], np.broadcast_to(np.array([1, -1, 1, -1], F32), (B, A)))
            ga = got['gaction']
            assert (ga != 0).all(), 'the critic passes no gradient: the case shows nothing'
            # db of the only layer is the sum of g over the rows in ascending order: ga passes at exactly +-1 and is +0.0 beyond, the L2 term
            # l2scale * o is there on both sides
            want = np.zeros(A, F32)
            for b in range(B):
                g = fmaf(np.full(A, l2scale, F32), ba[0], np.where(np.array([True, True, False, False]), ga[b], F32(0)))
                want = (want + g).astype(F32)
            eq_val(got['db'][0], want, ('edges: db', l2scale))
            assert (got['db'][0][:2] != 0).all()
            if l2scale == 0.0:
                assert np.array_equal(AC.bits(got['db'][0][2:] + F32(0)), AC.bits(np.zeros(2, F32))), 'a gradient passed the clip beyond +-1'
            else:
                assert got['db'][0][2] > 0 and got['db'][0][3] < 0, 'the L2 term is missing beyond the clip'
        # a tanh actor driven to o == 1.0f: the delta factor fmaf(-o, o, 1) is exactly 0, whatever g is
        Wa, ba = [np.zeros((A, Dx), F32)], [np.array([20, 20, -20, 0.5], F32)]
        got = device_policy_grad(h, Wa, ba, Wc, bc, x, -1.0 / B, 0.25, act_a=1)
        assert (got['out'][:, :2] == 1).all() and (got['out'][:, 2] == -1).all() and (np.abs(got['out'][:, 3]) < 1).all()
        check(got, device_sequence(h, Wa, ba, Wc, bc, x, -1.0 / B, 0.25, act_a=1), 'tanh at 1')
        assert (got['db'][0][:3] == 0).all() and got['db'][0][3] != 0 and (got['dW'][0][:3] == 0).all()
        # o = NaN (a NaN bias of unit 1), input only: a = fminf(fmaxf(NaN, -1), 1) = -1, q and ga are those of that action
        Wa, ba = GC.net(303, (Dx, 33, A))
        ba[1][1] = np.nan
        got = device_policy_grad(h, Wa, ba, Wc, bc, x, -1.0 / B, 0.25, grads=False)
        m = pg_model(x, Wa, ba, Wc, bc, -1.0 / B, 0.25, grads=False)
        assert np.isnan(got['out'][:, 1]).all() and (got['action'][:, 1] == -1).all() and np.isfinite(got['q']).all() and np.isfinite(got['gaction']).all()
        check(got, m, 'NaN o', ('action', 'q', 'gaction'))
        assert not m['inside'][:, 1].any() and np.isnan(m['g'][:, 1]).all()       # the model: +0.0 branch, and l2scale * NaN is NaN either way
        eq_val(np.delete(got['out'], 1, 1), np.delete(m['out'], 1, 1), 'NaN o: the other outputs')


# ----------------------------------------------------------------------------------------------------------------------
# 4. stale tile, both directions
def back_stale_case(regime, B):
    """Dx = 30, A = 3 (Dx + A = 33, A odd): an actor 30 -> 33 -> 3 whose first transposed chain reads delta_1 in columns 0..2 and the padding
    column 3 of the tile, behind a critic that leaves those columns as large as it can.
      'huge', 'inf': grad_cases.stale_case's critics (33 -> 256 -> 3 -> 1 with hidden activations of 1e31, 33 -> 256 -> 33 -> 1 with inf), on
              x = the first 30 columns of its rows.  'inf' is asked for the outputs alone (grads NULL), as there.
      'gx':   a critic 33 -> 33 -> 1 whose layer 0 has 3e38 in column 3 -- the weights of input x[3], which is 0 in every row, so the forward
              does not see them -- and gscale = -100: s_0[.][3], which the critic's layer 0 leaves in column 3 of the tile, overflows.  Only the
              hand-back's +0.0 in column A = 3 keeps 0 * inf = NaN out of the actor's delta_0, dW_0 and db_0."""
    def make():
        Dx, A = 30, 3
        Wa, ba = scaled_actor(401, (Dx, 33, A), 0)
        if regime == 'gx':
            Wc, bc = GC.net(402, (Dx + A, 33, 1))
            Wc[0][:, A] = 3e38
            x = np.random.RandomState(403 + B).uniform(-2, 2, (B, Dx)).astype(F32)
            x[:, A] = 0
            gscale = -100.0
        else:
            c = GC.stale_case(regime, B)
            Wc, bc, gscale = c['Ws'], c['bs'], -1.0 / B
            x = np.ascontiguousarray(np.concatenate([c['x'], c['a']], 1)[:, :Dx])
        with np.errstate(over='ignore', invalid='ignore'):
            m = pg_model(x, Wa, ba, Wc, bc, gscale, 0.01, grads=regime != 'inf')
            s0 = GC.model(x, Wc, bc, gscale=gscale, a=m['action'], weights=False)['gx']
            hid = np.maximum(AC.forward(np.concatenate([x, m['action']], 1), Wc[:1], None), 0)
        if regime == 'gx':
            assert not np.isfinite(s0[:, A]).any(), 'column A of the tile would be finite: the case shows nothing'
        else:
            assert np.isinf(hid).all() if regime == 'inf' else (np.isfinite(hid).all() and hid.min() > 1e30)
        for k in OUTPUTS:
            assert np.isfinite(m[k]).all(), (regime, k)
        if m['dW'] is not None:
            assert all(np.isfinite(t).all() for t in m['dW'] + m['db']) and np.abs(m['dW'][0]).max() > 0
        return dict(Wa=Wa, ba=ba, Wc=Wc, bc=bc, x=x, gscale=gscale, m=m)
    return cached(('pg stale', regime, B), make)


def case_stale_tile(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        # forward: td_cases' two regimes, the actor's hidden activations of 1e31 / inf under the critic's input and padding columns
        for regime in ('huge', 'inf'):
            for B in (TILE, TILE + 1):
                c = TC.stale_case(regime, B)
                got = device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], -1.0 / B, 0.01, grads=False, pad=1)
                for k in OUTPUTS:
                    assert np.isfinite(got[k]).all(), (regime, B, k, 'NaN or inf')
                with np.errstate(over='ignore', invalid='ignore'):
                    m = pg_model(c['x'], c['Wa'], c['ba'], c['Wc'], c['bc'], -1.0 / B, 0.01, grads=False)
                eq_val(m['q'], c['q'], 'the model is not td_cases')
                check(got, m, ('forward', regime, B))
        # backward: the critic's leavings under the columns the actor's first transposed chain reads, A odd
        for regime in ('huge', 'inf', 'gx'):
            for B in (TILE, TILE + 1):
                c = back_stale_case(regime, B)
                got = device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], c['gscale'], 0.01, grads=regime != 'inf', pad=1)
                for k in OUTPUTS:
                    assert np.isfinite(got[k]).all(), (regime, B, k, 'NaN or inf')
                if got['dW'] is not None:
                    assert all(np.isfinite(t).all() for t in got['dW'] + got['db']), (regime, B, 'NaN or inf in dW / db')
                check(got, c['m'], ('backward', regime, B))


# ----------------------------------------------------------------------------------------------------------------------
# 5. independence
def case_independence(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        B = 101
        c = pg_case(6, 3, (33,), (33,), B, act_a=1)
        args = (c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], -1.0 / B, 2.0 / (B * 3), 1, 0)
        big = device_policy_grad(h, *args, pad=1, shift=1)
        # a row alone and in its batch (row 100 sits in a tile with 27 rows past the batch)
        for lo, hi in ((0, 1), (32, 33), (100, 101), (0, 33)):
            sub = device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'][lo:hi], *args[5:], grads=False, shift=2)
            for k in OUTPUTS:
                assert np.array_equal(AC.bits(sub[k]), AC.bits(big[k][lo:hi])), (k, lo, 'a row depends on its batch')
        again = device_policy_grad(h, *args, pad=1, shift=1, twice=True)
        for k in OUTPUTS:
            assert np.array_equal(AC.bits(again[k]), AC.bits(big[k])), (k, 'two calls differ')
        for u, v in zip(big['dW'] + big['db'], again['dW'] + again['db']):
            assert np.array_equal(AC.bits(u), AC.bits(v)), 'two calls differ in dW / db'
        # a permutation of the rows: the rows' outputs move with them, dW / db become the model's of the permuted batch -- another chain
        perm = np.random.RandomState(5).permutation(B)
        xp = np.ascontiguousarray(c['x'][perm])
        rev = device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], xp, *args[5:])
        for k in OUTPUTS:
            assert np.array_equal(AC.bits(rev[k]), AC.bits(big[k][perm])), (k, 'a row depends on its place')
        check(rev, pg_model(xp, c['Wa'], c['ba'], c['Wc'], c['bc'], *args[5:], out=rev['out']), 'permuted', ('dW', 'db'))
        check(big, pg_model(c['x'], c['Wa'], c['ba'], c['Wc'], c['bc'], *args[5:], out=big['out']), 'in order', ('dW', 'db'))
        assert any(not np.array_equal(AC.bits(u), AC.bits(v)) for u, v in zip(rev['dW'], big['dW']))
        # every optional output NULL in turn (and all of them): the others' bits stay; grads NULL: the workspace is not touched
        for null in (('action',), ('out',), ('q',), ('gaction',), OUTPUTS):
            got = device_policy_grad(h, *args, null=null, shift=3)
            check(got, big, ('NULL', null))
            assert all(got[k] is None for k in null)
        for null in ((), ('q',), ('gaction',), ('q', 'gaction'), ('action', 'out', 'gaction'), ('action', 'out', 'q')):
            got = device_policy_grad(h, *args, grads=False, null=null, pad=2)       # (device_policy_grad requires the workspace untouched)
            assert got['dW'] is None and got['db'] is None
            check(got, big, ('grads NULL', null))


def wave_order_run(library):
    """what tests/test_policy_grad_wave_order.py runs under every wavefront order -> dict of arrays"""
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        shapes = {'small': (6, 3, (33,), (33,), 33, 1), 'wide': (3, 12, (256, 256), (256,), 33, 0), 'odd': (29, 4, (255, 31), (33, 255), 32, 0), 'flat': (2, 5, (), (), 31, 0)}
        for name, (Dx, A, ah, ch, B, act) in shapes.items():
            c = pg_case(Dx, A, ah, ch, B, act_a=act)
            got = device_policy_grad(h, c['Wa'], c['ba'], c['Wc'], c['bc'], c['x'], -1.0 / B, 2.0 / (B * A), act, 0, pad=1, shift=1)
            for k in OUTPUTS:
                res[name + k] = got[k]
            for l, (w, b) in enumerate(zip(got['dW'], got['db'])):
                res['%sdW%d' % (name, l)], res['%sdb%d' % (name, l)] = w, b
    return res


# ----------------------------------------------------------------------------------------------------------------------
# 6. through the faces
def case_through_the_faces(library):
    """Actor.policy_grad and adam_step_device against the three calls it replaces, l2scale = 0 and a tanh actor (the clip is never active)"""
    import pytest
    from pybullet_multigoal_gym_amd.actor import Actor
    from pybullet_multigoal_gym_amd.critic import Critic
    Dx, A, B, lr = 6, 3, 33, 1e-3
    env = AC.stepped(library, 'reach', 8)
    actor, critic, old = env.actor, env.critic, Actor(env)
    Wa, ba = GC.net(811, (Dx, 33, A))
    Wc, bc = GC.net(812, (Dx + A, 33, 1))
    for net in (actor, old):
        net.load(Wa, ba, out_activation='tanh')
    critic.load(Wc, bc)
    x = np.random.RandomState(813).uniform(-2, 2, (B, Dx)).astype(F32)
    # the old way
    a_pi = old.forward(x)
    gq = critic.grad(x, a_pi, grads=None, gscale=-1.0 / B)
    go = old.grad(x, gout=gq['ga'])
    so = old.adam_state()
    old.adam_step_device(go, so, lr)
    # the one call
    for R in (None, 16):
        got = actor.policy_grad(critic, x, -1.0 / B, chunk_rows=R)
        eq_val(got['out'], a_pi, 'out')
        eq_val(got['action'], a_pi, 'action')
        eq_val(got['gaction'], gq['ga'], 'gaction')
        eq_val(got['q'], gq['out'][:, 0], 'q')
        if R is None:
            GC.check(got, go, 'policy_grad against the three calls', ('dW', 'db'))
    got = actor.policy_grad(critic, x, -1.0 / B)
    sa = actor.adam_state()
    actor.adam_step_device(got, sa, lr)
    for u, v in zip(sum(actor.parameters(), []), sum(old.parameters(), [])):
        assert np.array_equal(u, v), 'the weights after Adam differ from the three-call sequence'
    assert any(not np.array_equal(u, w) for u, w in zip(actor.parameters()[0], Wa))
    # the L2 term and the device form: grads into the state's buffer, nothing downloaded
    h = env.handle
    with Dev(h) as dev:
        d_x = dev.put(x)
        work = actor.policy_grad_work_floats(critic, B, 16)
        assert work == actor.grad_work_floats(B, 16) and actor.policy_grad_work_floats(critic, B) == actor.grad_work_floats(B)
        d_work = dev.alloc(4 * work)
        actor.policy_grad_device(critic, B, d_x, d_work, work, -1.0 / B, 2.0 / (B * A), grads=sa.g, chunk_rows=16)
        dW, db = sa.g.download()
    W1, b1 = actor.parameters()
    m = pg_model(x, W1, b1, Wc, bc, -1.0 / B, 2.0 / (B * A), 1, 0, out=actor.forward(x), R=16)
    GC.check({'dW': dW, 'db': db}, m, 'policy_grad_device into AdamState.g', ('dW', 'db'))
    without = actor.policy_grad(critic, x, -1.0 / B, chunk_rows=16)
    assert any(not np.array_equal(u, v) for u, v in zip(dW, without['dW'])), 'l2scale changes nothing'
    out_only = actor.policy_grad(critic, x, -1.0 / B, grads=False)
    assert out_only['dW'] is None and out_only['db'] is None
    eq_val(out_only['gaction'], without['gaction'], 'grads=False')
    empty = actor.policy_grad(critic, x[:0], -1.0)
    assert empty['action'].shape == (0, A) and empty['q'].shape == (0,) and empty['dW'][0].shape == (33, Dx)
    # the faces refuse what does not fit
    wrong = Critic(env)
    wrong.load(*GC.net(814, (Dx + A + 1, 33, 1)))
    for bad in (lambda: actor.policy_grad(wrong, x, -1.0), lambda: actor.policy_grad(old, x, -1.0), lambda: actor.policy_grad(critic, x[:, :5], -1.0),
                lambda: actor.policy_grad(critic, x, INF), lambda: actor.policy_grad(critic, x, -1.0, float('nan')), lambda: actor.policy_grad(critic, x, -1.0, chunk_rows=3),
                lambda: actor.policy_grad(critic, x[0], -1.0), lambda: actor.policy_grad_work_floats(wrong, B), lambda: actor.policy_grad_work_floats(critic, B, 1)):
        with pytest.raises(ValueError):
            bad()
    wrong.close()
    old.close()
    env.close()


# ----------------------------------------------------------------------------------------------------------------------
# 7. invalid calls
def case_invalid_calls(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B = 6, 3, 8
        Wa, ba = GC.net(91, (Dx, 16, A))
        Wn, _ = GC.net(92, (Dx, 16, A), bias=False)
        Wc, bc = GC.net(93, (Dx + A, 16, 1))
        W2, b2 = GC.net(94, (Dx + A, 16, 2))
        W3, b3 = GC.net(95, (Dx + A + 1, 16, 1))
        nan = float('nan')
        with Dev(h) as dev:
            actor, nobias, critic, two, wide = Net(h, dev, Wa, ba, 0), Net(h, dev, Wn, None, 0), Net(h, dev, Wc, bc, 0), Net(h, dev, W2, b2, 0), Net(h, dev, W3, b3, 0)
            d_x = dev.put(np.zeros((B, Dx), F32))
            NB = 4096
            outs = [dev.put(np.full(NB, SENTINEL, np.uint8)) for _ in range(9)]      # action, out, q, gaction, work, dW0, db0, dW1, db1
            work = h.policy_grad_work_floats(actor.mlp, critic.mlp, B, 0)
            work2 = h.policy_grad_work_floats(actor.mlp, critic.mlp, B, 2)
            assert 0 < work < work2 and 4 * work2 <= NB and work == h.mlp_grad_work_floats(actor.mlp, B) and work2 == h.mlp_grad_chunked_work_floats(actor.mlp, B, 2)

            def mlp(n, **kw):
                m = h.mlp_struct(n.widths, n.d_w, n.d_b, 0)
                for k, v in kw.items():
                    if k in ('width', 'd_weight', 'd_bias'):
                        getattr(m, k)[v[0]] = v[1]
                    else:
                        setattr(m, k, v)
                return m

            def params(**kw):
                p = h.params_struct([outs[5], outs[7]], [outs[6], outs[8]])
                for k, v in kw.items():
                    getattr(p, k)[v[0]] = v[1]
                return p
            par = params()

            def call(a=None, c=None, null_g=False, R=0, **kw):
                args = dict(batch=B, d_x=d_x, x_stride=Dx, d_work=outs[4], work_floats=work2, gscale=-0.125, l2scale=0.01, grads=par, d_action=outs[0],
                            action_stride=A, d_out=outs[1], out_stride=A, d_q=outs[2], d_gaction=outs[3], gaction_stride=A)
                size = kw.pop('struct_size', None)
                args.update(kw)
                s = h.policy_grad_struct(**args)
                if size is not None:
                    s.struct_size = size
                return h.L.lib.pmg_policy_grad_device(h.h, C.byref(a or mlp(actor)), C.byref(c or mlp(critic)), None if null_g else C.byref(s), C.c_int64(R))
            bad_kw = (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)), dict(width=(1, 0)),
                      dict(d_weight=(0, None)), dict(out_activation=2))
            bad = [lambda kw=kw: call(a=mlp(actor, **kw)) for kw in bad_kw] + [lambda kw=kw: call(c=mlp(critic, **kw)) for kw in bad_kw] + [
                lambda: call(a=mlp(actor, d_weight=(1, actor.d_w[1] + 2))), lambda: call(c=mlp(critic, d_bias=(0, critic.d_b[0] + 1))),
                lambda: call(c=mlp(wide)), lambda: call(c=mlp(two)),                                   # critic.width[0] != Dx + A; critic.width[L] != 1
                lambda: call(gscale=nan), lambda: call(gscale=INF), lambda: call(l2scale=nan), lambda: call(l2scale=-INF),
                lambda: call(grads=None, d_action=None, d_out=None, d_q=None, d_gaction=None),
                lambda: call(grads=params(d_weight=(1, None))), lambda: call(grads=params(d_bias=(0, None))),
                lambda: call(a=mlp(nobias)),                                                           # a bias gradient where the actor has no bias
                lambda: call(d_work=None), lambda: call(work_floats=work - 1), lambda: call(work_floats=0), lambda: call(work_floats=work2 - 1, R=2),
                lambda: call(grads=None, d_work=None), lambda: call(grads=None, work_floats=work - 1),
                lambda: call(d_x=None), lambda: call(d_x=d_x + 2), lambda: call(d_action=outs[0] + 1), lambda: call(d_out=outs[1] + 2), lambda: call(d_q=outs[2] + 3),
                lambda: call(d_gaction=outs[3] + 1), lambda: call(d_work=outs[4] + 2), lambda: call(grads=params(d_weight=(0, outs[5] + 2))),
                lambda: call(grads=params(d_bias=(1, outs[8] + 1))),
                lambda: call(x_stride=Dx - 1), lambda: call(action_stride=A - 1), lambda: call(out_stride=0), lambda: call(gaction_stride=A - 1),
                lambda: call(batch=-1), lambda: call(R=-2), lambda: call(R=1), lambda: call(R=3),
                lambda: call(batch=2 * 65535 + 1, R=2, work_floats=1 << 40),                           # more than PMG_GRAD_MAX_CHUNKS chunks
                lambda: call(null_g=True), lambda: call(struct_size=C.sizeof(PmgPolicyGrad) - 8), lambda: call(struct_size=0)]
            g0 = h.policy_grad_struct(B, d_x, Dx, outs[4], work2, -0.125, d_q=outs[2])
            assert h.L.lib.pmg_policy_grad_device(h.h, None, C.byref(mlp(critic)), C.byref(g0), C.c_int64(0)) == E_INVALID
            assert h.L.lib.pmg_policy_grad_device(h.h, C.byref(mlp(actor)), None, C.byref(g0), C.c_int64(0)) == E_INVALID
            wf = h.policy_grad_work_floats
            assert wf(actor.mlp, critic.mlp, -1) < 0 and wf(actor.mlp, mlp(wide), B) < 0 and wf(actor.mlp, mlp(two), B) < 0 and wf(mlp(actor, num_layers=5), critic.mlp, B) < 0
            assert wf(actor.mlp, critic.mlp, B, 1) < 0 and wf(actor.mlp, critic.mlp, B, 3) < 0 and wf(actor.mlp, critic.mlp, B, -2) < 0 and wf(actor.mlp, critic.mlp, 2 * 65535 + 1, 2) < 0
            assert h.L.lib.pmg_policy_grad_work_floats(None, C.byref(critic.mlp), C.c_int64(B), C.c_int64(0)) < 0
            assert h.L.lib.pmg_policy_grad_work_floats(C.byref(actor.mlp), None, C.c_int64(B), C.c_int64(0)) < 0
            assert wf(actor.mlp, critic.mlp, 0) == 0

            def untouched():
                h.sync()
                for o in outs:
                    assert (dev.get(o, NB, np.uint8) == SENTINEL).all()
            for k, f in enumerate(bad):
                assert f() == E_INVALID, k
                assert h.L.error(h.h), k
            untouched()
            assert call(batch=0) == 0 and call(batch=0, work_floats=0) == 0 and call(batch=0, R=2) == 0          # a no-op that leaves grads untouched
            untouched()
            # what is allowed: a network without biases whose grads carry none, the outputs alone, one output alone, chunks
            p_nb = params()
            p_nb.d_bias[0] = p_nb.d_bias[1] = None
            assert call(a=mlp(nobias), grads=p_nb) == 0 and call(grads=None) == 0 and call(grads=None, d_action=None, d_out=None, d_gaction=None) == 0
            assert call(R=2) == 0 and call(R=8, work_floats=work) == 0 and call(d_action=None, d_out=None, d_q=None, d_gaction=None) == 0
            h.sync()
