"""The cases of the behaviour-cloning policy-gradient tests (include/pmg.h pmg_policy_grad_bc_device) and their numpy model,
shared by tests/test_policy_grad_bc_emulated.py (the g++ build of the product sources over the fiber emulator),
tests/test_gpu_policy_grad_bc.py (libpmg_hip.so on the MI355X), tests/test_policy_grad_bc_host.py (the numpy faces, and the model against
torch.autograd) and tests/test_policy_grad_bc_wave_order.py.  The model is policy_grad_cases.pg_model for steps 1-3, actor_cases.forward for
qd, the head below, and grad_cases' / grad_chunk_cases' model of the actor's backward.

Bars.  The fused call is DEFINED as a sequence of existing calls (pmg_mlp_forward_device -> clip on the host -> pmg_q_device on x | ad ->
pmg_mlp_grad_device of the critic, input gradients only -> f and g on the host with an exact fmaf -> pmg_mlp_grad[_chunked]_device of the
actor from d_gout), so every output is compared bit for bit with that sequence on the same library (GC.eq_val: zeros by value) and with
the numpy model.  A tanh output goes through the library's tanhf: the model then starts from the call's own out / q / q_demo, each held to
the float64 tanh of the model's bit-exact z within actor_cases.ACTION_TOL.

Demonstration actions are uniform in [-1, 1].  Rows below demo_begin are uploaded as NaN: a kernel that reads them shows.  Every case with
at least MIN_SIDE rows on both sides of demo_begin asserts on the MODEL that some demonstration rows pass the Q-filter and some do not, and
that a row below demo_begin would pass it (a kernel that ignores demo_begin fails); the demonstrations' seed is the first for which the
model says so (a property of the data, decided before any device runs).  With fewer rows -- B = 1 -- the property cannot hold and the
case checks the bits alone."""
import ctypes as C

import numpy as np

import actor_cases as AC
import grad_cases as GC
import grad_chunk_cases as GCC
import policy_grad_cases as PC
import td_cases as TC
from actor_cases import ACTION_TOL, Net, fmaf
from grad_cases import Params, eq_val, read_rows, rows_out
from normalizer_cases import SENTINEL, Dev, handle
from policy_grad_cases import OUTPUTS, PAIRS, fclip, pg_case, pg_model
from pybullet_multigoal_gym_amd._lib import PmgMlp, PmgPolicyBc, PmgPolicyGrad
from td_cases import Out, cached, put_rows

E_INVALID = -1
TILE = AC.TILE
F32 = np.float32
INF = float('inf')
BATCHES = GC.BATCHES
HIDDEN = (((), (33,)), ((33,), ()), ((256, 256, 256), (256, 256, 256)))
ALL = OUTPUTS + ('q_demo', 'filter')
MIN_SIDE = 8                 # rows on each side of demo_begin from which the filter's property is asserted: 2 * 0.6^8 < 4 % per seed tried
DEMO_BEGINS = (0, 1, 31, 32, 33, 64, 100, 101)

# The model against float64 autograd (tests/test_policy_grad_bc_host.py): max|g32 - g64| / max|g64| over the actor's dW and db, gaction, q and
# q_demo, on MODEL_NETS x MODEL_SEEDS at B = 33 with demo_begin = 11, both q_filter settings, with equal masks, clip predicates and filters,
# measured on the CPU (grad_cases' convention: the bar is 4 x the largest; a MEASURED value above 1e-5 would mean the model is wrong):
#   6-256-256-256-3 tanh: 8.18e-7      5-33-4: 2.02e-7      (the largest: 8.18e-7; the filter passed 32 ... 59 % of the demonstration rows)
MODEL_WORST = 8.18e-7
assert MODEL_WORST < 1e-5
MODEL_TOL = 4 * MODEL_WORST
MODEL_DEMO_BEGIN = 11


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def bc_head(o, ad, g4, f, bcscale):
    """step 4: g = f ? fmaf(bcscale, o - ad, g4) : g4, the difference rounded once"""
    with np.errstate(over='ignore', invalid='ignore'):
        e = (np.asarray(o, F32) - np.asarray(ad, F32)).astype(F32)
        return np.where(np.asarray(f, bool)[:, None], fmaf(np.full(o.shape, bcscale, F32), e, g4).reshape(o.shape), g4).astype(F32)


def filter_of(q, qd, demo_begin, q_filter):
    """step 2c: a float32 >, false with a NaN on either side"""
    with np.errstate(invalid='ignore'):
        return (np.arange(len(q)) >= demo_begin) & ((not q_filter) | (np.asarray(qd, F32) > np.asarray(q, F32)))


def bc_model(x, ad, demo_begin, Wa, ba, Wc, bc, gscale, bcscale, l2scale=0.0, q_filter=1, act_a=0, act_c=0, out=None, q=None, q_demo=None, grads=True, R=None):
    """steps 1-5 -> pg_model's dict (its g / dW / db with the cloning term) plus q_demo (ALL rows: what the filter would see), zd, filter, g4.
    out / q / q_demo: the call's own values where that network has a tanh output (q_demo: rows below demo_begin are taken from numpy's tanh)."""
    with np.errstate(over='ignore', invalid='ignore'):
        m = pg_model(x, Wa, ba, Wc, bc, gscale, l2scale, act_a, act_c, out=out, q=q, grads=False)
        zd = AC.forward(np.concatenate([x, ad], 1), Wc, bc)[:, 0]
        qd = zd
        if act_c:
            qd = np.tanh(zd).astype(F32)
            if q_demo is not None:
                qd[demo_begin:] = np.asarray(q_demo, F32)[demo_begin:]
        f = filter_of(m['q'], qd, demo_begin, q_filter)
        g = bc_head(m['out'], ad, m['g'], f, bcscale)
        m.update(q_demo=qd, zd=zd, filter=f, g4=m['g'], g=g)
        if grads:
            o = m['out']
            ma = GC.model(x, Wa, ba, act_a, gout=g, out=o) if R is None or R >= x.shape[0] else GCC.chunk_model(x, Wa, ba, R, act_a, gout=g, out=o)
            m.update(dW=ma['dW'], db=ma['db'], masks_a=ma['masks'])
    return m


def check(got, want, label, keys=('dW', 'db') + ALL):
    PC.check(got, want, label, tuple(k for k in keys if k not in ('q_demo', 'filter')))
    if 'q_demo' in keys and got.get('q_demo') is not None:
        b = got['demo_begin']
        eq_val(got['q_demo'][b:], np.asarray(want['q_demo'], F32)[b:], (label, 'q_demo'))
    if 'filter' in keys and got.get('filter') is not None:
        assert np.array_equal(got['filter'], np.asarray(want['filter']).astype(np.uint8)), (label, 'filter', got['filter'], want['filter'])


# ----------------------------------------------------------------------------------------------------------------------
# cases
def bc_case(Dx, A, ah, ch, B, demo_begin, bias=True, act_a=0, act_c=0, seed=None):
    """policy_grad_cases.pg_case with demonstration actions uniform in [-1, 1] for every row (the model looks below demo_begin too)"""
    def make():
        c = dict(pg_case(Dx, A, ah, ch, B, bias, act_a, act_c, seed))
        need = demo_begin >= MIN_SIDE and B - demo_begin >= MIN_SIDE
        for s in range(3000 + 17 * Dx + A + B, 3000 + 17 * Dx + A + B + 64):
            ad = np.random.RandomState(s).uniform(-1, 1, (B, A)).astype(F32)
            if not need:
                break
            with np.errstate(over='ignore', invalid='ignore'):
                m = bc_model(c['x'], ad, demo_begin, c['Wa'], c['ba'], c['Wc'], c['bc'], -1.0 / B, 1.0, act_a=act_a, act_c=act_c, grads=False)
                above = m['q_demo'] > m['q']
            if above[demo_begin:].any() and not above[demo_begin:].all() and above[:demo_begin].any():
                break
        else:
            raise AssertionError('no demonstrations with a mixed filter in 64 seeds', Dx, A, ah, ch, B, demo_begin)
        c.update(ad=ad, demo_begin=demo_begin, mixed=need)
        return c
    return cached(('bc', Dx, A, tuple(ah), tuple(ch), B, demo_begin, bias, act_a, act_c, seed), make)


# ----------------------------------------------------------------------------------------------------------------------
# device calls
def device_bc(h, c, gscale, bcscale, l2scale=0.0, q_filter=1, grads=True, null=(), pad=0, shift=0, R=None, twice=False, nan_work=False, demo_begin=None,
              ad=None, x=None, null_ad=False, plain=False):
    """pmg_policy_grad_bc_device on canary-framed, sentinel-filled outputs -> dict(dW, db, action, out, q, gaction, q_demo, filter, demo_begin)
    (None for what was passed as NULL).  pad, shift, the workspace: as policy_grad_cases.device_policy_grad; d_demo_action sits at the phase
    behind d_x's, its rows below demo_begin are NaN; d_filter sits at an odd address; d_q_demo must keep its sentinel below demo_begin.
    plain: pmg_policy_grad_device on the same buffers instead."""
    x = c['x'] if x is None else x
    ad = c['ad'] if ad is None else ad
    b0 = c['demo_begin'] if demo_begin is None else demo_begin
    Wa, ba, Wc, bc = c['Wa'], c['ba'], c['Wc'], c['bc']
    B, A = x.shape[0], Wa[-1].shape[0]
    with Dev(h) as dev:
        actor, critic = Net(h, dev, Wa, ba, c['act_a']), Net(h, dev, Wc, bc, c['act_c'])
        d_x, xs = put_rows(h, dev, x, pad, shift)
        up = np.array(ad, F32)
        up[:b0] = np.nan
        d_ad, ads = (None, 0) if null_ad else put_rows(h, dev, up, pad, (shift + 1) & 3)
        outs = {'action': rows_out(dev, B, A, pad, (shift + 1) & 3), 'out': rows_out(dev, B, A, pad, (shift + 2) & 3),
                'q': Out(dev, 4 * B, 4 * ((shift + 3) & 3)), 'gaction': rows_out(dev, B, A, pad, shift & 3),
                'q_demo': Out(dev, 4 * B, 4 * ((shift + 2) & 3)), 'filter': Out(dev, B, 1 + 2 * (shift & 1))}
        par = Params(h, dev, Wa, ba, shift)
        work = h.policy_grad_work_floats(actor.mlp, critic.mlp, B, R or 0)
        o_work = Out(dev, 4 * work, 4 * ((shift + 1) & 3))
        if nan_work and work:
            h.upload(o_work.ptr, np.full(work, 0x7FC00000 | 0x1234, np.uint32))
        ptr = lambda k: None if k in null else outs[k].ptr
        g = h.policy_grad_struct(B, d_x, xs, o_work.ptr, work, gscale, l2scale, par.struct if grads else None, ptr('action'), A + pad, ptr('out'), A + pad,
                                 ptr('q'), ptr('gaction'), A + pad)
        s = h.policy_bc_struct(b0, d_ad, ads, bcscale, q_filter, ptr('q_demo'), ptr('filter'))
        for _ in range(2 if twice else 1):
            if plain:
                h.policy_grad_device(actor.mlp, critic.mlp, g, R or 0)
            else:
                h.policy_grad_bc_device(actor.mlp, critic.mlp, g, s, R or 0)
        h.sync()
        o_work.read(np.uint8, written=bool(grads) or nan_work)
        dW, db = par.read(written=grads)
        res = {'dW': dW, 'db': db, 'demo_begin': b0}
        for k in ('action', 'out', 'gaction'):
            res[k] = read_rows(outs[k], B, A, pad, k not in null)
        res['q'] = outs['q'].read(written='q' not in null)
        if 'q_demo' in null or plain or b0 == B:
            outs['q_demo'].read(written=False)
            res['q_demo'] = None if 'q_demo' in null or plain else np.full(B, np.nan, F32)
        else:
            raw = outs['q_demo'].read(np.uint8)
            assert (raw[:4 * b0] == SENTINEL).all(), 'd_q_demo was written below demo_begin'
            res['q_demo'] = raw.view(F32).copy()
        res['filter'] = outs['filter'].read(np.uint8, written=not ('filter' in null or plain))
        for net in (actor, critic):                                # neither network's weights are written
            for p, W in zip(net.d_w, (Wa if net is actor else Wc)):
                assert np.array_equal(AC.bits(dev.get(p, W.shape, F32)), AC.bits(W)), 'a weight was written'
        return res


def device_sequence(h, c, gscale, bcscale, l2scale=0.0, q_filter=1, grads=True, R=None, demo_begin=None):
    """the sequence of existing calls the fused call is defined by -> the same dict"""
    x, ad, Wa, ba, Wc, bc, act_a, act_c = (c[k] for k in ('x', 'ad', 'Wa', 'ba', 'Wc', 'bc', 'act_a', 'act_c'))
    b0 = c['demo_begin'] if demo_begin is None else demo_begin
    B = x.shape[0]
    o = AC.device_forward(h, Wa, ba, x, act_a)
    a = fclip(o)
    qd = np.full(B, np.nan, F32)
    if b0 < B:        # pmg_q_device takes an identity critic; pmg_mlp_forward_device on the joined rows is the same chain with the tanh
        qd[b0:] = TC.device_q(h, Wc, bc, x[b0:], ad[b0:]) if not act_c else AC.device_forward(h, Wc, bc, np.concatenate([x[b0:], ad[b0:]], 1), 1)[:, 0]
    with np.errstate(over='ignore', invalid='ignore'):
        cr = GC.device_grad(h, Wc, bc, x, a, act_c, gscale=gscale, grads=False, null=('gx',))
        q = np.ascontiguousarray(cr['out'][:, 0])
        g4, _ = PC.head(o, cr['ga'], l2scale)
        f = filter_of(q, qd, b0, q_filter)
        g = bc_head(o, np.where(np.arange(B)[:, None] >= b0, ad, F32(0)), g4, f, bcscale)
    res = {'dW': None, 'db': None, 'action': a, 'out': o, 'q': q, 'gaction': cr['ga'], 'q_demo': qd, 'filter': f}
    if grads:
        p = GC.device_grad(h, Wa, ba, x, None, act_a, gout=g, null=('gx',)) if R is None else GCC.device_grad_chunked(h, Wa, ba, x, R, None, act_a, gout=g, null=('gx',))
        eq_val(p['out'], o, 'the actor gradient call starts from another o than the forward call gave')
        res.update(dW=p['dW'], db=p['db'])
    return res


def model_of(c, got, gscale, bcscale, l2scale=0.0, q_filter=1, grads=True, R=None, demo_begin=None):
    """the numpy model, started from the call's own tanh outputs"""
    b0 = c['demo_begin'] if demo_begin is None else demo_begin
    return bc_model(c['x'], c['ad'], b0, c['Wa'], c['ba'], c['Wc'], c['bc'], gscale, bcscale, l2scale, q_filter, c['act_a'], c['act_c'], out=got['out'],
                    q=got['q'], q_demo=got['q_demo'], grads=grads, R=R)


def assert_mixed(c, m):
    """on the model: demonstration rows on both sides of the filter, and a row below demo_begin the filter would pass"""
    if c['mixed']:
        b0 = c['demo_begin']
        above = m['q_demo'] > m['q']
        assert above[b0:].any() and not above[b0:].all(), 'every demonstration row falls on one side of the filter: the case shows nothing'
        assert above[:b0].any(), 'no row below demo_begin has qd > q: a kernel that ignores demo_begin would pass'


def run_both(h, c, gscale, bcscale, l2scale, q_filter, n=0, R=None, model=True, **kw):
    """the fused call against the sequence of existing calls on the same library and, asked for, against the numpy model -> the fused result"""
    got = device_bc(h, c, gscale, bcscale, l2scale, q_filter, pad=n % 3, shift=n % 4, R=R, **kw)
    grads = kw.get('grads', True)
    check(got, device_sequence(h, c, gscale, bcscale, l2scale, q_filter, grads=grads, R=R), ('the sequence', n))
    m = model_of(c, got, gscale, bcscale, l2scale, q_filter, grads=grads and model, R=R)
    assert_mixed(c, m)
    check(got, m, ('the model', n), ('dW', 'db') + ALL if model else ALL)
    return got


# ----------------------------------------------------------------------------------------------------------------------
# 1. bit-equal to the sequence and to the model
def case_bit_exact(library, hidden):
    """every pair (Dx, A) on one choice of hidden widths; batches, biases, l2scale, q_filter, both output activations, strides and phases in turn"""
    ah, ch = hidden
    big = len(ah) + len(ch) > 2
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A) in enumerate(PAIRS):
            k = n + HIDDEN.index(hidden)
            B = BATCHES[(k + 1) % (4 if big else 5)]              # (the largest networks take the batches up to 33: the emulator's cost is B)
            b0 = {1: 0, 31: 13, 32: 16, 33: 20, 101: 45}[B]
            c = bc_case(Dx, A, ah, ch, B, b0, bias=k % 3 != 2, act_a=k % 2, act_c=(k // 2) % 2)
            run_both(h, c, -1.0 / B, 2.0 * 0.0078, 0.0 if n % 2 else 2.0 / (B * A), (n + k // 3) % 2, k, model=not big)


def case_every_switch(library):
    """l2scale zero / non-zero x q_filter 0 / 1 x the two activations of both networks x biases, on the flagship pair at B = 33"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        n = 0
        for act_a in (0, 1):
            for act_c in (0, 1):
                c = bc_case(6, 3, (33,), (33,), 33, 14, bias=(act_a + act_c) != 1, act_a=act_a, act_c=act_c)
                for l2scale in (0.0, 0.02):
                    for q_filter in (0, 1):
                        run_both(h, c, -1.0 / 33, 0.0156, l2scale, q_filter, n)
                        n += 1


def case_chunks(library):
    """chunk rows None, 2 and 32 at B = 101, against the chunked sequence and the chunked model"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A, ah, ch) in enumerate(((6, 3, (33,), (33,)), (3, 12, (33,), ()), (29, 4, (), (33,)))):
            c = bc_case(Dx, A, ah, ch, 101, 45 + n, bias=n != 1)
            for R in (None, 2, 32):
                run_both(h, c, -1.0 / 101, 0.0156, 2.0 / (101 * A), 1, n + 1, R=R, model=R != 2, nan_work=R == 32)


def case_tanh(library):
    """out, q and q_demo of tanh networks against the float64 tanh of the model's bit-exact z"""
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A, ah, ch) in enumerate(((6, 3, (33,), (33,)), (29, 4, (), ()))):
            c = bc_case(Dx, A, ah, ch, 33, 12, act_a=1, act_c=1)
            got = device_bc(h, c, -1.0 / 33, 0.0156, 0.01, 1, shift=n)
            m = model_of(c, got, -1.0 / 33, 0.0156, 0.01, 1)
            err = max(float(np.abs(got['out'] - np.tanh(m['z'].astype(np.float64))).max()), float(np.abs(got['q'] - np.tanh(m['zc'].astype(np.float64))[:, 0]).max()),
                      float(np.abs(got['q_demo'][12:] - np.tanh(m['zd'].astype(np.float64))[12:]).max()))
            worst = max(worst, err)
            assert err <= ACTION_TOL, (Dx, A, err)
            check(got, m, ('tanh', n))
    print('tanh outputs: largest |o - tanh64(z)|, |q - tanh64(z_c)|, |q_demo - tanh64(z_d)| = %.3g (bar %.3g)' % (worst, ACTION_TOL))


# ----------------------------------------------------------------------------------------------------------------------
# 2. demo_begin against the tile
def case_demo_begin(library):
    B = 101
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        c = bc_case(6, 3, (33,), (33,), B, 45)
        args = (-1.0 / B, 0.0156, 2.0 / (B * 3))
        plain = device_bc(h, c, *args, plain=True, pad=1, shift=1)
        cloned = 0
        for n, b0 in enumerate(DEMO_BEGINS):
            got = device_bc(h, c, *args, q_filter=n % 2, demo_begin=b0, pad=n % 3, shift=n % 4)     # (device_bc: q_demo keeps its sentinel below b0)
            assert got['filter'].shape == (B,) and not got['filter'][:b0].any()
            check(got, device_sequence(h, c, *args, q_filter=n % 2, demo_begin=b0), ('demo_begin: the sequence', b0))
            check(got, model_of(c, got, *args, q_filter=n % 2, demo_begin=b0), ('demo_begin: the model', b0))
            cloned += int(got['filter'].sum())
            if b0 == B:
                check(got, plain, 'demo_begin = B: pmg_policy_grad_device', ('dW', 'db') + OUTPUTS)
                assert not got['filter'].any()
                none = device_bc(h, c, *args, demo_begin=B, null_ad=True, pad=1, shift=1)
                check(none, plain, 'demo_begin = B, d_demo_action NULL', ('dW', 'db') + OUTPUTS)
            elif b0 < B - 1:
                assert any(not np.array_equal(AC.bits(u), AC.bits(v)) for u, v in zip(got['dW'], plain['dW'])), (b0, 'the cloning term changes nothing')
        assert cloned > 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. the equal case
def case_equal(library):
    """demonstrations equal to the action a first call returned: q_demo has the bits of q, so under the filter nothing is cloned"""
    B = 33
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (Dx, A, act_a) in enumerate(((6, 3, 0), (29, 4, 1), (3, 12, 0))):
            c = dict(bc_case(Dx, A, (33,), (33,), B, 0, act_a=act_a))
            args = (-1.0 / B, 0.0156, 2.0 / (B * A))
            first = device_bc(h, c, *args, plain=True)
            c['ad'] = first['action']
            with np.errstate(over='ignore', invalid='ignore'):         # on the model Q(x, clip(o)) as a row of its own has the bits of q
                m = bc_model(c['x'], c['ad'], 0, c['Wa'], c['ba'], c['Wc'], c['bc'], *args, act_a=act_a, out=first['out'])
            assert np.array_equal(AC.bits(m['q_demo']), AC.bits(m['q']))
            got = device_bc(h, c, *args, q_filter=1, shift=n)
            assert np.array_equal(AC.bits(got['q_demo']), AC.bits(got['q'])), 'Q(x, a) of the demonstration pass differs from q'
            assert not got['filter'].any()
            check(got, first, 'equal, filtered: pmg_policy_grad_device', ('dW', 'db') + OUTPUTS)
            got0 = device_bc(h, c, *args, q_filter=0, shift=n)
            assert got0['filter'].all()
            check(got0, model_of(c, got0, *args, q_filter=0), 'equal, unfiltered')
            if not act_a:                                              # (a tanh actor never leaves [-1, 1]: o - clip(o) is 0 everywhere)
                assert any(not np.array_equal(AC.bits(u), AC.bits(v)) for u, v in zip(got0['dW'], first['dW']))


# ----------------------------------------------------------------------------------------------------------------------
# 4. pure cloning equals the MSE head
def case_pure_cloning(library):
    B = 33
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, act_a in enumerate((0, 1)):
            c = bc_case(6, 3, (33,), (33,), B, 0, act_a=act_a)
            got = device_bc(h, c, 0.0, 2.0 / B, 0.0, 0, shift=n)
            assert got['filter'].all()
            mse = GC.device_grad(h, c['Wa'], c['ba'], c['x'], None, act_a, target=c['ad'], gscale=2.0 / B, null=('gx',))
            GC.check(got, mse, ('pure cloning against the MSE head', act_a), ('dW', 'db', 'out'))
            assert np.abs(got['dW'][0]).max() > 0


# ----------------------------------------------------------------------------------------------------------------------
# 5. NaN
def case_nan(library):
    """a NaN demonstration action (a NaN qd) and a NaN q (a NaN x) give filter 0 on their rows; the other rows keep their bits"""
    B, b0 = 33, 4
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        c = bc_case(6, 3, (33,), (), B, b0)        # a critic of one layer: the fmaxf of a hidden layer's ReLU would turn the NaN into +0.0
        args = (-1.0 / B, 0.0156, 0.01)
        clean = device_bc(h, c, *args, q_filter=1, grads=False)
        rows = [int(i) for i in np.flatnonzero(clean['filter'])[:2]]
        assert len(rows) == 2, 'fewer than two cloned rows'
        ad, x = np.array(c['ad']), np.array(c['x'])
        ad[rows[0], 1] = np.nan
        x[rows[1], 2] = np.nan
        got = device_bc(h, c, *args, q_filter=1, grads=False, ad=ad, x=x)
        assert np.isnan(got['q_demo'][rows[0]]) and np.isnan(got['q'][rows[1]]) and np.isnan(got['q_demo'][rows[1]])
        assert not got['filter'][rows].any()
        keep = np.setdiff1d(np.arange(B), rows)
        for k in ALL:
            assert np.array_equal(got[k][keep].view(np.uint8), clean[k][keep].view(np.uint8)), (k, 'a NaN row changed another row')
        for k in OUTPUTS:                                              # the row with the NaN demonstration: everything but q_demo and the filter stays
            assert np.array_equal(AC.bits(got[k][rows[0]]), AC.bits(clean[k][rows[0]])), k
        # unfiltered, the NaN demonstration is cloned: its row of g is NaN, and the last layer's dW with it
        got0 = device_bc(h, dict(c, ad=ad), *args, q_filter=0)
        assert got0['filter'][b0:].all() and np.isnan(got0['dW'][-1]).any()


# ----------------------------------------------------------------------------------------------------------------------
# 6. stale tile: the demonstration pass is the one that leaves 1e31 / inf on the tile
def stale_case(regime, B):
    """td_cases.stale_case's actor 29 -> 256 (-> 32) -> 4 as the CRITIC's body: the critic 33 -> 256 (-> 32) -> 1 has hidden activations of
    1e31 ('huge') or inf ('inf') on the rows x | ad of the demonstration pass, left in columns up to 255 of the tile when the actor
    29 -> 33 -> 4 starts, whose layer 0 multiplies the padding column 29 by its stand-in zero.  x and ad are positive, as the regimes need."""
    def make():
        t = TC.stale_case(regime, B)
        Dx, A = 25, 4
        rows = t['x']                                                  # [B, 29], every entry positive
        x, ad = np.ascontiguousarray(rows[:, :Dx]), np.ascontiguousarray(rows[:, Dx:])
        Wc = [np.array(t['Wa'][0])] + [np.array(W) for W in t['Wa'][1:]]
        Wc[-1] = np.ascontiguousarray(Wc[-1][:1])
        bc = [None] * (len(Wc) - 1) + [np.array(t['ba'][-1][:1])]
        Wa, ba = PC.scaled_actor(97, (Dx, 33, A), 0)
        Wa[0] = (Wa[0] * (1.0 if regime == 'huge' else 1e-9)).astype(F32)
        b0 = 5
        with np.errstate(over='ignore', invalid='ignore'):
            hid = np.maximum(AC.forward(np.concatenate([x, ad], 1), Wc[:1], None), 0)
        assert np.isinf(hid[b0:]).all() if regime == 'inf' else (np.isfinite(hid).all() and hid.min() > 1e30)
        return dict(Wa=Wa, ba=ba, Wc=Wc, bc=bc, x=x, ad=ad, act_a=0, act_c=0, demo_begin=b0, mixed=False)
    return cached(('bc stale', regime, B), make)


def case_stale_tile(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for regime in ('huge', 'inf'):
            for B in (TILE, TILE + 1):
                c = stale_case(regime, B)
                args = (-1.0 / B, 0.0156, 0.01)
                with np.errstate(over='ignore', invalid='ignore'):
                    m = bc_model(c['x'], c['ad'], c['demo_begin'], c['Wa'], c['ba'], c['Wc'], c['bc'], *args, q_filter=0)
                # the critic of the second pass sees x | clip(o) with |clip(o)| <= 1: its own hidden layer is huge / inf too and its q finite
                for k in ALL:
                    assert np.isfinite(np.asarray(m[k], np.float64)[c['demo_begin']:]).all(), ('the model is not finite', regime, k)
                assert all(np.isfinite(t).all() for t in m['dW'] + [b for b in m['db'] if b is not None]) and np.abs(m['dW'][0]).max() > 0
                got = device_bc(h, c, *args, q_filter=0, pad=1)
                for k in OUTPUTS + ('q_demo',):
                    assert np.isfinite(got[k][c['demo_begin']:]).all(), (regime, B, k, 'NaN or inf')
                assert all(np.isfinite(t).all() for t in got['dW'] + [b for b in got['db'] if b is not None]), (regime, B, 'NaN or inf in dW / db')
                check(got, m, ('stale', regime, B))


# ----------------------------------------------------------------------------------------------------------------------
# 7. order and independence
def same_rows(got, want, demo_begin, label):
    """the per-row outputs bit for bit; q_demo from demo_begin on (below it nothing is written)"""
    for k in ALL:
        u, v = (got[k][demo_begin:], want[k][demo_begin:]) if k == 'q_demo' else (got[k], want[k])
        assert np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), (k, label)


def case_independence(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        B, b0 = 101, 30
        c = bc_case(6, 3, (33,), (33,), B, b0, act_a=1)
        args = (-1.0 / B, 0.0156, 2.0 / (B * 3))
        big = device_bc(h, c, *args, pad=1, shift=1)
        # a row alone and in its batch, demo_begin shifted with the cut: clamp(demo_begin - s, 0, B_piece)
        for lo, hi in ((0, 1), (32, 33), (100, 101), (0, 33), (29, 31)):
            piece = dict(c, x=c['x'][lo:hi], ad=c['ad'][lo:hi])
            sb = min(max(b0 - lo, 0), hi - lo)
            sub = device_bc(h, piece, *args, grads=False, shift=2, demo_begin=sb)
            same_rows(sub, {k: big[k][lo:hi] for k in ALL}, sb, (lo, 'a row depends on its batch'))
        again = device_bc(h, c, *args, pad=1, shift=1, twice=True)
        same_rows(again, big, b0, 'two calls differ')
        for u, v in zip(big['dW'] + big['db'], again['dW'] + again['db']):
            assert np.array_equal(AC.bits(u), AC.bits(v)), 'two calls differ in dW / db'
        # a permutation of the demonstration rows among themselves and of the others among themselves: the rows' outputs move with them
        rs = np.random.RandomState(5)
        perm = np.concatenate([rs.permutation(b0), b0 + rs.permutation(B - b0)])
        moved = dict(c, x=np.ascontiguousarray(c['x'][perm]), ad=np.ascontiguousarray(c['ad'][perm]))
        rev = device_bc(h, moved, *args)
        same_rows(rev, {k: big[k][perm] for k in ALL}, b0, 'a row depends on its place')
        check(rev, model_of(moved, rev, *args), 'permuted', ('dW', 'db'))
        check(big, model_of(c, big, *args), 'in order', ('dW', 'db'))
        assert any(not np.array_equal(AC.bits(u), AC.bits(v)) for u, v in zip(rev['dW'], big['dW']))
        # every optional output NULL in turn (and all of them): the others' bits stay; grads NULL: the workspace is not touched
        for null in tuple((k,) for k in ALL) + (ALL,):
            got = device_bc(h, c, *args, null=null, shift=3)
            check(got, big, ('NULL', null))
            assert all(got[k] is None for k in null)
        for null in ((), ('q',), ('filter',), ('q', 'gaction', 'filter'), OUTPUTS + ('filter',), OUTPUTS + ('q_demo',), ('action', 'out', 'q', 'q_demo', 'filter')):
            got = device_bc(h, c, *args, grads=False, null=null, pad=2)               # (device_bc requires the workspace untouched)
            assert got['dW'] is None and got['db'] is None
            check(got, big, ('grads NULL', null))


def wave_order_run(library):
    """what tests/test_policy_grad_bc_wave_order.py runs under every wavefront order -> dict of arrays: policy_grad_cases.wave_order_run's
    shapes with demo_begin inside a tile"""
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        shapes = {'small': (6, 3, (33,), (33,), 33, 1, 9), 'wide': (3, 12, (256, 256), (256,), 33, 0, 17), 'odd': (29, 4, (255, 31), (33, 255), 32, 0, 11),
                  'flat': (2, 5, (), (), 31, 0, 10)}
        for name, (Dx, A, ah, ch, B, act, b0) in shapes.items():
            c = bc_case(Dx, A, ah, ch, B, b0, act_a=act)
            got = device_bc(h, c, -1.0 / B, 0.0156, 2.0 / (B * A), 1, pad=1, shift=1)
            assert got['filter'].any() and not got['filter'][b0:].all()
            for k in ALL:
                res[name + k] = got[k][b0:] if k == 'q_demo' else got[k]
            for l, (w, b) in enumerate(zip(got['dW'], got['db'])):
                res['%sdW%d' % (name, l)], res['%sdb%d' % (name, l)] = w, b
    return res


# ----------------------------------------------------------------------------------------------------------------------
# 8. the model is the gradient (CPU only: tests/test_policy_grad_bc_host.py)
def model_vs_autograd(widths, out_act, critic_hidden, B, seed, q_filter):
    """-> (largest max|g32 - g64| / max|g64| over the actor's dW, db and over gaction, q and q_demo; masks, clip predicates and filter equal
    to float64's; the share of demonstration rows cloned) against float64 autograd of
    gscale * sum Q + l2scale / 2 * sum o^2 + bcscale / 2 * sum_{b in F} sum_j (o - ad)^2, F the MODEL's filter, detached"""
    import torch
    Dx, A = widths[0], widths[-1]
    Wa, ba = PC.scaled_actor(seed, widths, out_act)
    Wc, bc = GC.net(seed + 50, (Dx + A,) + tuple(critic_hidden) + (1,))
    rs = np.random.RandomState(seed + 77)
    x = rs.uniform(-1, 1, (B, Dx)).astype(F32)
    ad = rs.uniform(-1, 1, (B, A)).astype(F32)
    b0 = MODEL_DEMO_BEGIN
    gscale, l2scale, bcscale = -1.0 / B, 2.0 / (B * A), 2 * 0.0078
    m = bc_model(x, ad, b0, Wa, ba, Wc, bc, gscale, bcscale, l2scale, q_filter, out_act, 0)
    dt = torch.float64
    tW, tb = [torch.tensor(W, dtype=dt, requires_grad=True) for W in Wa], [torch.tensor(b, dtype=dt, requires_grad=True) for b in ba]
    cW, cb = [torch.tensor(W, dtype=dt) for W in Wc], [torch.tensor(b, dtype=dt) for b in bc]
    tx, tad = torch.tensor(x, dtype=dt), torch.tensor(ad, dtype=dt)

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
    qd = mlp(torch.cat([tx, tad], 1), cW, cb, [])
    f64 = (np.arange(B) >= b0) & ((not q_filter) | (qd.detach().numpy()[:, 0] > q.detach().numpy()[:, 0]))
    F = torch.tensor(m['filter'].astype(np.float64))[:, None]
    loss = float(F32(gscale)) * q.sum() + float(F32(l2scale)) / 2 * (o * o).sum() + float(F32(bcscale)) / 2 * (F * (o - tad) ** 2).sum()
    loss.backward()
    inside64 = ((o >= -1) & (o <= 1)).detach().numpy()
    same = all(np.array_equal(u, v) for u, v in zip(m['masks_a'] + m['masks_c'], masks_a + masks_c)) and np.array_equal(m['inside'], inside64) and \
        np.array_equal(m['filter'], f64)
    pairs = list(zip(m['dW'] + m['db'] + [m['gaction'], m['q'], m['q_demo']],
                     [t.grad.numpy() for t in tW + tb] + [a.grad.numpy(), q.detach().numpy()[:, 0], qd.detach().numpy()[:, 0]]))
    worst = max(float(np.abs(np.asarray(u, np.float64) - v).max() / np.abs(v).max()) for u, v in pairs)
    return worst, same, float(m['filter'][b0:].mean())


# ----------------------------------------------------------------------------------------------------------------------
# 9. through the faces
def case_through_the_faces(library):
    """Actor.policy_grad_bc and policy_grad_bc_device against the model and against Actor.policy_grad, and what the faces refuse"""
    import pytest
    from pybullet_multigoal_gym_amd.critic import Critic
    Dx, A, B, b0 = 6, 3, 33, 14
    env = AC.stepped(library, 'reach', 8)
    actor, critic = env.actor, env.critic
    c = bc_case(Dx, A, (33,), (33,), B, b0, act_a=1)
    actor.load(c['Wa'], c['ba'], out_activation='tanh')
    critic.load(c['Wc'], c['bc'])
    x, ad = c['x'], c['ad']
    args = (-1.0 / B, 2 * 0.0078, 2.0 / (B * A))
    for R in (None, 16):
        for q_filter in (True, False):
            got = actor.policy_grad_bc(critic, x, ad, b0, *args, q_filter=q_filter, chunk_rows=R)
            assert got['filter'].dtype == bool and got['q_demo'].shape == (B,) and np.isnan(got['q_demo'][:b0]).all()
            m = bc_model(x, ad, b0, c['Wa'], c['ba'], c['Wc'], c['bc'], *args, q_filter=q_filter, act_a=1, out=got['out'], R=R)
            got['demo_begin'] = b0
            got['filter'] = got['filter'].astype(np.uint8)
            check(got, m, ('the face', R, q_filter))
    plain = actor.policy_grad(critic, x, args[0], args[2])
    none = actor.policy_grad_bc(critic, x, ad, B, *args)
    PC.check(none, plain, 'demo_begin = B: Actor.policy_grad')
    assert not none['filter'].any() and np.isnan(none['q_demo']).all()
    # the device form: grads into the Adam state's buffer, the demonstrations in the joined minibatch's action table
    h = env.handle
    sa = actor.adam_state()
    with Dev(h) as dev:
        d_x, d_ad = dev.put(x), dev.put(ad)
        work = actor.policy_grad_work_floats(critic, B, 16)
        d_work, d_f = dev.alloc(4 * work), dev.alloc(B + 1)
        actor.policy_grad_bc_device(critic, B, d_x, d_ad, b0, d_work, work, *args[:2], l2scale=args[2], grads=sa.g, d_filter=d_f + 1, chunk_rows=16)
        dW, db = sa.g.download()
        f = dev.get(d_f + 1, B, np.uint8)
    want = actor.policy_grad_bc(critic, x, ad, b0, *args, chunk_rows=16)
    GC.check({'dW': dW, 'db': db}, want, 'policy_grad_bc_device into AdamState.g', ('dW', 'db'))
    assert np.array_equal(f.astype(bool), want['filter'])
    out_only = actor.policy_grad_bc(critic, x, ad, b0, *args, grads=False)
    assert out_only['dW'] is None and out_only['db'] is None and np.array_equal(out_only['filter'], want['filter'])
    empty = actor.policy_grad_bc(critic, x[:0], ad[:0], 0, *args)
    assert empty['action'].shape == (0, A) and empty['q_demo'].shape == (0,) and empty['filter'].shape == (0,) and empty['dW'][0].shape == (33, Dx)
    # the faces refuse what does not fit
    wrong = Critic(env)
    wrong.load(*GC.net(814, (Dx + A + 1, 33, 1)))
    nan = float('nan')
    for bad in (lambda: actor.policy_grad_bc(wrong, x, ad, b0, *args), lambda: actor.policy_grad_bc(actor, x, ad, b0, *args),
                lambda: actor.policy_grad_bc(critic, x[:, :5], ad, b0, *args), lambda: actor.policy_grad_bc(critic, x, ad[:, :2], b0, *args),
                lambda: actor.policy_grad_bc(critic, x, ad[:-1], b0, *args), lambda: actor.policy_grad_bc(critic, x, ad, B + 1, *args),
                lambda: actor.policy_grad_bc(critic, x, ad, -1, *args), lambda: actor.policy_grad_bc(critic, x, ad, 1.5, *args),
                lambda: actor.policy_grad_bc(critic, x, ad, b0, INF, 1.0), lambda: actor.policy_grad_bc(critic, x, ad, b0, -1.0, nan),
                lambda: actor.policy_grad_bc(critic, x, ad, b0, -1.0, 1.0, -INF), lambda: actor.policy_grad_bc(critic, x, ad, b0, *args, chunk_rows=3),
                lambda: actor.policy_grad_bc(critic, x[0], ad[0], 0, *args)):
        with pytest.raises(ValueError):
            bad()
    wrong.close()
    env.close()


# ----------------------------------------------------------------------------------------------------------------------
# 10. invalid calls
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
            d_ad = dev.put(np.zeros((B, A), F32))
            NB = 4096
            outs = [dev.put(np.full(NB, SENTINEL, np.uint8)) for _ in range(11)]     # action, out, q, gaction, work, dW0, db0, dW1, db1, q_demo, filter
            work = h.policy_grad_work_floats(actor.mlp, critic.mlp, B, 0)
            work2 = h.policy_grad_work_floats(actor.mlp, critic.mlp, B, 2)
            assert 0 < work < work2 and 4 * work2 <= NB

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
            BC_KEYS = ('demo_begin', 'd_demo_action', 'demo_action_stride', 'bcscale', 'q_filter', 'd_q_demo', 'd_filter')

            def call(a=None, c=None, null_g=False, null_bc=False, R=0, **kw):
                args = dict(batch=B, d_x=d_x, x_stride=Dx, d_work=outs[4], work_floats=work2, gscale=-0.125, l2scale=0.01, grads=par, d_action=outs[0],
                            action_stride=A, d_out=outs[1], out_stride=A, d_q=outs[2], d_gaction=outs[3], gaction_stride=A)
                bca = dict(demo_begin=3, d_demo_action=d_ad, demo_action_stride=A, bcscale=0.0156, q_filter=1, d_q_demo=outs[9], d_filter=outs[10])
                size, bc_size = kw.pop('struct_size', None), kw.pop('bc_struct_size', None)
                bca.update({k: kw.pop(k) for k in BC_KEYS if k in kw})
                args.update(kw)
                s, t = h.policy_grad_struct(**args), h.policy_bc_struct(**bca)
                if size is not None:
                    s.struct_size = size
                if bc_size is not None:
                    t.struct_size = bc_size
                return h.L.lib.pmg_policy_grad_bc_device(h.h, C.byref(a or mlp(actor)), C.byref(c or mlp(critic)), None if null_g else C.byref(s),
                                                         None if null_bc else C.byref(t), C.c_int64(R))
            bad_kw = (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)), dict(width=(1, 0)),
                      dict(d_weight=(0, None)), dict(out_activation=2))
            no_outs = dict(grads=None, d_action=None, d_out=None, d_q=None, d_gaction=None)
            bad = [lambda kw=kw: call(a=mlp(actor, **kw)) for kw in bad_kw] + [lambda kw=kw: call(c=mlp(critic, **kw)) for kw in bad_kw] + [
                # everything pmg_policy_grad_device rejects
                lambda: call(a=mlp(actor, d_weight=(1, actor.d_w[1] + 2))), lambda: call(c=mlp(critic, d_bias=(0, critic.d_b[0] + 1))),
                lambda: call(c=mlp(wide)), lambda: call(c=mlp(two)),
                lambda: call(gscale=nan), lambda: call(gscale=INF), lambda: call(l2scale=nan), lambda: call(l2scale=-INF),
                lambda: call(d_q_demo=None, d_filter=None, **no_outs),                                 # d_q_demo and d_filter count as outputs
                lambda: call(grads=params(d_weight=(1, None))), lambda: call(grads=params(d_bias=(0, None))),
                lambda: call(a=mlp(nobias)),
                lambda: call(d_work=None), lambda: call(work_floats=work - 1), lambda: call(work_floats=0), lambda: call(work_floats=work2 - 1, R=2),
                lambda: call(grads=None, d_work=None), lambda: call(grads=None, work_floats=work - 1),
                lambda: call(d_x=None), lambda: call(d_x=d_x + 2), lambda: call(d_action=outs[0] + 1), lambda: call(d_out=outs[1] + 2), lambda: call(d_q=outs[2] + 3),
                lambda: call(d_gaction=outs[3] + 1), lambda: call(d_work=outs[4] + 2), lambda: call(grads=params(d_weight=(0, outs[5] + 2))),
                lambda: call(grads=params(d_bias=(1, outs[8] + 1))),
                lambda: call(x_stride=Dx - 1), lambda: call(action_stride=A - 1), lambda: call(out_stride=0), lambda: call(gaction_stride=A - 1),
                lambda: call(batch=-1), lambda: call(R=-2), lambda: call(R=1), lambda: call(R=3),
                lambda: call(batch=2 * 65535 + 1, R=2, work_floats=1 << 40, demo_begin=0),
                lambda: call(null_g=True), lambda: call(struct_size=C.sizeof(PmgPolicyGrad) - 8), lambda: call(struct_size=0),
                # and the cloning term's own
                lambda: call(null_bc=True), lambda: call(bc_struct_size=C.sizeof(PmgPolicyBc) - 8), lambda: call(bc_struct_size=0),
                lambda: call(bcscale=nan), lambda: call(bcscale=INF), lambda: call(bcscale=-INF),
                lambda: call(q_filter=2), lambda: call(q_filter=-1),
                lambda: call(demo_begin=-1), lambda: call(demo_begin=B + 1),
                lambda: call(d_demo_action=None), lambda: call(d_demo_action=None, demo_begin=B - 1), lambda: call(d_demo_action=d_ad + 2),
                lambda: call(d_demo_action=d_ad + 1, demo_begin=B), lambda: call(demo_action_stride=A - 1), lambda: call(demo_action_stride=0),
                lambda: call(d_q_demo=outs[9] + 1), lambda: call(d_q_demo=outs[9] + 2)]
            g0 = h.policy_grad_struct(B, d_x, Dx, outs[4], work2, -0.125, d_q=outs[2])
            t0 = h.policy_bc_struct(3, d_ad, A, 0.0156)
            assert h.L.lib.pmg_policy_grad_bc_device(h.h, None, C.byref(mlp(critic)), C.byref(g0), C.byref(t0), C.c_int64(0)) == E_INVALID
            assert h.L.lib.pmg_policy_grad_bc_device(h.h, C.byref(mlp(actor)), None, C.byref(g0), C.byref(t0), C.c_int64(0)) == E_INVALID

            def untouched():
                h.sync()
                for o in outs:
                    assert (dev.get(o, NB, np.uint8) == SENTINEL).all()
            for k, f in enumerate(bad):
                assert f() == E_INVALID, k
                assert h.L.error(h.h), k
            untouched()
            assert call(batch=0, demo_begin=0) == 0 and call(batch=0, work_floats=0, demo_begin=0) == 0 and call(batch=0, R=2, demo_begin=0, d_demo_action=None) == 0
            untouched()
            # the allowed corners: demo_begin = B with NULL demonstrations, d_filter at an odd address, one of the two new outputs alone, chunks
            assert call(demo_begin=B, d_demo_action=None, demo_action_stride=0) == 0 and call(d_filter=outs[10] + 1) == 0 and call(d_filter=outs[10] + 3, demo_begin=0) == 0
            assert call(d_q_demo=None, d_filter=outs[10], **no_outs) == 0 and call(d_q_demo=outs[9], d_filter=None, **no_outs) == 0
            assert call(R=2) == 0 and call(R=8, work_floats=work) == 0 and call(q_filter=0, demo_begin=0) == 0 and call(bcscale=0.0) == 0 and call(bcscale=-1.0) == 0
            p_nb = params()
            p_nb.d_bias[0] = p_nb.d_bias[1] = None
            assert call(a=mlp(nobias), grads=p_nb) == 0 and call(grads=None) == 0
            h.sync()
