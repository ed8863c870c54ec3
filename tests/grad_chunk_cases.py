"""The cases of the chunked batch reduction (include/pmg.h pmg_mlp_grad_chunked_device, pmg_mlp_grad_chunked_work_floats) and
their numpy model, shared by tests/test_grad_chunk_emulated.py (the g++ build of the product sources over the fiber emulator),
tests/test_gpu_grad_chunk.py (libpmg_hip.so on the MI355X), tests/test_grad_chunk_host.py (the model against torch.autograd, the faces'
ValueErrors) and tests/test_grad_chunk_wave_order.py.  Everything stands on tests/grad_cases.py, which is imported and not edited.

The model.  Per-row quantities do not depend on the batch a row is in, so chunk c's partial IS grad_cases.model on the chunk's rows of
x / a / gout / target with the caller's gscale, and the merge is float32 addition of the partials in ascending c; gx / ga / out are
grad_cases.model's on the whole batch.  Bars: those of grad_cases -- dW, db, gx, ga and out bit for bit (zeros by value), out under tanh
within ACTION_TOL of the float64 tanh and everything else bit-equal to the model evaluated from the device's own out."""
import ctypes as C

import numpy as np

import actor_cases as AC
import grad_cases as GC
from actor_cases import ACTION_TOL, Net
from grad_cases import F32, Params, check, eq_val, read_rows, rows_out
from normalizer_cases import SENTINEL, Dev, handle
from td_cases import Out, cached, put_rows

E_INVALID = -1
CHUNKS = (2, 16, 34)            # at B = 101: 16-step blocks (34 rows = 16 + 16 + 2), the pair remainder, an odd last chunk (34 + 34 + 33)
MAX_CHUNKS = 65535              # PMG_GRAD_MAX_CHUNKS of include/pmg.h
CRITIC = ((13, 256, 256, 256, 1), 9)

# The chunked model against float64 autograd (case 8): max|g32 - g64| / max|g64| per tensor (dW, db, gx) over GC.MODEL_NETS x GC.MODEL_SEEDS at
# B = 101, R = 34 (three partial chains and two float32 additions per element), equal float32 and float64 ReLU masks every time, measured on
# the CPU:   9-256-256-256-1: 2.32e-6   6-256-256-256-3 tanh: 1.12e-6   33-33-4: 3.74e-7   5-1: 1.90e-7      (the largest: 2.32e-6)
# against 2.79e-6 for the single chain of grad_cases over B = 33 and 101.  The bar is 4 x the largest, the project's convention; as there, a
# MEASURED value above 1e-5 would mean the model is wrong, not that the bar is tight.
CHUNK_MODEL_WORST = 2.32e-6
assert CHUNK_MODEL_WORST < 1e-5
CHUNK_MODEL_TOL = 4 * CHUNK_MODEL_WORST
MODEL_B, MODEL_R = 101, 34


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def chunk_model(x, Ws, bs, R, out_act=0, gout=None, target=None, gscale=1.0, out=None, a=None):
    """-> GC.model's dict with dW / db = the partials of the chunks of R rows added in ascending chunk order, in float32"""
    m = GC.model(x, Ws, bs, out_act, gout, target, gscale, out, a, weights=False)
    cut = lambda t, s: None if t is None else t[s]
    dW = db = None
    with np.errstate(over='ignore', invalid='ignore'):
        for lo in range(0, x.shape[0], R):
            s = slice(lo, lo + R)
            p = GC.model(x[s], Ws, bs, out_act, cut(gout, s), cut(target, s), gscale, cut(out, s), cut(a, s))
            if dW is None:
                dW, db = list(p['dW']), list(p['db'])
            else:
                dW = [(u + v).astype(F32) for u, v in zip(dW, p['dW'])]
                db = [None if u is None else (u + v).astype(F32) for u, v in zip(db, p['db'])]
    m['dW'], m['db'] = dW, db
    return m


# ----------------------------------------------------------------------------------------------------------------------
# device calls
def device_grad_chunked(h, Ws, bs, x, R, a=None, out_act=0, gout=None, target=None, gscale=1.0, grads=True, null=(), pad=0, shift=0, twice=False,
                        nan_work=False):
    """pmg_mlp_grad_chunked_device as GC.device_grad calls pmg_mlp_grad_device: canary-framed, sentinel-filled outputs, the workspace sized to
    exactly the chunked figure (with grads NULL: to the unchunked one).  nan_work: the workspace starts as NaN bit patterns."""
    B, Dx, A = x.shape[0], x.shape[1], Ws[-1].shape[0]
    Da = 0 if a is None else a.shape[1]
    with Dev(h) as dev:
        n = Net(h, dev, Ws, bs, out_act)
        d_x, xs = put_rows(h, dev, x, pad, shift)
        d_a, as_ = (None, 0) if a is None else put_rows(h, dev, a, pad, (shift + 1) & 3)
        d_go, gos = (None, 0) if gout is None else put_rows(h, dev, np.asarray(gout, F32), pad, (shift + 2) & 3)
        d_t, ts = (None, 0) if target is None else put_rows(h, dev, np.asarray(target, F32), pad, (shift + 3) & 3)
        o_gx, o_ga, o_out = rows_out(dev, B, Dx, pad, (shift + 1) & 3), rows_out(dev, B, max(Da, 1), pad, (shift + 2) & 3), rows_out(dev, B, A, pad, (shift + 3) & 3)
        par = Params(h, dev, Ws, bs, shift)
        work = h.mlp_grad_chunked_work_floats(n.mlp, B, R) if grads else h.mlp_grad_work_floats(n.mlp, B)
        assert work >= h.mlp_grad_work_floats(n.mlp, B) >= 0
        o_work = Out(dev, 4 * work, 4 * (shift & 3))
        if nan_work and work:
            h.upload(o_work.ptr, np.full(work, 0x7FC00000 | 0x1234, np.uint32))
        use_ga = Da > 0 and 'ga' not in null
        g = h.grad_struct(B, d_x, xs, Dx, o_work.ptr, work, d_a, as_, Da, d_go, gos, d_t, ts, gscale, par.struct if grads else None,
                          None if 'gx' in null else o_gx.ptr, Dx + pad, o_ga.ptr if use_ga else None, Da + pad if use_ga else 0,
                          None if 'out' in null else o_out.ptr, A + pad)
        for _ in range(2 if twice else 1):
            h.mlp_grad_chunked_device(n.mlp, g, R)
        h.sync()
        o_work.read(np.uint8)
        dW, db = par.read(written=grads)
        return {'dW': dW, 'db': db, 'gx': read_rows(o_gx, B, Dx, pad, 'gx' not in null), 'ga': read_rows(o_ga, B, max(Da, 1), pad, use_ga),
                'out': read_rows(o_out, B, A, pad, 'out' not in null)}


def chunk_case(widths, Dx, B, R, bias=True, out_act=0, head='target'):
    """GC.grad_case's network and rows with the chunked model in place of the single chain"""
    c = GC.grad_case(widths, Dx, B, bias, out_act, head)
    m = None if out_act else cached(('chunk model', tuple(widths), Dx, B, R, bias, head), lambda: chunk_model(c['x'], c['Ws'], c['bs'], R, 0, a=c['a'], **c['kw']))
    return dict(c, m=m)


def run_case(h, c, R, n=0, **kw):
    return device_grad_chunked(h, c['Ws'], c['bs'], c['x'], R, c['a'], c['out_act'], pad=n % 3, shift=n % 4, **dict(c['kw'], **kw))


# ----------------------------------------------------------------------------------------------------------------------
# 1. bit-exact
def nets(group):
    """(widths, Dx) of a group, the shapes of grad_cases without their batches; the two 3 x 256 actors of RAW_CASES are a group of their own"""
    cases = {'cat': lambda: GC.cat_cases((33,)), 'raw': lambda: GC.RAW_CASES[:-2], 'raw256': lambda: GC.RAW_CASES[-2:], 'extreme': lambda: GC.EXTREME_CASES,
             'critic': lambda: [CRITIC + (0,)]}[group]()
    return [(w, Dx) for w, Dx, _ in cases]


GROUPS = ('cat', 'raw', 'raw256', 'extreme', 'critic')
assert len(nets('raw')) + len(nets('raw256')) == len(GC.RAW_CASES) and all(len(w) == 5 for w, _ in nets('raw256'))


def case_bit_exact(library, group, R, B, heads=('target', 'gout', 'const')):
    """every network of the group on B rows in chunks of R rows; the heads and the bias in turn as in grad_cases"""
    k = GC.BATCHES.index(B)
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, Dx) in enumerate(nets(group)):
            c = chunk_case(widths, Dx, B, R, bias=n % 4 != 3, head=heads[(n + k) % len(heads)])
            check(run_case(h, c, R, n + k), c['m'], (widths, Dx, B, R))


def case_tanh(library, R):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        widths, Dx = (6, 33, 3), 6
        for n, B in enumerate(GC.BATCHES):
            for head in ('gout', 'target', 'const'):
                c = chunk_case(widths, Dx, B, R, out_act=1, head=head)
                got = run_case(h, c, R, n)
                z = GC.forward_saved(c['x'], c['Ws'], c['bs'])[1]
                err = float(np.abs(got['out'] - np.tanh(z.astype(np.float64))).max())
                worst = max(worst, err)
                assert err <= ACTION_TOL, (widths, head, B, R, err)
                check(got, chunk_model(c['x'], c['Ws'], c['bs'], R, 1, out=got['out'], **c['kw']), (widths, head, B, R, 'from the device out'), ('dW', 'db', 'gx', 'ga'))
    print('tanh output, R = %d: largest |out - tanh64(z)| = %.3g (bar %.3g)' % (R, worst, ACTION_TOL))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# 2. chunk edges
def case_chunk_edges(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        n = 0
        for widths, Dx in (((9, 33, 1), 6), ((6, 33, 3), 6)):
            for R in (2, 32):
                for Cn in (2, 3):
                    for B in (R * Cn, R * Cn + 1, R * Cn - 1):       # whole chunks; a last chunk of one row (the tail step alone); one row short
                        c = chunk_case(widths, Dx, B, R, head=('target', 'gout', 'const')[n % 3])
                        check(run_case(h, c, R, n), c['m'], (widths, B, R))
                        n += 1
            # R >= B is one chunk: what pmg_mlp_grad_device returns from the same library on the same inputs
            for B, R in ((33, 34), (32, 32), (1, 2), (101, 1 << 20)):
                c = GC.grad_case(widths, Dx, B, head='target')
                single = GC.run_case(h, c, 1)
                one = run_case(h, c, R, 1)
                for k in ('gx', 'ga', 'out'):
                    if single[k] is not None:
                        assert np.array_equal(AC.bits(one[k]), AC.bits(single[k])), (widths, B, R, k)
                for u, v in zip(one['dW'] + one['db'], single['dW'] + single['db']):
                    assert np.array_equal(AC.bits(u), AC.bits(v)), (widths, B, R, 'one chunk is not the single chain')
                check(one, c['m'], (widths, B, R, 'one chunk'))


# ----------------------------------------------------------------------------------------------------------------------
# 3. nothing stale is read, everything is overwritten
def case_nothing_stale(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, Dx, B, R) in enumerate((((9, 33, 1), 6, 101, 34), ((6, 33, 3), 6, 33, 2), ((33, 255, 31, 2), 29, 33, 16))):
            c = chunk_case(widths, Dx, B, R, bias=n != 1)
            once = run_case(h, c, R, n, nan_work=True)                 # grads start as sentinel bytes (Params), the workspace as NaNs
            check(once, c['m'], (widths, B, R, 'NaN workspace'))
            twice = run_case(h, c, R, n, nan_work=True, twice=True)
            for k in ('gx', 'ga', 'out'):
                if once[k] is not None:
                    assert np.array_equal(AC.bits(twice[k]), AC.bits(once[k])), (widths, k, 'two calls differ')
            for u, v in zip(once['dW'] + once['db'], twice['dW'] + twice['db']):
                assert (u is None) == (v is None)
                if u is not None:
                    assert np.array_equal(AC.bits(u), AC.bits(v)), (widths, 'two calls differ in dW / db')


# ----------------------------------------------------------------------------------------------------------------------
# 4. order
def case_order(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        widths, Dx, B, R = (9, 33, 1), 6, 101, 34
        c = GC.grad_case(widths, Dx, B, head='gout')
        x, a, g = c['x'], c['a'], c['kw']['gout']
        base = device_grad_chunked(h, c['Ws'], c['bs'], x, R, a, gout=g, pad=1, shift=1)
        check(base, chunk_model(x, c['Ws'], c['bs'], R, a=a, gout=g), 'base')
        # rows permuted WITHIN the chunks: the model on the permuted rows, and another dW than before
        perm = np.concatenate([lo + np.random.RandomState(7 + lo).permutation(min(R, B - lo)) for lo in range(0, B, R)])
        assert sorted(perm) == list(range(B)) and all(perm[i] // R == i // R for i in range(B)) and not np.array_equal(perm, np.arange(B))
        xp, ap, gp = (np.ascontiguousarray(t[perm]) for t in (x, a, g))
        got = device_grad_chunked(h, c['Ws'], c['bs'], xp, R, ap, gout=gp, shift=2)
        check(got, chunk_model(xp, c['Ws'], c['bs'], R, a=ap, gout=gp), 'permuted within the chunks')
        for k in ('gx', 'ga', 'out'):
            assert np.array_equal(AC.bits(got[k]), AC.bits(base[k][perm])), (k, 'a row depends on its place')
        assert any(not np.array_equal(AC.bits(u), AC.bits(v)) for u, v in zip(got['dW'], base['dW'])), 'dW ignores the order within a chunk'
        # another R: the model of that R; gx / ga / out are the unchunked call's for every R
        single = GC.device_grad(h, c['Ws'], c['bs'], x, a, gout=g, pad=1, shift=1)
        seen = [base['dW']]
        for R2 in (2, 16, 32, 50, 100, 102):
            got = device_grad_chunked(h, c['Ws'], c['bs'], x, R2, a, gout=g, pad=1, shift=1)
            check(got, cached(('chunk order', R2), lambda: chunk_model(x, c['Ws'], c['bs'], R2, a=a, gout=g)), ('R', R2))
            for k in ('gx', 'ga', 'out'):
                assert np.array_equal(AC.bits(got[k]), AC.bits(single[k])), (R2, k, 'an input gradient depends on R')
            seen.append(got['dW'])
        for k in ('gx', 'ga', 'out'):
            assert np.array_equal(AC.bits(base[k]), AC.bits(single[k])), (R, k)
        assert len({tuple(AC.bits(w).tobytes() for w in dW) for dW in seen}) > 1, 'dW ignores R'
        for u, v in zip(seen[-1], single['dW']):                          # R = 102 >= B: the single chain
            assert np.array_equal(AC.bits(u), AC.bits(v))


# ----------------------------------------------------------------------------------------------------------------------
# 5. masks and inf
def case_masks_and_inf(library):
    R = 2
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for regime in ('huge', 'inf'):
            for B in (GC.TILE, GC.TILE + 1):
                c = GC.stale_case(regime, B)
                got = device_grad_chunked(h, c['Ws'], c['bs'], c['x'], R, c['a'], gscale=-1.0 / B, grads=regime == 'huge', pad=1)
                for k in ('gx', 'ga', 'out'):
                    assert np.isfinite(got[k]).all(), (regime, B, k, 'NaN or inf')
                if regime == 'huge':
                    want = cached(('chunk stale', B), lambda: chunk_model(c['x'], c['Ws'], c['bs'], R, a=c['a'], gscale=-1.0 / B))
                    assert all(np.isfinite(t).all() for t in want['dW'])
                    check(got, want, (regime, B))
                else:
                    check(got, c['m'], (regime, B))
        # a masked unit whose s is inf (grad_cases test 5): delta_0[.][0] is a real +0.0, so no partial sees 0 * inf
        Ws, bs = [np.array([[-1, 0], [0, 1]], F32), np.array([[1e30, 2]], F32)], None
        x = np.array([[1, 1], [2, 3], [3, 1], [1, 2], [2, 2]], F32)
        got = device_grad_chunked(h, Ws, bs, x, R, gscale=1e10)
        assert np.array_equal(got['gx'], np.array([[0, 2e10]] * 5, F32)), got['gx']
        assert all(np.isfinite(t).all() for t in got['dW']), 'a masked inf reached a partial as NaN'
        with np.errstate(over='ignore'):
            check(got, chunk_model(x, Ws, bs, R, gscale=1e10), 'masked inf')


# ----------------------------------------------------------------------------------------------------------------------
# 6. input-only
def case_input_only(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, Dx, B, R) in enumerate((((9, 33, 1), 6, 101, 34), ((13, 256, 256, 256, 1), 9, 33, 2), ((6, 33, 3), 6, 33, 16))):
            c = GC.grad_case(widths, Dx, B, head='const')
            got = run_case(h, c, R, n, grads=False)                    # (the workspace is at the UNCHUNKED size)
            single = GC.run_case(h, c, n, grads=False)
            assert got['dW'] is None and got['db'] is None
            for k in ('gx', 'ga', 'out'):
                if single[k] is not None:
                    assert np.array_equal(AC.bits(got[k]), AC.bits(single[k])), (widths, k)
            check(got, c['m'], (widths, 'input-only'), ('gx', 'ga', 'out'))


# ----------------------------------------------------------------------------------------------------------------------
# 7. invalid calls
def case_invalid_calls(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B, R = 6, 3, 8, 2
        Wc, bc = GC.net(91, (Dx + A, 16, 1))
        Wn, _ = GC.net(92, (Dx + A, 16, 1), bias=False)
        nan = float('nan')
        with Dev(h) as dev:
            critic, nobias = Net(h, dev, Wc, bc, 0), Net(h, dev, Wn, None, 0)
            d_x, d_a, d_go = dev.put(np.zeros((B, Dx + A), F32)), dev.put(np.zeros((B, A), F32)), dev.put(np.zeros((B, 1), F32))
            NB = 8192
            outs = [dev.put(np.full(NB, SENTINEL, np.uint8)) for _ in range(9)]      # gx, ga, out, work, dW0, db0, dW1, db1, spare
            work = h.mlp_grad_chunked_work_floats(critic.mlp, B, R)
            single = h.mlp_grad_work_floats(critic.mlp, B)
            P = sum((K + 1) * J for J, K in (W.shape for W in Wc))
            assert work == single + 4 * P and 0 < 4 * work <= NB
            par = h.params_struct([outs[4], outs[6]], [outs[5], outs[7]])

            def mlp(n, **kw):
                m = h.mlp_struct(n.widths, n.d_w, n.d_b, 0)
                for k, v in kw.items():
                    if k in ('width', 'd_weight', 'd_bias'):
                        getattr(m, k)[v[0]] = v[1]
                    else:
                        setattr(m, k, v)
                return m

            def params(**kw):
                p = h.params_struct([outs[4], outs[6]], [outs[5], outs[7]])
                for k, v in kw.items():
                    getattr(p, k)[v[0]] = v[1]
                return p

            def grad(m=None, null_g=False, chunk_rows=R, **kw):
                a = dict(batch=B, d_x=d_x, x_stride=Dx, x_dim=Dx, d_work=outs[3], work_floats=work, d_a=d_a, a_stride=A, a_dim=A, d_gout=None, gout_stride=1,
                         d_target=d_go, target_stride=1, gscale=0.25, grads=par, d_gx=outs[0], gx_stride=Dx, d_ga=outs[1], ga_stride=A, d_out=outs[2], out_stride=1)
                size = kw.pop('struct_size', None)
                a.update(kw)
                s = h.grad_struct(**a)
                if size is not None:
                    s.struct_size = size
                return h.L.lib.pmg_mlp_grad_chunked_device(h.h, C.byref(m or mlp(critic)), None if null_g else C.byref(s), C.c_int64(chunk_rows))
            bad_nets = [mlp(critic, **kw) for kw in (dict(struct_size=C.sizeof(GC.PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                                     dict(d_weight=(0, None)), dict(out_activation=2))]
            bad = [lambda m=m: grad(m) for m in bad_nets] + [
                lambda: grad(chunk_rows=0), lambda: grad(chunk_rows=1), lambda: grad(chunk_rows=3), lambda: grad(chunk_rows=-2),
                lambda: grad(work_floats=work - 1), lambda: grad(work_floats=single), lambda: grad(work_floats=0), lambda: grad(d_work=None),
                # a sample of what pmg_mlp_grad_device rejects
                lambda: grad(null_g=True), lambda: grad(struct_size=C.sizeof(GC.PmgMlpGrad) - 8), lambda: grad(d_x=None), lambda: grad(d_a=None),
                lambda: grad(x_dim=Dx - 1), lambda: grad(d_gout=d_go), lambda: grad(gscale=nan), lambda: grad(gscale=GC.INF),
                lambda: grad(grads=None, d_gx=None, d_ga=None, d_out=None), lambda: grad(grads=params(d_weight=(1, None))),
                lambda: grad(grads=params(d_bias=(0, None))), lambda: grad(mlp(nobias)), lambda: grad(d_x=d_x + 2), lambda: grad(d_work=outs[3] + 2),
                lambda: grad(grads=params(d_bias=(1, outs[7] + 1))), lambda: grad(x_stride=Dx - 1), lambda: grad(gx_stride=Dx - 1), lambda: grad(out_stride=0),
                lambda: grad(batch=-1)]
            assert h.L.lib.pmg_mlp_grad_chunked_device(h.h, None, C.byref(h.grad_struct(B, d_x, Dx, Dx, outs[3], work)), C.c_int64(R)) == E_INVALID
            lib_floats = h.L.lib.pmg_mlp_grad_chunked_work_floats
            assert lib_floats(None, C.c_int64(B), C.c_int64(R)) < 0 and h.mlp_grad_chunked_work_floats(critic.mlp, -1, R) < 0
            for r in (0, 1, 3, -2):
                assert h.mlp_grad_chunked_work_floats(critic.mlp, B, r) < 0, r
            assert h.mlp_grad_chunked_work_floats(mlp(critic, width=(1, 257)), B, R) < 0 and h.mlp_grad_chunked_work_floats(mlp(critic, num_layers=5), B, R) < 0
            assert h.mlp_grad_chunked_work_floats(critic.mlp, 0, R) == 0
            assert h.mlp_grad_chunked_work_floats(critic.mlp, B, B) == single == h.mlp_grad_chunked_work_floats(critic.mlp, B, B + 2)      # one chunk: no partials
            assert h.mlp_grad_chunked_work_floats(critic.mlp, B + 1, B) == h.mlp_grad_work_floats(critic.mlp, B + 1) + 2 * P

            def untouched():
                h.sync()
                for o in outs:
                    assert (dev.get(o, NB, np.uint8) == SENTINEL).all()
            for k, call in enumerate(bad):
                assert call() == E_INVALID, k
                assert h.L.error(h.h), k
            untouched()
            assert grad(batch=0) == 0 and grad(batch=0, work_floats=0) == 0            # a no-op that leaves grads untouched
            untouched()
            # what is allowed: input gradients alone at the UNCHUNKED workspace size, one chunk at that size, a network without biases
            assert grad(grads=None, work_floats=single) == 0
            assert grad(chunk_rows=B, work_floats=single) == 0 and grad(chunk_rows=1 << 40, work_floats=single) == 0
            p_nb = params()
            p_nb.d_bias[0] = p_nb.d_bias[1] = None
            assert grad(mlp(nobias), grads=p_nb) == 0
            h.sync()
        # one chunk more than the launcher puts in one grid, on a 1 -> 1 network whose buffers hold that call in full
        W1, b1 = GC.net(93, (1, 1))
        Bmax = R * MAX_CHUNKS
        with Dev(h) as dev:
            tiny = Net(h, dev, W1, b1, 0)
            assert h.mlp_grad_chunked_work_floats(tiny.mlp, Bmax, R) == Bmax + 2 * MAX_CHUNKS
            for Bx in (Bmax + 1, Bmax + R):
                assert h.mlp_grad_chunked_work_floats(tiny.mlp, Bx, R) < 0
                room = Bx + 2 * (MAX_CHUNKS + 1)
                d_rows, o_out, o_work = dev.put(np.zeros(Bx, F32)), Out(dev, 4 * Bx), Out(dev, 4 * room)
                par1 = Params(h, dev, W1, b1)
                g = h.grad_struct(Bx, d_rows, 1, 1, o_work.ptr, room, grads=par1.struct, d_out=o_out.ptr, out_stride=1)
                assert h.L.lib.pmg_mlp_grad_chunked_device(h.h, C.byref(tiny.mlp), C.byref(g), C.c_int64(R)) == E_INVALID
                assert 'chunks' in h.L.error(h.h)
                h.sync()
                o_out.read(written=False), o_work.read(written=False), par1.read(written=False)


# ----------------------------------------------------------------------------------------------------------------------
# 8. the model is the gradient (CPU only: tests/test_grad_chunk_host.py)
def chunk_model_vs_autograd(widths, out_act, seed, B=MODEL_B, R=MODEL_R):
    """GC.model_vs_autograd with the chunked model: -> (largest max|g32 - g64| / max|g64| over dW, db, gx, masks equal)"""
    import torch
    Ws, bs = GC.net(seed, widths)
    rs = np.random.RandomState(seed + 77)
    x = rs.uniform(-1, 1, (B, widths[0])).astype(F32)
    g = rs.uniform(-1.0 / B, 1.0 / B, (B, widths[-1])).astype(F32)
    m = chunk_model(x, Ws, bs, R, out_act, gout=g)
    tW = [torch.tensor(W, dtype=torch.float64, requires_grad=True) for W in Ws]
    tb = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in bs]
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    hcur, masks = tx, []
    for l in range(len(tW)):
        z = hcur @ tW[l].T + tb[l]
        if l + 1 < len(tW):
            masks.append((z > 0).numpy())
            hcur = torch.relu(z)
    o = torch.tanh(z) if out_act else z
    (o * torch.tensor(g, dtype=torch.float64)).sum().backward()
    want = [t.grad.numpy() for t in tW] + [t.grad.numpy() for t in tb] + [tx.grad.numpy()]
    same = all(np.array_equal(u, v) for u, v in zip(m['masks'], masks))
    worst = max(float(np.abs(np.asarray(u, np.float64) - v).max() / np.abs(v).max()) for u, v in zip(list(m['dW']) + list(m['db']) + [m['gx']], want))
    return worst, same


# ----------------------------------------------------------------------------------------------------------------------
# 9. one whole update through the faces, the two full gradients chunked
def case_whole_update(library, R=32):
    """GC.case_whole_update's sequence (the docstring of critic.py) at B = 101 with chunk_rows = R on the two full-gradient calls: every
    intermediate is held as there, with the chunked model in place of the single chain"""
    from pybullet_multigoal_gym_amd.actor import Actor
    from pybullet_multigoal_gym_amd.critic import Critic
    import td_cases as TC
    Dx, A, B, gamma, tau, lr = 6, 3, 101, 0.98, 0.05, 1e-3
    env = AC.stepped(library, 'reach', 8)
    actor, critic, actor_t, critic_t = env.actor, env.critic, Actor(env), Critic(env)
    Wa, ba = GC.net(801, (Dx, 33, A))
    Wc, bc = GC.net(802, (Dx + A, 33, 1))
    Wat, bat = GC.net(803, (Dx, 33, A))
    Wct, bct = GC.net(804, (Dx + A, 33, 1))
    actor.load(Wa, ba, out_activation='identity')
    actor_t.load(Wat, bat, out_activation='identity')
    critic.load(Wc, bc)
    critic_t.load(Wct, bct)
    rs = np.random.RandomState(805)
    x, xn = rs.uniform(-2, 2, (B, Dx)).astype(F32), rs.uniform(-2, 2, (B, Dx)).astype(F32)
    act, r = rs.uniform(-1, 1, (B, A)).astype(F32), -rs.randint(0, 2, B).astype(F32)
    sa, sc = actor.adam_state(), critic.adam_state()
    assert critic.grad_work_floats(B, R) == critic.grad_work_floats(B) + 4 * sum((K + 1) * J for J, K in (W.shape for W in Wc))
    # critic: y, MSE gradient in chunks, Adam
    y, _, _ = critic_t.td_target(actor_t, xn, r, gamma, -1.0 / (1.0 - gamma), 0.0)
    TC.eq_y(y, TC.td_model(xn, r, Wat, bat, Wct, bct, gamma, -1.0 / (1.0 - gamma), 0.0)['y'], 'y')
    gc = critic.grad(x, act, target=y[:, None], gscale=2.0 / B, chunk_rows=R)
    mc = chunk_model(x, Wc, bc, R, a=act, target=y[:, None], gscale=2.0 / B)
    check(gc, mc, 'critic gradient')
    single = GC.model(x, Wc, bc, a=act, target=y[:, None], gscale=2.0 / B)
    assert any(not np.array_equal(AC.bits(u), AC.bits(v)) for u, v in zip(mc['dW'], single['dW'])), 'the chunked model is the single chain here: the case shows nothing'
    critic.adam_step_device(gc, sc, lr)
    Wc1, bc1 = critic.parameters()
    worst = 0.0
    for got, p, g in [(Wc1[l], Wc[l], mc['dW'][l]) for l in range(2)] + [(bc1[l], bc[l], mc['db'][l]) for l in range(2)]:
        _, _, p64, step = GC.adam_model(p, g, np.zeros_like(p), np.zeros_like(p), lr, 0.9, 0.999, 1e-8, 1)
        worst = max(worst, GC.adam_error(got, p64, step, 'critic adam'))
    # actor: a = pi(x), dQ / da from the UPDATED critic with grads = None (chunk_rows has nothing to chunk there), back through the actor, Adam
    a_pi = actor.forward(x)
    eq_val(a_pi, AC.forward(x, Wa, ba), 'pi(x)')
    gq = critic.grad(x, a_pi, grads=None, gscale=-1.0 / B, chunk_rows=R)
    assert gq['dW'] is None and gq['db'] is None
    check(gq, GC.model(x, Wc1, bc1, a=a_pi, gscale=-1.0 / B, weights=False), 'dQ / da', ('gx', 'ga', 'out'))
    ga = actor.grad(x, gout=gq['ga'], chunk_rows=R)
    ma = chunk_model(x, Wa, ba, R, gout=gq['ga'])
    check(ga, ma, 'actor gradient')
    actor.adam_step_device(ga, sa, lr)
    Wa1, ba1 = actor.parameters()
    for got, p, g in [(Wa1[l], Wa[l], ma['dW'][l]) for l in range(2)] + [(ba1[l], ba[l], ma['db'][l]) for l in range(2)]:
        _, _, p64, step = GC.adam_model(p, g, np.zeros_like(p), np.zeros_like(p), lr, 0.9, 0.999, 1e-8, 1)
        worst = max(worst, GC.adam_error(got, p64, step, 'actor adam'))
    assert worst <= GC.ADAM_TOL, worst
    assert sa.t == 1 and sc.t == 1
    # m and v after the first step from zero moments, bit for bit from the chunked gradients
    for state, mdl in ((sc, mc), (sa, ma)):
        (mW, mb), (vW, vb) = state.m.download(), state.v.download()
        for l in range(2):
            for g, m_got, v_got in ((mdl['dW'][l], mW[l], vW[l]), (mdl['db'][l], mb[l], vb[l])):
                m1, v1, _, _ = GC.adam_model(np.zeros_like(g), g, np.zeros_like(g), np.zeros_like(g), lr, 0.9, 0.999, 1e-8, 1)
                assert np.array_equal(AC.bits(m_got), AC.bits(m1)) and np.array_equal(AC.bits(v_got), AC.bits(v1)), ('m / v', l)
    # targets: Polyak of the device's own parameters, bit for bit
    actor_t.soft_update_from(actor, tau)
    critic_t.soft_update_from(critic, tau)
    for net_t, new, old in ((actor_t, (Wa1, ba1), (Wat, bat)), (critic_t, (Wc1, bc1), (Wct, bct))):
        got = net_t.parameters()
        for k in range(2):
            for l in range(2):
                want = GC.fmaf(np.full(old[k][l].shape, tau, F32), new[k][l] - old[k][l], old[k][l]).reshape(old[k][l].shape)
                assert np.array_equal(AC.bits(got[k][l]), AC.bits(want)), ('polyak', k, l)
    actor_t.close()
    critic_t.close()
    env.close()
    return worst


def case_host_value_errors(library):
    """the faces refuse a chunk_rows that is no even integer >= 2 on the host, naming it, before anything reaches the library"""
    import pytest
    env = AC.stepped(library, 'reach', 8)
    try:
        critic = env.critic
        critic.load(*GC.net(802, (9, 33, 1)))
        x, act = np.zeros((8, 6), F32), np.zeros((8, 3), F32)
        for bad in (0, 1, 3, -2, 2.0, '4', True):
            for call in (lambda: critic.grad(x, act, chunk_rows=bad), lambda: critic.grad_work_floats(8, bad), lambda: critic.grad(x, act, grads=None, chunk_rows=bad),
                         lambda: critic.grad_device(8, 16, 6, 16, 0, d_a=16, a_dim=3, chunk_rows=bad)):
                with pytest.raises(ValueError, match='chunk_rows'):
                    call()
        assert critic.grad_work_floats(8, None) == critic.grad_work_floats(8) == critic.grad_work_floats(8, 8)
        assert critic.grad_work_floats(8, 2) > critic.grad_work_floats(8)
        assert critic.grad(x[:0], act[:0], chunk_rows=2)['gx'].shape == (0, 6)
        got, ref = critic.grad(x + 1, act, chunk_rows=np.int64(4)), critic.grad(x + 1, act, chunk_rows=4)
        assert all(np.array_equal(u, v) for u, v in zip(got['dW'], ref['dW']))
    finally:
        env.close()


# ----------------------------------------------------------------------------------------------------------------------
def wave_order_run(library):
    """what tests/test_grad_chunk_wave_order.py runs under every wavefront order -> dict of arrays"""
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for name, (widths, Dx, B, R) in {'small': ((9, 33, 1), 6, 33, 16), 'wide': ((6, 256, 256, 3), 6, 33, 2), 'odd': ((33, 255, 31, 2), 29, 101, 34)}.items():
            c = GC.grad_case(widths, Dx, B, head='target', out_act=1)
            got = run_case(h, c, R, 1)
            for k in ('gx', 'ga', 'out'):
                if got[k] is not None:
                    res[name + k] = got[k]
            for l, (w, b) in enumerate(zip(got['dW'], got['db'])):
                res['%sdW%d' % (name, l)], res['%sdb%d' % (name, l)] = w, b
    return res
