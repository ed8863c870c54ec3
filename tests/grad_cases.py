"""The cases of the back-propagation / Adam / Polyak tests (include/pmg.h pmg_mlp_grad_device, pmg_mlp_adam_device, pmg_mlp_polyak_device;
DESIGN.md 3.11) and their numpy model, shared by tests/test_grad_emulated.py (the g++ build of the product sources over the fiber
emulator), tests/test_gpu_grad.py (libpmg_hip.so on the MI355X), tests/test_grad_host.py (the numpy faces, and the model against
torch.autograd) and tests/test_grad_wave_order.py.  The model stands on tests/actor_cases.py's exact float32 fmaf; every device case takes
the loaded library and goes through the C ABI with buffers from pmg_device_alloc.

Bars.  Every gradient is a float32 fmaf chain in a stated order, the head is a subtract and a multiply, the mask a select: with an identity
output dW, db, gx, ga and out are compared bit for bit with the model (eq_val: zeros by value, a padding product may turn -0 into +0).
With a tanh output, out is the float32 library tanh: it is held to the float64 tanh of the model's bit-exact z within
actor_cases.ACTION_TOL, and everything else is bit-equal to the model evaluated from the DEVICE's own out.  Adam's m and v and Polyak are
bit-exact; Adam's p goes through the build's sqrtf and division: it is held to the float64 step evaluated from the bit-exact m and v
within ADAM_TOL of the size of that step."""
import ctypes as C

import numpy as np

import actor_cases as AC
from actor_cases import ACTION_TOL, POISON, Net, fmaf
from normalizer_cases import SENTINEL, Dev, handle
from pybullet_multigoal_gym_amd._lib import PmgAdam, PmgMlp, PmgMlpGrad, PmgMlpParams
from td_cases import Out, cached, put_rows

E_INVALID = -1
TILE = AC.TILE
BATCHES = (1, 31, 32, 33, 101)
CAT_DX, CAT_A = (1, 6, 31, 33), (1, 3, 4)
HIDDEN = ((33,), (256, 256, 256))
F32 = np.float32
INF = float('inf')

# The model against float64 autograd (test 1): max|g32 - g64| / max|g64| per tensor (dW, db, gx) of the float32 CHAIN model over the four
# networks x B = 33, 101 x seeds MODEL_SEEDS, with equal float32 and float64 ReLU masks every time, measured on the CPU:
#   9-256-256-256-1: 2.79e-6   6-256-256-256-3 tanh: 1.17e-6   33-33-4: 4.17e-7   5-1: 4.96e-7      (the largest: 2.79e-6)
# against 1.84e-6 / 9.14e-7 / 3.14e-7 / 2.86e-7 for torch's own float32 in place of the chain: a serial chain of 256 terms rounds a little
# more than torch's blocked sums.  The bar is 4 x the largest, the headroom ACTION_TOL gives.  A MEASURED value above 1e-5 would mean the
# model is wrong, not that the bar is tight.
MODEL_WORST = 2.79e-6
assert MODEL_WORST < 1e-5
MODEL_TOL = 4 * MODEL_WORST
MODEL_NETS = (((9, 256, 256, 256, 1), 0), ((6, 256, 256, 256, 3), 1), ((33, 33, 4), 0), ((5, 1), 0))
MODEL_SEEDS = (1, 2, 3)

# Adam's step (test 7): largest |p - p64| / |step64| over case_adam, p64 = p - step64 in float64 from the bit-exact m and v: 8.47e-5 on
# the emulator and 8.47e-5 on the MI355X.  On the emulator the figure comes from a parameter of -0.408 with a step of
# 1.74e-4: the error, 1.47e-8, is the half ulp of that parameter (1.49e-8) -- the rounding of p itself, not the step's sqrtf or division,
# sets it.  The bar is 4 x the larger.  A wrong element or a wrong t moves p by the whole step: a ratio of the order of 1.
ADAM_WORST = 8.47e-5
ADAM_TOL = 4 * ADAM_WORST


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def net(seed, widths, bias=True):
    """weights uniform in +-1 / sqrt(K), biases in +-0.5 (None without bias)"""
    rs = np.random.RandomState(seed)
    Ws = [(rs.uniform(-1, 1, (widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(F32) for l in range(len(widths) - 1)]
    bs = [rs.uniform(-0.5, 0.5, widths[l + 1]).astype(F32) for l in range(len(widths) - 1)] if bias else None
    return Ws, bs


def forward_saved(x, Ws, bs):
    """the chain of actor_cases.forward, keeping every layer's input -> hs [L] (hs[0] = x), z [B, width[L]]"""
    h = np.asarray(x, F32)
    hs = []
    for l, W in enumerate(Ws):
        hs.append(h)
        b = bs[l] if bs is not None and bs[l] is not None else np.zeros(W.shape[0], F32)
        acc = np.broadcast_to(b.astype(F32), (h.shape[0], W.shape[0])).copy()
        for k in range(W.shape[1]):
            acc = fmaf(h[:, k:k + 1], W[None, :, k], acc).reshape(acc.shape)
        z, h = acc, np.maximum(acc, F32(0))
    return hs, z


def head_of(o, gout=None, target=None, gscale=1.0):
    if gout is not None:
        return np.asarray(gout, F32)
    if target is not None:
        return F32(gscale) * (o - np.asarray(target, F32))                       # two roundings
    return np.full(o.shape, gscale, F32)


def backward(hs, Ws, bs, delta, weights=True):
    """the normative backward from delta_{L-1} -> dW [L], db [L], s_0 [B, width[0]]"""
    L, B = len(Ws), delta.shape[0]
    dW, db = [None] * L, [None] * L
    with np.errstate(over='ignore', invalid='ignore'):
        for l in range(L - 1, -1, -1):
            W, h = Ws[l], hs[l]
            if weights:
                acc, sb = np.zeros(W.shape, F32), np.zeros(W.shape[0], F32)
                for b in range(B):
                    acc = fmaf(delta[b][:, None], h[b][None, :], acc).reshape(W.shape)
                    sb = sb + delta[b]
                dW[l] = acc
                db[l] = sb if bs is not None and bs[l] is not None else None
            s = np.zeros(h.shape, F32)
            for j in range(W.shape[0]):
                s = fmaf(delta[:, j:j + 1], W[j][None, :], s).reshape(h.shape)
            delta = np.where(h > 0, s, F32(0)) if l else s
    return dW, db, delta


def model(x, Ws, bs, out_act=0, gout=None, target=None, gscale=1.0, out=None, a=None, weights=True):
    """-> dict(z, out, dW, db, gx, ga, masks).  x | a are the rows; with a tanh output `out` is the device's own out (or the float32 numpy
    tanh when none is given)."""
    rows = np.asarray(x, F32) if a is None else np.concatenate([x, a], 1).astype(F32)
    with np.errstate(over='ignore', invalid='ignore'):
        hs, z = forward_saved(rows, Ws, bs)
        o = z if not out_act else (np.tanh(z).astype(F32) if out is None else np.asarray(out, F32))
        g = head_of(o, gout, target, gscale)
        delta = (g * fmaf(-o, o, np.ones(o.shape, F32)).reshape(o.shape)) if out_act else g
        dW, db, s0 = backward(hs, Ws, bs, delta.astype(F32), weights)
    Dx = x.shape[1]
    return {'z': z, 'out': o, 'dW': dW, 'db': db, 'gx': np.ascontiguousarray(s0[:, :Dx]), 'ga': None if a is None else np.ascontiguousarray(s0[:, Dx:]),
            'masks': [h > 0 for h in hs[1:]]}


def eq_val(got, want, label):
    """bit for bit, zeros by value (+0.0 is added to both sides); NaNs must sit in the same places with the same bits"""
    got, want = np.asarray(got, F32) + F32(0), np.asarray(want, F32) + F32(0)
    gb, wb = AC.bits(got), AC.bits(want)
    assert got.shape == want.shape and np.array_equal(gb, wb), (label, np.argwhere(gb != wb)[:4].tolist(), got[gb != wb][:4], want[gb != wb][:4])


def check(got, want, label, keys=('dW', 'db', 'gx', 'ga', 'out')):
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
def rows_out(dev, B, W, pad, shift):
    return Out(dev, 4 * (B * (W + pad)), 4 * shift)


def read_rows(out, B, W, pad, written=True):
    if not written:
        out.read(written=False)
        return None
    raw = out.read(np.uint8).reshape(B, 4 * (W + pad))
    assert (raw[:, 4 * W:] == SENTINEL).all(), 'the padding between output rows was written'
    return np.ascontiguousarray(raw[:, :4 * W]).view(F32)


class Params:
    """canary-framed tensors shaped like a network, pre-filled with sentinel bytes, tensor k at phase (shift + k) & 3"""

    def __init__(self, h, dev, Ws, bs, shift=0, fill=None):
        self.shapes = [(W.shape, None if bs is None or bs[l] is None else bs[l].shape) for l, W in enumerate(Ws)]
        self.w, self.b = [], []
        k = shift
        for ws, bshape in self.shapes:
            self.w.append(Out(dev, 4 * int(np.prod(ws)), 4 * (k & 3)))
            self.b.append(None if bshape is None else Out(dev, 4 * bshape[0], 4 * ((k + 1) & 3)))
            k += 2
        self.struct = h.params_struct([o.ptr for o in self.w], [None if o is None else o.ptr for o in self.b])
        if fill is not None:
            for l, W in enumerate(fill[0]):
                h.upload(self.w[l].ptr, np.ascontiguousarray(W, F32))
                if self.b[l] is not None:
                    h.upload(self.b[l].ptr, np.ascontiguousarray(fill[1][l], F32))

    def read(self, written=True):
        W = [o.read(written=written) for o in self.w]
        b = [None if o is None else o.read(written=written) for o in self.b]
        if not written:
            return None, None
        return [w.reshape(s[0]) for w, s in zip(W, self.shapes)], b


def device_grad(h, Ws, bs, x, a=None, out_act=0, gout=None, target=None, gscale=1.0, grads=True, null=(), pad=0, shift=0, twice=False):
    """pmg_mlp_grad_device on canary-framed, sentinel-filled outputs -> dict(dW, db, gx, ga, out) (None for what was passed as NULL).
    pad: floats of poison behind every input row and of sentinel between output rows; shift: the phase of the first float pointer, the
    others follow in turn; the workspace is sized exactly.  twice: the call is issued a second time on the same buffers."""
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
        work = h.mlp_grad_work_floats(n.mlp, B)
        assert work >= 0
        o_work = Out(dev, 4 * work, 4 * (shift & 3))
        use_ga = Da > 0 and 'ga' not in null
        g = h.grad_struct(B, d_x, xs, Dx, o_work.ptr, work, d_a, as_, Da, d_go, gos, d_t, ts, gscale, par.struct if grads else None,
                          None if 'gx' in null else o_gx.ptr, Dx + pad, o_ga.ptr if use_ga else None, Da + pad if use_ga else 0,
                          None if 'out' in null else o_out.ptr, A + pad)
        for _ in range(2 if twice else 1):
            h.mlp_grad_device(n.mlp, g)
        h.sync()
        o_work.read(np.uint8)
        dW, db = par.read(written=grads)
        return {'dW': dW, 'db': db, 'gx': read_rows(o_gx, B, Dx, pad, 'gx' not in null), 'ga': read_rows(o_ga, B, max(Da, 1), pad, use_ga),
                'out': read_rows(o_out, B, A, pad, 'out' not in null)}


# ----------------------------------------------------------------------------------------------------------------------
# 1. the model is the gradient (CPU only: tests/test_grad_host.py)
def model_vs_autograd(widths, out_act, B, seed):
    """-> (largest max|g32 - g64| / max|g64| over dW, db, gx of the chain model, the same for torch's own float32, masks equal)"""
    import torch
    Ws, bs = net(seed, widths)
    rs = np.random.RandomState(seed + 77)
    x = rs.uniform(-1, 1, (B, widths[0])).astype(F32)
    g = rs.uniform(-1.0 / B, 1.0 / B, (B, widths[-1])).astype(F32)
    m = model(x, Ws, bs, out_act, gout=g)

    def autograd(dtype):
        tW = [torch.tensor(W, dtype=dtype, requires_grad=True) for W in Ws]
        tb = [torch.tensor(b, dtype=dtype, requires_grad=True) for b in bs]
        tx = torch.tensor(x, dtype=dtype, requires_grad=True)
        h, masks = tx, []
        for l in range(len(tW)):
            z = h @ tW[l].T + tb[l]
            if l + 1 < len(tW):
                masks.append((z > 0).numpy())
                h = torch.relu(z)
        o = torch.tanh(z) if out_act else z
        (o * torch.tensor(g, dtype=dtype)).sum().backward()
        return [t.grad.numpy().astype(np.float64) for t in tW], [t.grad.numpy().astype(np.float64) for t in tb], tx.grad.numpy().astype(np.float64), masks
    W64, b64, x64, masks64 = autograd(torch.float64)
    W32, b32, x32, _ = autograd(torch.float32)
    same = all(np.array_equal(a, b) for a, b in zip(m['masks'], masks64))

    def worst(dW, db, gx):
        return max(float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()) for a, b in zip(list(dW) + list(db) + [gx], W64 + b64 + [x64]))
    return worst(m['dW'], m['db'], m['gx']), worst(W32, b32, x32), same


# ----------------------------------------------------------------------------------------------------------------------
# 2. bit-exact gradients
def grad_case(widths, Dx, B, bias=True, out_act=0, head='target', seed=None):
    """a network of `widths` on B rows x | a (Dx of the width[0] columns are x; Dx == width[0]: raw rows) with its model"""
    def make():
        s = (seed if seed is not None else 1000 + 31 * widths[0] + 7 * len(widths) + widths[-1] + Dx)
        Ws, bs = net(s, widths, bias)
        rs = np.random.RandomState(s + B)
        rows = rs.uniform(-2, 2, (B, widths[0])).astype(F32)
        x, a = np.ascontiguousarray(rows[:, :Dx]), (np.ascontiguousarray(rows[:, Dx:]) if Dx < widths[0] else None)
        A = widths[-1]
        kw = {'gscale': 2.0 / B}
        if head == 'target':
            kw['target'] = rs.uniform(-1, 1, (B, A)).astype(F32)
        elif head == 'gout':
            kw = {'gout': rs.uniform(-1.0 / B, 1.0 / B, (B, A)).astype(F32)}
        else:
            kw = {'gscale': -1.0 / B}
        return dict(Ws=Ws, bs=bs, x=x, a=a, kw=kw, out_act=out_act, m=None if out_act else model(x, Ws, bs, 0, a=a, **kw))
    return cached(('grad', tuple(widths), Dx, B, bias, out_act, head, seed), make)


def run_case(h, c, n=0, **kw):
    return device_grad(h, c['Ws'], c['bs'], c['x'], c['a'], c['out_act'], pad=n % 3, shift=n % 4, **dict(c['kw'], **kw))


def cat_cases(hidden):
    """Dx x A cat rows into a critic, the batches in turn (the largest network takes the batches up to 33: the model's cost is its B)"""
    out, n = [], HIDDEN.index(hidden)
    for Dx in CAT_DX:
        for A in CAT_A:
            B = BATCHES[n % (len(BATCHES) if len(hidden) == 1 else 4)]
            n += 1
            out.append(((Dx + A,) + hidden + (1,), Dx, B))
    return out


RAW_CASES = [((Dx, 33, A), Dx, BATCHES[(i + 2) % 5]) for i, (Dx, A) in enumerate((Dx, A) for Dx in CAT_DX for A in CAT_A)] + \
            [((6, 256, 256, 256, 3), 6, 33), ((33, 256, 256, 256, 4), 33, 31)]
EXTREME_CASES = [((5, 1), 5, 33), ((5, 1), 2, 101), ((1, 1), 1, 1), ((256, 256), 256, 33), ((3, 1, 1, 2), 3, 33), ((6, 33, 1, 33, 3), 6, 101),
                 ((2, 1, 1, 1, 1), 1, 32), ((256, 33, 1), 252, 33), ((256, 33, 1), 1, 31), ((256, 31, 32, 2), 128, 32), ((31, 255, 2), 31, 33)]


def case_bit_exact(library, cases, heads=('target', 'gout', 'const')):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, Dx, B) in enumerate(cases):
            c = grad_case(widths, Dx, B, bias=n % 4 != 3, head=heads[n % len(heads)])
            check(run_case(h, c, n), c['m'], (widths, Dx, B))


def case_every_batch(library):
    """every batch size on one shape per hidden width, against the model of that batch"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for widths, Dx in (((9, 33, 1), 6), ((10, 256, 256, 256, 1), 6)):
            for n, B in enumerate(BATCHES if len(widths) == 3 else BATCHES[:4]):
                c = grad_case(widths, Dx, B)
                check(run_case(h, c, n + 1), c['m'], (widths, B))


def case_tanh(library):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, Dx, B) in enumerate((((6, 33, 3), 6, 33), ((6, 256, 256, 256, 3), 6, 32), ((9, 33, 1), 6, 101), ((5, 4), 5, 31))):
            for head in ('gout', 'target', 'const'):
                c = grad_case(widths, Dx, B, out_act=1, head=head)
                got = run_case(h, c, n)
                z = forward_saved(c['x'] if c['a'] is None else np.concatenate([c['x'], c['a']], 1), c['Ws'], c['bs'])[1]
                err = float(np.abs(got['out'] - np.tanh(z.astype(np.float64))).max())
                worst = max(worst, err)
                assert err <= ACTION_TOL, (widths, head, err)
                check(got, model(c['x'], c['Ws'], c['bs'], 1, a=c['a'], out=got['out'], **c['kw']), (widths, head, 'from the device out'), ('dW', 'db', 'gx', 'ga'))
    print('tanh output: largest |out - tanh64(z)| = %.3g (bar %.3g)' % (worst, ACTION_TOL))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# 3. lane maps name themselves
def case_lane_maps(library):
    """Exact integers on a one-layer identity network J <- K.  Transposed step: W[j][k] = j K + k and delta one-hot at (b, j = b % J) through
    d_gout: gx[b][k] = (b % J) K + k names the row and the column of W a lane read; then delta with ones in a whole residue class of j, whose
    exact sums name the columns.  Weights step: the same one-hot delta against integer rows h[b][k] = b K + k + 1: dW[j][k] is the sum of the
    rows b with b % J == j and db[j] their count.  Everything is below 2^24, so a swapped A / B / C map of either step returns another
    integer.  J and K of 256 cover both strips of every wavefront (units w and w + 4)."""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for J, K, B in ((256, 256, 64), (33, 255, 33), (255, 33, 64), (1, 256, 3), (256, 1, 33)):
            W = (np.arange(J, dtype=np.float64)[:, None] * K + np.arange(K)[None, :]).astype(F32)
            b = np.arange(B)
            delta = np.zeros((B, J), F32)
            delta[b, b % J] = 1
            x = (b[:, None] * K + np.arange(K)[None, :] + 1).astype(F32)
            assert x.max() < 2 ** 24 and W.max() < 2 ** 24
            got = device_grad(h, [W], [np.zeros(J, F32)], x, gout=delta, pad=1, shift=1)
            assert np.array_equal(got['gx'], W[b % J]), (J, K, 'gx: one-hot rows of delta against W')
            want = np.zeros((J, K), F32)
            cnt = np.zeros(J, F32)
            for r in b:
                want[r % J] += x[r]
                cnt[r % J] += 1
            assert want.max() < 2 ** 24
            assert np.array_equal(got['dW'][0], want), (J, K, 'dW: one-hot delta against integer h')
            assert np.array_equal(got['db'][0], cnt), (J, K, 'db')
            # one-hot columns: row b carries delta[b][j] = 1 for EVERY j of one residue class: gx[b][k] = sum of those rows of W (exact)
            jj = np.arange(J)
            delta = (jj[None, :] % 8 == (b % 8)[:, None]).astype(F32)
            want = delta.astype(np.float64) @ W.astype(np.float64)
            if want.max() < 2 ** 24:
                got = device_grad(h, [W], None, x, gout=delta, grads=False, shift=2)
                assert np.array_equal(got['gx'].astype(np.float64), want), (J, K, 'gx: columns')


# ----------------------------------------------------------------------------------------------------------------------
# 4. heads
def case_heads(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for widths, Dx, B in (((9, 33, 1), 6, 33), ((6, 33, 3), 6, 101)):
            c = grad_case(widths, Dx, B, head='target')
            m = c['m']
            full = run_case(h, c, 1)
            check(full, m, (widths, 'target'))
            # the d_gout form fed gscale (o - target) from the model: the same bits as the d_target form
            g = head_of(m['out'], target=c['kw']['target'], gscale=c['kw']['gscale'])
            via = device_grad(h, c['Ws'], c['bs'], c['x'], c['a'], gout=g, pad=2, shift=3)
            check(via, full, (widths, 'gout == target form'))
            # the constant: the d_gout form fed a constant table
            const = device_grad(h, c['Ws'], c['bs'], c['x'], c['a'], gscale=-1.0 / B, shift=2)
            check(const, device_grad(h, c['Ws'], c['bs'], c['x'], c['a'], gout=np.full((B, widths[-1]), -1.0 / B, F32), gscale=123.0), (widths, 'const == gout form'))
            check(const, model(c['x'], c['Ws'], c['bs'], a=c['a'], gscale=-1.0 / B), (widths, 'const'))
            # grads == NULL leaves no trace but gx / ga (and out when asked for); every optional output NULL in turn
            for null in (('out',), ('gx',), ('ga',), ('gx', 'out'), ('gx', 'ga')):
                if set(null) >= ({'gx', 'out'} if c['a'] is None else {'gx', 'ga', 'out'}):
                    continue                                                 # nothing left to compute: an invalid call (case 9)
                got = run_case(h, c, 2, grads=False, null=null)
                assert got['dW'] is None and got['db'] is None
                check(got, m, (widths, 'grads NULL', null))
            got = run_case(h, c, 3, null=('gx', 'ga', 'out'))
            check(got, m, (widths, 'grads alone'))


# ----------------------------------------------------------------------------------------------------------------------
# 5. stale tile and masks
def stale_case(regime, B):
    """Dx = 29, A = 4 cat rows (33 inputs, odd), hidden 256 then a narrow layer, one output.
      'huge': 33 -> 256 -> 3 -> 1.  Layer 0 has weights of 1e30 on inputs in [0.5, 2): hidden activations of some 1e31 that fill the tile's
              columns 0..255; layer 1 (1e-30) brings them back to the hundreds.  The backward of layer 2 reads delta_2 in column 0 and the padding
              column 1, the backward of layer 1 reads delta_1 in columns 0..2 and the padding column 3: both held 1e31 when the backward began.
      'inf':  33 -> 256 -> 33 -> 1 with inputs of 1e9: h_1 is inf everywhere.  Layer 1 has NEGATIVE weights: z_1 = -inf, h_2 = +0.0, every unit of
              h_2 is masked, so delta_1 is a real +0.0 everywhere although s_2 = delta_2 W_2 is not; dW_2 = delta_2 h_2 = 0, dW_1 = delta_1 h_1
              would be 0 * inf = NaN -- that IS the normative value of a chain over an inf activation and the model says the same --, so this
              regime is asked for input gradients and out only (grads NULL), where a masked unit's s is never multiplied: gx and ga hold +0.0,
              no NaN."""
    def make():
        rs = np.random.RandomState(190 + B)
        Dx, A = 29, 4
        if regime == 'huge':
            rows = rs.uniform(0.5, 2, (B, Dx + A)).astype(F32)
            Ws = [np.full((256, Dx + A), 1e30, F32), (rs.uniform(0.5, 1, (3, 256)) * np.array([[1], [-1], [1]]) * 1e-30).astype(F32), rs.uniform(0.5, 1, (1, 3)).astype(F32)]   # unit 1 of h_2 is off
            bs = [None, rs.uniform(-0.5, 0.5, 3).astype(F32), rs.uniform(-0.5, 0.5, 1).astype(F32)]
        else:
            rows = (rs.uniform(0.5, 2, (B, Dx + A)) * 1e9).astype(F32)
            Ws = [np.full((256, Dx + A), 1e30, F32), -rs.uniform(0.5, 1, (33, 256)).astype(F32), rs.uniform(-1, 1, (1, 33)).astype(F32)]
            bs = [None, None, rs.uniform(-0.9, 0.9, 1).astype(F32)]
        x, a = np.ascontiguousarray(rows[:, :Dx]), np.ascontiguousarray(rows[:, Dx:])
        m = model(x, Ws, bs, a=a, gscale=-1.0 / B, weights=regime == 'huge')
        hid = np.maximum(forward_saved(rows, Ws[:1], None)[1], 0)
        assert np.isinf(hid).all() if regime == 'inf' else (np.isfinite(hid).all() and hid.min() > 1e30)
        for k in ('gx', 'ga', 'out'):
            assert np.isfinite(m[k]).all(), (regime, k)
        if regime == 'huge':
            assert all(np.isfinite(t).all() for t in m['dW']) and m['masks'][1].any() and not m['masks'][1].all() and np.abs(m['gx']).max() > 0
        return dict(Ws=Ws, bs=bs, x=x, a=a, m=m)
    return cached(('grad stale', regime, B), make)


def case_stale_tile(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for regime in ('huge', 'inf'):
            for B in (TILE, TILE + 1):
                c = stale_case(regime, B)
                got = device_grad(h, c['Ws'], c['bs'], c['x'], c['a'], gscale=-1.0 / B, grads=regime == 'huge', pad=1)
                for k in ('gx', 'ga', 'out'):
                    assert np.isfinite(got[k]).all(), (regime, B, k, 'NaN or inf')
                check(got, c['m'], (regime, B))
        # a unit whose z is exactly 0 has mask 0: 2 -> 2 -> 1, unit 0 of the hidden layer is x0 - x1 on rows with x0 == x1
        Ws, bs = [np.array([[1, -1], [1, 1]], F32), np.array([[3, 5]], F32)], None
        x = np.array([[1, 1], [2, 1], [-3, -3], [0.5, 0.25]], F32)
        got = device_grad(h, Ws, bs, x, gscale=1.0)
        assert np.array_equal(got['gx'], np.array([[5, 5], [8, 2], [0, 0], [8, 2]], F32)), got['gx']
        check(got, model(x, Ws, bs, gscale=1.0), 'z == 0')
        # a masked unit whose s is inf: 2 -> 2 -> 1, unit 0 is off (z < 0) and s_1[.][0] = 1e10 * 1e30 = inf: delta_0[.][0] is a real +0.0,
        # where a product with a zero mask would be NaN
        Ws, bs = [np.array([[-1, 0], [0, 1]], F32), np.array([[1e30, 2]], F32)], None
        x = np.array([[1, 1], [2, 3]], F32)
        got = device_grad(h, Ws, bs, x, gscale=1e10)
        assert np.array_equal(got['gx'], np.array([[0, 2e10], [0, 2e10]], F32)), got['gx']
        with np.errstate(over='ignore'):
            check(got, model(x, Ws, bs, gscale=1e10), 'masked inf')


# ----------------------------------------------------------------------------------------------------------------------
# 6. order and independence
def case_independence(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for widths, Dx in (((9, 33, 1), 6), ((10, 256, 256, 256, 1), 6)):
            c = grad_case(widths, Dx, 101, head='gout')
            big = run_case(h, c, 1, grads=len(widths) == 3)
            sub = device_grad(h, c['Ws'], c['bs'], c['x'][:33], c['a'][:33], gout=c['kw']['gout'][:33], pad=2, shift=2, grads=False)
            for k in ('gx', 'ga', 'out'):
                assert np.array_equal(AC.bits(sub[k]), AC.bits(big[k][:33])), (widths, k, 'a row depends on its batch')
            again = run_case(h, c, 1, grads=len(widths) == 3, twice=True)
            for k in ('gx', 'ga', 'out'):
                assert np.array_equal(AC.bits(again[k]), AC.bits(big[k])), (widths, k, 'two calls differ')
            if big['dW'] is not None:
                for a, b in zip(big['dW'] + big['db'], again['dW'] + again['db']):
                    assert np.array_equal(AC.bits(a), AC.bits(b)), (widths, 'two calls differ in dW / db')
            # dW depends on the row order: the reversed batch is another chain
            if big['dW'] is not None:
                rev = device_grad(h, c['Ws'], c['bs'], c['x'][::-1].copy(), c['a'][::-1].copy(), gout=c['kw']['gout'][::-1].copy())
                assert np.array_equal(AC.bits(rev['gx'][::-1]), AC.bits(big['gx']))
                assert any(not np.array_equal(AC.bits(a), AC.bits(b)) for a, b in zip(rev['dW'], big['dW']))


def wave_order_run(library):
    """what tests/test_grad_wave_order.py runs under every wavefront order -> dict of arrays"""
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for name, (widths, Dx, B, act) in {'small': ((9, 33, 1), 6, 33, 0), 'wide': ((6, 256, 256, 3), 6, 33, 1), 'odd': ((33, 255, 31, 2), 29, 32, 0)}.items():
            c = grad_case(widths, Dx, B, out_act=act, head='target')
            got = run_case(h, c, 1)
            for k in ('gx', 'ga', 'out'):
                if got[k] is not None:
                    res[name + k] = got[k]
            for l, (w, b) in enumerate(zip(got['dW'], got['db'])):
                res['%sdW%d' % (name, l)], res['%sdb%d' % (name, l)] = w, b
    return res


# ----------------------------------------------------------------------------------------------------------------------
# 7. Adam / Polyak
ADAM_SHAPES = (((1, 1), False), ((5, 51), False), ((16, 16), False), ((256, 256), False), ((6, 33, 3), True), ((9, 256, 256, 256, 1), True))


def adam_model(p, g, m, v, lr, beta1, beta2, eps, t):
    """-> m, v float32 (bit-exact model), p64 and step64 (float64, from those m and v and the float32 factors the host passes)"""
    b1, b2 = F32(beta1), F32(beta2)
    omb1, omb2 = F32(1.0 - float(b1)), F32(1.0 - float(b2))
    step_size = float(F32(float(F32(lr)) / (1.0 - float(b1) ** t)))
    rsc2 = float(F32(1.0 / np.sqrt(1.0 - float(b2) ** t)))
    m1 = fmaf(np.full(m.shape, b1, F32), m, omb1 * g).reshape(m.shape)
    v1 = fmaf(np.full(v.shape, b2, F32), v, omb2 * (g * g)).reshape(v.shape)
    step = step_size * (m1.astype(np.float64) / (np.sqrt(v1.astype(np.float64)) * rsc2 + float(F32(eps))))
    return m1, v1, p.astype(np.float64) - step, step


def adam_error(p, p64, step, label):
    """-> largest |p - p64| / |step| where the step is not zero; where it is zero p must not have moved"""
    zero = step == 0
    assert np.array_equal(p[zero].astype(np.float64), p64[zero]), (label, 'a parameter moved without a step')
    return float((np.abs(p.astype(np.float64) - p64)[~zero] / np.abs(step[~zero])).max()) if (~zero).any() else 0.0


def case_adam(library, shapes=ADAM_SHAPES):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, bias) in enumerate(shapes):
            Ws, bs = net(40 + n, widths, bias)
            rs = np.random.RandomState(50 + n)

            def like(lo, hi, sign):
                """magnitudes in [lo, hi) with the given signs: m and g agree in sign, so no step is small beside an ulp of its parameter"""
                mk = (lambda a: (rs.uniform(lo, hi, a.shape) * (sign[id(a)] if sign else 1)).astype(F32))
                return [mk(W) for W in Ws], None if bs is None else [mk(b) for b in bs]
            sign = {id(a): rs.choice([-1.0, 1.0], a.shape) for a in list(Ws) + list(bs or ())}
            for t, state in ((1, 'zero'), (1000, 'warm')):
                G, M, V = like(0.05, 0.15, sign), like(0.02, 0.08, sign), like(0.001, 0.01, None)
                if state == 'zero':
                    for T in (M, V):
                        for arrs in T:
                            for arr in arrs or ():
                                arr[...] = 0
                G[0][0].flat[::3] = 0                                    # g = 0 (with m = v = 0 at t = 1: no step at all)
                V[0][0].flat[1::5] = 0                                   # v = 0
                with Dev(h) as dev:
                    shape = Net(h, dev, Ws, bs, 0)
                    P, Gd, Md, Vd = (Params(h, dev, Ws, bs, k, fill=T) for k, T in enumerate(((Ws, bs), G, M, V)))
                    adam = h.adam_struct(1e-3, t, 0.9, 0.999, 1e-8)
                    h.mlp_adam_device(shape.mlp, P.struct, Gd.struct, Md.struct, Vd.struct, adam)
                    h.sync()
                    gp, gg, gm, gv = P.read(), Gd.read(), Md.read(), Vd.read()
                for k in range(2):
                    for l in range(len(Ws)):
                        if k and bs is None:
                            continue
                        p, g, m, v = ((Ws, bs)[k][l], G[k][l], M[k][l], V[k][l])
                        m1, v1, p64, step = adam_model(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, t)
                        label = (widths, t, 'wb'[k], l)
                        AC.check_z(gg[k][l], g, label + ('g was written',))
                        assert np.array_equal(AC.bits(gm[k][l]), AC.bits(m1)) and np.array_equal(AC.bits(gv[k][l]), AC.bits(v1)), label + ('m / v',)
                        err = adam_error(gp[k][l], p64, step, label)
                        worst = max(worst, err)
                        assert err <= ADAM_TOL, label + (err,)
    print('adam: largest |p - p64| / |step64| = %.3g (bar %.3g)' % (worst, ADAM_TOL))
    return worst


def case_polyak(library, shapes=ADAM_SHAPES):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, bias) in enumerate(shapes):
            Ws, bs = net(60 + n, widths, bias)
            Wt, bt = net(70 + n, widths, bias)
            for tau in (0.05, 0.0, 1.0):
                with Dev(h) as dev:
                    src = Net(h, dev, Ws, bs, 0)
                    T = Params(h, dev, Wt, bt, n + 1, fill=(Wt, bt))
                    h.mlp_polyak_device(src.mlp, T.struct, tau)
                    h.sync()
                    gw, gb = T.read()
                    sw = [dev.get(p, W.shape, F32) for p, W in zip(src.d_w, Ws)]
                for l in range(len(Ws)):
                    assert np.array_equal(sw[l], Ws[l]), 'the source was written'
                    for got, p, t in ((gw[l], Ws[l], Wt[l]),) + (((gb[l], bs[l], bt[l]),) if bias else ()):
                        want = fmaf(np.full(t.shape, tau, F32), p - t, t).reshape(t.shape)
                        assert np.array_equal(AC.bits(got), AC.bits(want)), (widths, tau, l)
                        if tau == 0.0:
                            assert np.array_equal(got, t)


# ----------------------------------------------------------------------------------------------------------------------
# 8. one whole update through the faces
def case_whole_update(library):
    from pybullet_multigoal_gym_amd.actor import Actor
    from pybullet_multigoal_gym_amd.critic import Critic
    import td_cases as TC
    Dx, A, B, gamma, tau, lr = 6, 3, 33, 0.98, 0.05, 1e-3
    env = AC.stepped(library, 'reach', 8)
    actor, critic, actor_t, critic_t = env.actor, env.critic, Actor(env), Critic(env)
    Wa, ba = net(801, (Dx, 33, A))
    Wc, bc = net(802, (Dx + A, 33, 1))
    Wat, bat = net(803, (Dx, 33, A))
    Wct, bct = net(804, (Dx + A, 33, 1))
    actor.load(Wa, ba, out_activation='identity')
    actor_t.load(Wat, bat, out_activation='identity')
    critic.load(Wc, bc)
    critic_t.load(Wct, bct)
    rs = np.random.RandomState(805)
    x, xn = rs.uniform(-2, 2, (B, Dx)).astype(F32), rs.uniform(-2, 2, (B, Dx)).astype(F32)
    act, r = rs.uniform(-1, 1, (B, A)).astype(F32), -rs.randint(0, 2, B).astype(F32)
    sa, sc = actor.adam_state(), critic.adam_state()
    # critic: y, MSE gradient, Adam
    y, _, _ = critic_t.td_target(actor_t, xn, r, gamma, -1.0 / (1.0 - gamma), 0.0)
    TC.eq_y(y, TC.td_model(xn, r, Wat, bat, Wct, bct, gamma, -1.0 / (1.0 - gamma), 0.0)['y'], 'y')
    gc = critic.grad(x, act, target=y[:, None], gscale=2.0 / B)
    mc = model(x, Wc, bc, a=act, target=y[:, None], gscale=2.0 / B)
    check(gc, mc, 'critic gradient')
    critic.adam_step_device(gc, sc, lr)
    Wc1, bc1 = critic.parameters()
    worst = 0.0
    for got, p, g in [(Wc1[l], Wc[l], mc['dW'][l]) for l in range(2)] + [(bc1[l], bc[l], mc['db'][l]) for l in range(2)]:
        _, _, p64, step = adam_model(p, g, np.zeros_like(p), np.zeros_like(p), lr, 0.9, 0.999, 1e-8, 1)
        worst = max(worst, adam_error(got, p64, step, 'critic adam'))
    # actor: a = pi(x), dQ / da from the UPDATED critic with grads = None, back through the actor, Adam
    a_pi = actor.forward(x)
    eq_val(a_pi, AC.forward(x, Wa, ba), 'pi(x)')
    gq = critic.grad(x, a_pi, grads=None, gscale=-1.0 / B)
    assert gq['dW'] is None and gq['db'] is None
    check(gq, model(x, Wc1, bc1, a=a_pi, gscale=-1.0 / B, weights=False), 'dQ / da', ('gx', 'ga', 'out'))
    ga = actor.grad(x, gout=gq['ga'])
    ma = model(x, Wa, ba, gout=gq['ga'])
    check(ga, ma, 'actor gradient')
    actor.adam_step_device(ga, sa, lr)
    Wa1, ba1 = actor.parameters()
    for got, p, g in [(Wa1[l], Wa[l], ma['dW'][l]) for l in range(2)] + [(ba1[l], ba[l], ma['db'][l]) for l in range(2)]:
        _, _, p64, step = adam_model(p, g, np.zeros_like(p), np.zeros_like(p), lr, 0.9, 0.999, 1e-8, 1)
        worst = max(worst, adam_error(got, p64, step, 'actor adam'))
    assert worst <= ADAM_TOL, worst
    assert sa.t == 1 and sc.t == 1
    # targets: Polyak of the device's own parameters, bit for bit
    actor_t.soft_update_from(actor, tau)
    critic_t.soft_update_from(critic, tau)
    for net_t, new, old in ((actor_t, (Wa1, ba1), (Wat, bat)), (critic_t, (Wc1, bc1), (Wct, bct))):
        got = net_t.parameters()
        for k in range(2):
            for l in range(2):
                want = fmaf(np.full(old[k][l].shape, tau, F32), new[k][l] - old[k][l], old[k][l]).reshape(old[k][l].shape)
                assert np.array_equal(AC.bits(got[k][l]), AC.bits(want)), ('polyak', k, l)
    # the faces refuse what does not fit, and close() frees the states
    import pytest
    for bad in (lambda: critic.grad(x, act[:, :2]), lambda: critic.grad(x, act, gout=y[:, None], target=y[:, None]), lambda: actor.grad(x, gout=gq['ga'][:, :2]),
                lambda: actor.adam_step_device(gc, sa, lr), lambda: actor.adam_step_device(ga, sc, lr), lambda: actor.adam_step_device(ga, sa, lr, beta1=1.0),
                lambda: actor_t.soft_update_from(critic, tau), lambda: actor_t.soft_update_from(actor, 1.5), lambda: critic.grad(x, act, gscale=INF)):
        with pytest.raises(ValueError):
            bad()
    assert critic.grad(x[:0], act[:0])['gx'].shape == (0, Dx)
    actor_t.close()
    critic_t.close()
    env.close()
    assert sa.m is None and sc.g is None
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# 9. invalid calls
def case_invalid_calls(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        Dx, A, B = 6, 3, 8
        Wc, bc = net(91, (Dx + A, 16, 1))
        Wn, _ = net(92, (Dx + A, 16, 1), bias=False)
        vp = C.c_void_p
        nan = float('nan')
        with Dev(h) as dev:
            critic, nobias = Net(h, dev, Wc, bc, 0), Net(h, dev, Wn, None, 0)
            d_x, d_a, d_go = dev.put(np.zeros((B, Dx + A), F32)), dev.put(np.zeros((B, A), F32)), dev.put(np.zeros((B, 1), F32))
            NB = 2048
            outs = [dev.put(np.full(NB, SENTINEL, np.uint8)) for _ in range(9)]      # gx, ga, out, work, dW0, db0, dW1, db1, spare
            work = h.mlp_grad_work_floats(critic.mlp, B)
            assert 0 < 4 * work <= NB
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

            def grad(m=None, null_g=False, **kw):
                a = dict(batch=B, d_x=d_x, x_stride=Dx, x_dim=Dx, d_work=outs[3], work_floats=work, d_a=d_a, a_stride=A, a_dim=A, d_gout=None, gout_stride=1,
                         d_target=d_go, target_stride=1, gscale=0.25, grads=par, d_gx=outs[0], gx_stride=Dx, d_ga=outs[1], ga_stride=A, d_out=outs[2], out_stride=1)
                size = kw.pop('struct_size', None)
                a.update(kw)
                s = h.grad_struct(**a)
                if size is not None:
                    s.struct_size = size
                return h.L.lib.pmg_mlp_grad_device(h.h, C.byref(m or mlp(critic)), None if null_g else C.byref(s))

            def adam(shape=None, p=None, g=None, m=None, v=None, null_a=False, **kw):
                a = dict(lr=1e-3, step=1, beta1=0.9, beta2=0.999, eps=1e-8)
                size = kw.pop('struct_size', None)
                a.update(kw)
                s = h.adam_struct(**a)
                if size is not None:
                    s.struct_size = size
                ptr = lambda q: None if q is False else C.byref(q or par)
                return h.L.lib.pmg_mlp_adam_device(h.h, C.byref(shape or mlp(critic)), ptr(p), ptr(g), ptr(m), ptr(v), None if null_a else C.byref(s))

            def polyak(src=None, t=None, tau=0.05):
                return h.L.lib.pmg_mlp_polyak_device(h.h, C.byref(src or mlp(critic)), None if t is False else C.byref(t or par), C.c_float(tau))
            bad_nets = [mlp(critic, **kw) for kw in (dict(struct_size=C.sizeof(PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                                     dict(width=(1, 0)), dict(d_weight=(0, None)), dict(out_activation=2), dict(d_weight=(1, critic.d_w[1] + 2)))]
            bad = [lambda m=m: grad(m) for m in bad_nets] + [lambda m=m: adam(shape=m) for m in bad_nets] + [lambda m=m: polyak(src=m) for m in bad_nets] + [
                lambda: grad(null_g=True), lambda: grad(struct_size=C.sizeof(PmgMlpGrad) - 8), lambda: grad(struct_size=0),
                lambda: grad(d_x=None), lambda: grad(x_dim=0, a_dim=Dx + A), lambda: grad(d_a=None), lambda: grad(a_dim=0, x_dim=Dx + A),
                lambda: grad(d_a=None, a_dim=0, d_ga=None), lambda: grad(x_dim=Dx - 1), lambda: grad(a_dim=A + 1),
                lambda: grad(d_a=None, a_dim=0, x_dim=Dx + A, x_stride=Dx + A, gx_stride=Dx + A),            # d_ga without d_a
                lambda: grad(d_gout=d_go), lambda: grad(gscale=nan), lambda: grad(gscale=INF),
                lambda: grad(grads=None, d_gx=None, d_ga=None, d_out=None),
                lambda: grad(grads=params(d_weight=(1, None))), lambda: grad(grads=params(d_bias=(0, None))),
                lambda: grad(mlp(nobias)), lambda: grad(mlp(nobias), grads=params(d_bias=(0, None))),           # a bias gradient without a bias
                lambda: grad(d_work=None), lambda: grad(work_floats=work - 1), lambda: grad(work_floats=0),
                lambda: grad(d_x=d_x + 2), lambda: grad(d_a=d_a + 1), lambda: grad(d_target=d_go + 2), lambda: grad(d_target=None, d_gout=d_go + 1),
                lambda: grad(d_gx=outs[0] + 2), lambda: grad(d_ga=outs[1] + 1), lambda: grad(d_out=outs[2] + 3), lambda: grad(d_work=outs[3] + 2),
                lambda: grad(grads=params(d_weight=(0, outs[4] + 2))), lambda: grad(grads=params(d_bias=(1, outs[7] + 1))),
                lambda: grad(x_stride=Dx - 1), lambda: grad(a_stride=A - 1), lambda: grad(target_stride=0), lambda: grad(d_target=None, d_gout=d_go, gout_stride=0),
                lambda: grad(gx_stride=Dx - 1), lambda: grad(ga_stride=A - 1), lambda: grad(out_stride=0), lambda: grad(batch=-1),
                lambda: adam(p=False), lambda: adam(g=False), lambda: adam(m=False), lambda: adam(v=False), lambda: adam(null_a=True),
                lambda: adam(struct_size=C.sizeof(PmgAdam) - 8), lambda: adam(p=params(d_weight=(0, None))), lambda: adam(g=params(d_bias=(1, None))),
                lambda: adam(m=params(d_weight=(1, outs[6] + 2))), lambda: adam(v=params(d_bias=(0, outs[5] + 1))),
                lambda: adam(lr=nan), lambda: adam(lr=INF), lambda: adam(eps=nan), lambda: adam(eps=INF), lambda: adam(eps=-1e-8),
                lambda: adam(beta1=1.0), lambda: adam(beta1=-0.1), lambda: adam(beta1=nan), lambda: adam(beta2=1.0), lambda: adam(beta2=nan), lambda: adam(beta2=INF),
                lambda: adam(step=0), lambda: adam(step=-3),
                lambda: polyak(t=False), lambda: polyak(t=params(d_weight=(0, None))), lambda: polyak(t=params(d_bias=(1, outs[7] + 2))),
                lambda: polyak(tau=-0.01), lambda: polyak(tau=1.01), lambda: polyak(tau=nan)]
            assert h.L.lib.pmg_mlp_grad_device(h.h, None, C.byref(h.grad_struct(B, d_x, Dx, Dx, outs[3], work))) == E_INVALID
            assert h.L.lib.pmg_mlp_grad_work_floats(None, C.c_int64(B)) < 0 and h.mlp_grad_work_floats(critic.mlp, -1) < 0
            assert h.mlp_grad_work_floats(mlp(critic, width=(1, 257)), B) < 0 and h.mlp_grad_work_floats(mlp(critic, num_layers=5), B) < 0
            assert h.mlp_grad_work_floats(critic.mlp, 0) == 0

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
            # what is allowed: raw rows, a network without biases whose grads carry none, input gradients alone, an ignored extra bias pointer
            assert grad(d_a=None, a_dim=0, x_dim=Dx + A, x_stride=Dx + A, gx_stride=Dx + A, d_ga=None) == 0
            p_nb = params()
            p_nb.d_bias[0] = p_nb.d_bias[1] = None
            assert grad(mlp(nobias), grads=p_nb) == 0
            assert grad(grads=None, d_out=None, d_ga=None) == 0
            assert adam(shape=mlp(nobias)) == 0 and polyak(src=mlp(nobias)) == 0 and adam(eps=0.0, beta1=0.0, beta2=0.0) == 0 and polyak(tau=0.0) == 0 and polyak(tau=1.0) == 0
            h.sync()
