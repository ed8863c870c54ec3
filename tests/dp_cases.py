"""The cases of the data-parallel learner (include/pmg.h pmg_mlp_params_pack_device ... pmg_norm_update_env_ranks_device) and
their numpy model, shared by tests/test_dp_emulated.py (the g++ build of the product sources over the fiber emulator: ranks simulated as slots
in one process, and 2 and 4 real processes over the emulator's shared-memory collective), tests/test_gpu_dp.py (libpmg_hip.so on the MI355X:
simulated ranks and one-rank RCCL), tests/test_dp_host.py (every rejection) and tests/test_dp_wave_order.py.  Everything stands on
tests/grad_cases.py, tests/grad_chunk_cases.py and tests/normalizer_cases.py, which are imported and not edited.

The model.  A slot is one rank's gradient in the flat order weight 0, bias 0, weight 1, ...; the merge is rank_sum: float32 additions of the
slots in ascending rank order starting from slot 0 ITSELF -- IEEE additions, so every bit is defined, the sign of a zero included; a NaN must
sit where the model has one (its payload is the hardware's).  Equivalence: the merge of the gradients of the R slices of B_local rows is, zeros
compared by value, pmg_mlp_grad_chunked_device(chunk_rows = B_local) on the whole batch -- asked of the device's own chunked call on every
shape and of grad_chunk_cases.chunk_model on the small ones.  The normaliser's collective update is asked to leave the BITS of one unsharded
pmg_norm_update_device on the concatenated rows, which tests/normalizer_cases.py holds to its float64 bars."""
import ctypes as C
import os
import socket

import numpy as np

import actor_cases as AC
import grad_cases as GC
import grad_chunk_cases as CC
import normalizer_cases as NC
import policy_grad_cases as PC
import sac_pg_cases as SP
from actor_cases import Net
from grad_cases import F32, Params, eq_val
from normalizer_cases import SENTINEL, Dev, handle
from td_cases import Out, cached

E_INVALID, E_STATE = -1, -4
RANKS = (1, 2, 3, 8)
B_LOCALS = (2, 34)
# every width of {1, 2, 31, 32, 33, 255, 256} as an input, a hidden and an output width; one to four layers; raw and x | a rows; biases on
# every layer, on none, and on all but layer 1
NETS = (((1, 1), 1, 'all'), ((2, 31), 2, 'none'), ((32, 33, 255), 31, 'mixed'), ((256, 2, 1), 250, 'all'), ((33, 255, 31, 2), 29, 'mixed'),
        ((9, 32, 256, 33, 1), 6, 'all'), ((31, 1, 256, 2, 33), 31, 'mixed'), ((6, 256, 256, 3), 6, 'all'))
MODEL_PARAMS = 20000            # networks up to this many parameters are also held to grad_chunk_cases.chunk_model
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------------
# the numpy model
def rank_sum(slots):
    """slots [R, P] float32 -> ((slot 0 + slot 1) + slot 2) ... in float32, one rounding per addition, from slot 0 itself"""
    slots = np.asarray(slots, F32)
    acc = slots[0].copy()
    with np.errstate(over='ignore', invalid='ignore'):
        for r in range(1, slots.shape[0]):
            acc = (acc + slots[r]).astype(F32)
    return acc


def flatten(W, b):
    """the tensors of a network -> one flat array in the order of pmg_mlp_param_floats"""
    parts = []
    for l, w in enumerate(W):
        parts.append(np.asarray(w, F32).ravel())
        if b is not None and b[l] is not None:
            parts.append(np.asarray(b[l], F32).ravel())
    return np.concatenate(parts)


def unflatten(flat, Ws, bs):
    W, b, k = [], [], 0
    for l, w in enumerate(Ws):
        W.append(flat[k:k + w.size].reshape(w.shape))
        k += w.size
        keep = bs is not None and bs[l] is not None
        b.append(flat[k:k + w.shape[0]] if keep else None)
        k += w.shape[0] if keep else 0
    assert k == flat.size
    return W, b


def eq_bits(got, want, label):
    """every bit, the sign of a zero included; NaNs in the same places"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (label, 'NaNs sit elsewhere', np.argwhere(np.isnan(got) != nan)[:4].tolist())
    gb, wb = AC.bits(got)[~nan], AC.bits(want)[~nan]
    assert np.array_equal(gb, wb), (label, np.argwhere(gb != wb)[:4].tolist(), got[~nan][gb != wb][:4], want[~nan][gb != wb][:4])


def network(widths, bias, seed):
    Ws, bs = GC.net(seed, widths, bias != 'none')
    if bias == 'mixed':
        bs = [None if l == 1 else b for l, b in enumerate(bs)]
    return Ws, bs


def dp_case(widths, Dx, B, bias='all', head='target', seed=None):
    """a network and B rows x | a with a head, as grad_cases.grad_case makes them (gscale = ... / B, the GLOBAL batch)"""
    def make():
        s = seed if seed is not None else 3000 + 31 * widths[0] + 7 * len(widths) + widths[-1] + Dx
        Ws, bs = network(widths, bias, s)
        rs = np.random.RandomState(s + B)
        rows = rs.uniform(-2, 2, (B, widths[0])).astype(F32)
        x, a = np.ascontiguousarray(rows[:, :Dx]), (np.ascontiguousarray(rows[:, Dx:]) if Dx < widths[0] else None)
        A = widths[-1]
        if head == 'target':
            kw = {'gscale': 2.0 / B, 'target': rs.uniform(-1, 1, (B, A)).astype(F32)}
        elif head == 'gout':
            kw = {'gout': rs.uniform(-1.0 / B, 1.0 / B, (B, A)).astype(F32)}
        else:
            kw = {'gscale': -1.0 / B}
        return dict(Ws=Ws, bs=bs, x=x, a=a, kw=kw)
    return cached(('dp', tuple(widths), Dx, B, bias, head, seed), make)


def cut(c, s):
    """the rows s of a case: what one rank holds"""
    return dict(x=c['x'][s], a=None if c['a'] is None else c['a'][s], kw={k: (v[s] if isinstance(v, np.ndarray) else v) for k, v in c['kw'].items()})


# ----------------------------------------------------------------------------------------------------------------------
# device calls
class Slots:
    """nslots flat slots of P floats, `stride` floats apart, in ONE canary-framed buffer that ends with the last slot's last float; the
    floats between two slots are sentinel bytes that must survive"""

    def __init__(self, h, dev, nslots, P, extra=0, shift=0, fill=None):
        self.h, self.n, self.P, self.stride = h, nslots, P, P + extra
        self.out = Out(dev, 4 * ((nslots - 1) * self.stride + P), 4 * (shift & 3))
        self.ptr = self.out.ptr
        for r in range(nslots if fill is not None else 0):
            h.upload(self.at(r), np.ascontiguousarray(fill[r], F32))

    def at(self, r):
        return self.ptr + 4 * r * self.stride

    def read(self):
        raw = self.out.read(np.uint8)
        for r in range(self.n - 1):
            assert (raw[4 * (r * self.stride + self.P):4 * (r + 1) * self.stride] == SENTINEL).all(), 'the floats between two slots were written'
        return np.stack([raw[4 * r * self.stride:4 * (r * self.stride + self.P)].copy().view(F32) for r in range(self.n)])


def device_pack(h, dev, net, Ws, bs, dW, db, d_flat, shift=0):
    """pmg_mlp_params_pack_device of the tensors dW / db (uploaded to tensors of their own, each at another 4-byte phase) -> d_flat"""
    src = Params(h, dev, Ws, bs, shift, fill=(dW, db))
    h.mlp_params_pack_device(net.mlp, src.struct, d_flat)
    h.sync()
    got = src.read()                                                 # the source is not written, nor anything around it
    for u, v in zip(got[0] + got[1], list(dW) + list(db if db is not None else [None] * len(dW))):
        assert (u is None) == (v is None) and (u is None or np.array_equal(AC.bits(u), AC.bits(np.asarray(v, F32).reshape(u.shape))))


def device_pack_merge(h, Ws, bs, grads, extra=1, shift=0):
    """grads [R] of (dW, db): pack rank r's into slot r on the device, merge the slots -> (the slots as packed [R, P], merged dW, merged db)"""
    R = len(grads)
    with Dev(h) as dev:
        net = Net(h, dev, Ws, bs, 0)
        P = h.mlp_param_floats(net.mlp)
        assert P == flatten(Ws, bs).size
        slots = Slots(h, dev, R, P, extra, shift)
        for r, (dW, db) in enumerate(grads):
            device_pack(h, dev, net, Ws, bs, dW, db, slots.at(r), shift + r)
        out = Params(h, dev, Ws, bs, shift + 1)
        h.mlp_params_merge_device(net.mlp, slots.ptr, slots.stride, R, out.struct)
        h.sync()
        packed = slots.read()
        mW, mb = out.read()
    return packed, mW, mb


def device_merge_flat(h, Ws, bs, slots, extra=1, shift=0):
    """pmg_mlp_params_merge_device on slots [R, P] given as numpy -> the merged flat gradient"""
    with Dev(h) as dev:
        net = Net(h, dev, Ws, bs, 0)
        d = Slots(h, dev, slots.shape[0], slots.shape[1], extra, shift, fill=slots)
        out = Params(h, dev, Ws, bs, shift + 1)
        h.mlp_params_merge_device(net.mlp, d.ptr, d.stride, slots.shape[0], out.struct)
        h.sync()
        assert np.array_equal(AC.bits(d.read()), AC.bits(slots)), 'the slots were written'
        return flatten(*out.read())


def check_merge(packed, mW, mb, grads, Ws, bs, whole, label, model=None):
    """the three claims of one simulated-rank case"""
    for r, (dW, db) in enumerate(grads):                              # pack: the input bits, in the flat order
        assert np.array_equal(AC.bits(packed[r]), AC.bits(flatten(dW, db))), (label, 'slot', r)
    eq_bits(flatten(mW, mb), rank_sum(packed), (label, 'the merge is not the rank-ordered sum'))
    for k, (got, want) in enumerate(zip(mW + mb, list(whole['dW']) + list(whole['db']))):
        assert (got is None) == (want is None), (label, k)
        if got is not None:
            eq_val(got, want, (label, k, 'the merge is not the chunked gradient of the whole batch'))
    if model is not None:
        for k, (got, want) in enumerate(zip(mW + mb, list(model['dW']) + list(model['db']))):
            if got is not None:
                eq_val(got, want, (label, k, 'the merge is not the chunked model'))


# ----------------------------------------------------------------------------------------------------------------------
# 1. simulated ranks: the gradient of slice r into slot r, merged, against the chunked gradient of the whole batch
def case_simulated_ranks(library, R, B_local, nets=NETS):
    B = R * B_local
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, Dx, bias) in enumerate(nets):
            c = dp_case(widths, Dx, B, bias, ('target', 'gout', 'const')[(n + R) % 3])
            Ws, bs = c['Ws'], c['bs']
            grads = []
            for r in range(R):
                m = cut(c, slice(r * B_local, (r + 1) * B_local))
                g = GC.device_grad(h, Ws, bs, m['x'], m['a'], pad=n % 3, shift=(n + r) % 4, **m['kw'])
                grads.append((g['dW'], g['db']))
            whole = CC.device_grad_chunked(h, Ws, bs, c['x'], B_local, c['a'], pad=n % 3, shift=n % 4, **c['kw'])
            model = None
            if flatten(Ws, bs).size <= MODEL_PARAMS:
                model = cached(('dp model', tuple(widths), Dx, B, B_local, bias), lambda: CC.chunk_model(c['x'], Ws, bs, B_local, a=c['a'], **c['kw']))
            packed, mW, mb = device_pack_merge(h, Ws, bs, grads, extra=1 + n % 4, shift=n)
            check_merge(packed, mW, mb, grads, Ws, bs, whole, (widths, bias, R, B_local), model)


def case_policy_grad_ranks(library, R=3, B_local=34):
    """the same through pmg_policy_grad_device: the actor's gradient through the critic, L2 and clip"""
    Dx, A, B = 6, 3, R * B_local
    Wa, ba = GC.net(3101, (Dx, 33, A))
    Wc, bc = GC.net(3102, (Dx + A, 33, 1))
    x = np.random.RandomState(3103).uniform(-2, 2, (B, Dx)).astype(F32)
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        grads = []
        for r in range(R):
            g = PC.device_policy_grad(h, Wa, ba, Wc, bc, x[r * B_local:(r + 1) * B_local], -1.0 / B, 2.0 / (B * A), shift=r)
            grads.append((g['dW'], g['db']))
        whole = PC.device_policy_grad(h, Wa, ba, Wc, bc, x, -1.0 / B, 2.0 / (B * A), R=B_local)
        packed, mW, mb = device_pack_merge(h, Wa, ba, grads, extra=3, shift=1)
        check_merge(packed, mW, mb, grads, Wa, ba, whole, ('policy_grad', R, B_local))


def case_sac_policy_grad_ranks(library, R=2, B_local=34):
    """the same through pmg_sac_policy_grad_device; rank r passes row_offset = r * B_local, so its draws are those of the global rows"""
    Dx, A, B = 6, 3, R * B_local
    Wa, ba = GC.net(3201, (Dx, 33, 2 * A))
    W1, b1 = GC.net(3202, (Dx + A, 33, 1))
    W2, b2 = GC.net(3203, (Dx + A, 17, 1))
    x = np.random.RandomState(3204).uniform(-2, 2, (B, Dx)).astype(F32)
    kw = dict(gscale=-1.0 / B, lscale=1.0 / B, alpha=0.2, seed=5, counter=7)
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        grads = []
        for r in range(R):
            g = SP.device_sac_pg(h, Wa, ba, W1, b1, W2, b2, x[r * B_local:(r + 1) * B_local], row_offset=r * B_local, shift=r, **kw)
            grads.append((g['dW'], g['db']))
        whole = SP.device_sac_pg(h, Wa, ba, W1, b1, W2, b2, x, R=B_local, **kw)
        packed, mW, mb = device_pack_merge(h, Wa, ba, grads, extra=2, shift=2)
        check_merge(packed, mW, mb, grads, Wa, ba, whole, ('sac_policy_grad', R, B_local))


# ----------------------------------------------------------------------------------------------------------------------
# 2. the order of the sum: zeros, infinities, NaNs, roundings
def special_slots(P, R=3):
    """[R, P] whose columns rotate through sums that tell the order, the start value and the rounding"""
    one, tiny, big, inf, nan = F32(1), F32(2.0 ** -24), F32(3e38), F32(np.inf), F32(np.nan)
    cols = [(-0.0, -0.0, -0.0),          # -0 + -0 + -0 = -0: a sum started from +0.0 would give +0
            (-0.0, 0.0, -0.0),           # +0
            (inf, -inf, one),            # NaN
            (inf, one, -inf),            # NaN, later
            (one, inf, inf),             # inf
            (big, big, -big),            # (big + big) = inf, - big = inf; the other order gives big
            (-big, big, big),            # 0 + big = big
            (one, tiny, tiny),           # (1 + 2^-24) + 2^-24 = 1 twice; 1 + (2^-24 + 2^-24) would be 1 + 2^-23
            (tiny, tiny, one),           # 1 + 2^-23
            (nan, one, one), (one, one, nan), (-inf, -inf, one), (F32(1e-45), F32(-1e-45), -0.0), (F32(0.1), F32(0.2), F32(0.3))]
    s = np.empty((R, P), F32)
    for i in range(P):
        s[:, i] = (cols[i % len(cols)] * R)[:R]
    return s


def case_special_values(library):
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, bias) in enumerate((((5, 7, 2), 'all'), ((33, 3), 'none'))):
            Ws, bs = network(widths, bias, 3300 + n)
            P = flatten(Ws, bs).size
            for R in (1, 2, 3):
                slots = special_slots(P, 3)[:R]
                want = rank_sum(slots)
                if R == 3:
                    assert np.isnan(want[2]) and np.isnan(want[3]) and np.isinf(want[5]) and want[6] == F32(3e38) and want[7] == 1 and want[8] > 1
                    assert np.signbit(want[0]) and not np.signbit(want[1])
                eq_bits(device_merge_flat(h, Ws, bs, slots, extra=n, shift=R), want, (widths, R, 'special values'))


def case_one_slot_is_a_copy(library):
    """pack, then merge with one slot: the input bits, NaN payloads and the signs of zeros included"""
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, Dx, bias) in enumerate(NETS[:5]):
            Ws, bs = network(widths, bias, 3400 + n)
            P = flatten(Ws, bs).size
            words = np.random.RandomState(3401 + n).randint(0, 2 ** 32, P, dtype=np.uint64).astype(np.uint32)   # any bit pattern: NaNs, denormals
            words[:min(4, P)] = np.array([0x80000000, 0x7FC01234, 0xFF800000, 0x00000001], np.uint32)[:min(4, P)]
            dW, db = unflatten(words.view(F32), Ws, bs)
            packed, mW, mb = device_pack_merge(h, Ws, bs, [(dW, db)], extra=0, shift=n)
            assert np.array_equal(AC.bits(packed[0]), words), (widths, 'pack is no bit copy')
            assert np.array_equal(AC.bits(flatten(mW, mb)), words), (widths, 'the merge of one slot is no bit copy')


# ----------------------------------------------------------------------------------------------------------------------
# 3. fused merge + Adam against merge, then Adam
ADAM_CASES = (((1, 1), 'none', 1), ((5, 51), 'all', 2), ((33, 255, 2), 'mixed', 3), ((9, 256, 256, 256, 1), 'all', 8))


def adam_inputs(widths, bias, R, seed, t):
    """parameters, moments and R slots whose rank-ordered sum has the magnitudes and signs grad_cases.case_adam gives g: m and g agree in
    sign, so no step is small beside an ulp of its parameter (that case's bar is the one applied here)"""
    Ws, bs = network(widths, bias, seed)
    p = flatten(Ws, bs)
    rs = np.random.RandomState(seed + 1)
    sign = rs.choice([-1.0, 1.0], p.size)
    g = (rs.uniform(0.05, 0.15, p.size) * sign).astype(F32)
    m = (rs.uniform(0.02, 0.08, p.size) * sign).astype(F32)
    v = rs.uniform(0.001, 0.01, p.size).astype(F32)
    if t == 1:
        m[:], v[:] = 0, 0
    g[::3] = 0
    v[1::5] = 0
    share = rs.uniform(0.5, 1.5, (R, p.size))
    slots = (g[None, :] * share / share.sum(0)).astype(F32)
    return Ws, bs, p, m, v, slots


def device_adam_merge(h, Ws, bs, p, m, v, slots, t, fused, keep, extra=1, shift=0, lr=1e-3):
    """fused: pmg_mlp_adam_merge_device; else pmg_mlp_params_merge_device, then pmg_mlp_adam_device -> flat p, m, v, g (g None when not kept)"""
    with Dev(h) as dev:
        net = Net(h, dev, Ws, bs, 0)
        d = Slots(h, dev, slots.shape[0], slots.shape[1], extra, shift, fill=slots)
        Pp, Pm, Pv = (Params(h, dev, Ws, bs, shift + k, fill=unflatten(t_, Ws, bs)) for k, t_ in enumerate((p, m, v)))
        Pg = Params(h, dev, Ws, bs, shift + 3)
        adam = h.adam_struct(lr, t, 0.9, 0.999, 1e-8)
        if fused:
            h.mlp_adam_merge_device(net.mlp, Pp.struct, d.ptr, d.stride, slots.shape[0], Pg.struct if keep else None, Pm.struct, Pv.struct, adam)
        else:
            h.mlp_params_merge_device(net.mlp, d.ptr, d.stride, slots.shape[0], Pg.struct)
            h.mlp_adam_device(net.mlp, Pp.struct, Pg.struct, Pm.struct, Pv.struct, adam)
        h.sync()
        assert np.array_equal(AC.bits(d.read()), AC.bits(slots)), 'the slots were written'
        g = Pg.read(written=keep or not fused)
        return flatten(*Pp.read()), flatten(*Pm.read()), flatten(*Pv.read()), None if g[0] is None else flatten(*g)


def case_fused_adam(library, cases=ADAM_CASES):
    worst = 0.0
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for n, (widths, bias, R) in enumerate(cases):
            for t in (1, 1000):
                Ws, bs, p, m, v, slots = adam_inputs(widths, bias, R, 3500 + n, t)
                g = rank_sum(slots)
                m1, v1, p64, step = GC.adam_model(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, t)
                two = device_adam_merge(h, Ws, bs, p, m, v, slots, t, False, True, extra=n, shift=n)
                for keep in (True, False):
                    one = device_adam_merge(h, Ws, bs, p, m, v, slots, t, True, keep, extra=n + 1, shift=n + 1)
                    label = (widths, R, t, keep)
                    for k, name in ((1, 'm'), (2, 'v')):
                        assert np.array_equal(AC.bits(one[k]), AC.bits(two[k])), label + (name, 'fused differs from merge-then-Adam')
                        assert np.array_equal(AC.bits(one[k]), AC.bits((m1, v1)[k - 1])), label + (name, 'differs from the model')
                    if keep:
                        eq_bits(one[3], g, label + ('grad_out',))
                        eq_bits(two[3], g, label + ('merged gradient',))
                    for got in (one[0], two[0]):
                        err = GC.adam_error(got, p64, step, label)
                        worst = max(worst, err)
                        assert err <= GC.ADAM_TOL, label + (err,)
    print('fused merge + Adam: largest |p - p64| / |step64| = %.3g (bar %.3g)' % (worst, GC.ADAM_TOL))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# 4. one rank over the library's own collective (RCCL on the GPU build, the shared-memory stand-in on the emulator)
def one_rank(h):
    h.comm_init(0, 1, h.comm_unique_id())
    assert h.comm_info() == (0, 1)


def case_one_rank(library):
    """with one rank every collective is its single-rank call: the all-reduce returns the input bits, the fused all-reduce is
    pmg_mlp_adam_device, the collective normaliser update is pmg_norm_update_device, the all-gather copies"""
    with handle(library, 'push', num_envs=64) as env, handle(library, 'push', num_envs=64) as ref:
        h, hr = env.handle, ref.handle
        one_rank(h)
        # all-gather: a copy
        src = np.random.RandomState(3600).uniform(-1, 1, 1001).astype(F32)
        with Dev(h) as dev:
            d_src, out = dev.put(src), Out(dev, 4 * src.size, 4)
            h.allgather_device(d_src, src.size, out.ptr)
            h.allgather_device(d_src, 0, out.ptr)
            assert np.array_equal(AC.bits(out.read()), AC.bits(src))
        for n, (widths, bias) in enumerate((((33, 255, 2), 'mixed'), ((9, 256, 256, 256, 1), 'all'))):
            Ws, bs, p, m, v, slots = adam_inputs(widths, bias, 1, 3601 + n, 1000)
            g = slots[0]
            with Dev(h) as dev:
                net = Net(h, dev, Ws, bs, 0)
                P = h.mlp_param_floats(net.mlp)
                need = h.mlp_allreduce_work_floats(net.mlp)
                assert need == 2 * P
                # the all-reduce in place: the input bits; the workspace is sized exactly
                Pg, work = Params(h, dev, Ws, bs, n, fill=unflatten(g, Ws, bs)), Out(dev, 4 * need, 4 * (n & 3))
                h.mlp_grad_allreduce_device(net.mlp, Pg.struct, work.ptr, need)
                h.sync()
                work.read()
                assert np.array_equal(AC.bits(flatten(*Pg.read())), AC.bits(g)), (widths, 'the all-reduce of one rank changed the gradient')
                # the fused all-reduce: pmg_mlp_adam_device
                Pp, Pm, Pv = (Params(h, dev, Ws, bs, n + k, fill=unflatten(t_, Ws, bs)) for k, t_ in enumerate((p, m, v)))
                adam = h.adam_struct(1e-3, 1000, 0.9, 0.999, 1e-8)
                h.mlp_adam_allreduce_device(net.mlp, Pp.struct, Pg.struct, Pm.struct, Pv.struct, adam, work.ptr, need)
                h.sync()
                work.read()
                got = [flatten(*t_.read()) for t_ in (Pp, Pm, Pv, Pg)]
                Qp, Qm, Qv, Qg = (Params(h, dev, Ws, bs, n + k, fill=unflatten(t_, Ws, bs)) for k, t_ in enumerate((p, m, v, g)))
                h.mlp_adam_device(net.mlp, Qp.struct, Qg.struct, Qm.struct, Qv.struct, adam)
                h.sync()
                want = [flatten(*t_.read()) for t_ in (Qp, Qm, Qv, Qg)]
            m1, v1, p64, step = GC.adam_model(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1000)
            for k, name in ((1, 'm'), (2, 'v'), (3, 'grads')):
                assert np.array_equal(AC.bits(got[k]), AC.bits(want[k])), (widths, name, 'the fused all-reduce differs from pmg_mlp_adam_device')
            assert np.array_equal(AC.bits(got[1]), AC.bits(m1)) and np.array_equal(AC.bits(got[2]), AC.bits(v1))
            assert GC.adam_error(got[0], p64, step, widths) <= GC.ADAM_TOL and GC.adam_error(want[0], p64, step, widths) <= GC.ADAM_TOL
        # the normaliser: the same totals and derived values as pmg_norm_update_device, masked and strided, and then the env form
        for which, B in ((NC.OBS, 257), (NC.GOAL, 64), (NC.POL, 4097)):
            D = h.norm_width(which)
            rows = NC.uniform_rows(3610 + which, B, D + 2)
            mask = (np.random.RandomState(3611).uniform(size=B) < 0.7).astype(np.uint8)
            for hh, call in ((h, h.norm_update_ranks_device), (hr, hr.norm_update_device)):
                with Dev(hh) as dev:
                    call(which, dev.put(rows), D + 2, B, dev.put(mask))
                    call(which, dev.put(rows), D + 2, 0, None)
                    hh.sync()
            same_norm(h, hr, which, ('one rank', which, B))
        h.norm_update_env_ranks_device(None)
        hr.norm_update_env_device(None)
        for which in NC.KINDS:
            same_norm(h, hr, which, ('one rank, env rows', which))


def same_norm(h, hr, which, label):
    got, want = h.norm_read(which), hr.norm_read(which)
    assert want['count'] > 0
    for k in ('sum', 'sumsq', 'mean', 'std', 'inv_std'):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (label, k, got[k], want[k])
    assert got['count'] == want['count'], (label, got['count'], want['count'])


# ----------------------------------------------------------------------------------------------------------------------
# 5. real ranks: processes over the library's collective
def free_port():
    """a port the system hands out for binding to port 0"""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def norm_chunk(R, batch_local):
    return 64 * -(-R * batch_local // (64 * 1022))


RANK_NORM_BATCHES = {2: (64, 65664), 4: (64, 128)}          # per rank; 2 x 65 664 rows are cut at 192
assert norm_chunk(2, 65664) == 192 and 65664 % 192 == 0 and norm_chunk(2, 64) == norm_chunk(4, 128) == 64


def rank_worker(rank, world, port, library_path):
    """one rank of `world`: its shard of every collective, each result against the single-process call on the whole batch made by this same
    process on a second, unsharded handle.  Every assertion that can differ between ranks comes AFTER the collectives of its block."""
    import pybullet_multigoal_gym_amd as pmg
    from pybullet_multigoal_gym_amd import distributed as D
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    lib = PmgLibrary(library_path)
    rdv = D.Rendezvous(rank, world, addr='127.0.0.1', port=port, timeout=60)
    N = 64
    env = D.make_sharded_env(pmg.make_env, world * N, world, rank, task='reach', seed=11, seed_stride=1, _library=lib)
    env_rows = world == 2                                   # the env form needs an unsharded env of all ranks' envs beside it: two ranks only
    ref = pmg.make_env(task='reach', num_envs=world * N if env_rows else 8, seed=11, seed_stride=1, _library=lib)
    assert D.init_rccl(env, rdv)
    h, hr = env.handle, ref.handle
    B_local = 34
    assert D.check_data_parallel(env, rdv, B_local) == (rank, world)
    B = world * B_local
    mine = slice(rank * B_local, (rank + 1) * B_local)
    # the critic's gradient: all-reduced in place, then the fused all-reduce on a second copy of the network
    c = dp_case((9, 33, 1), 6, B, 'all', 'target', seed=3700)
    critic, twin = env.critic, ref.critic
    critic.load(c['Ws'], c['bs'])
    twin.load(c['Ws'], c['bs'])
    whole = twin.grad(c['x'], c['a'], gscale=c['kw']['gscale'], target=c['kw']['target'], chunk_rows=B_local)
    local = critic.grad(c['x'][mine], c['a'][mine], gscale=c['kw']['gscale'], target=c['kw']['target'][mine])
    state, tstate = critic.adam_state(), twin.adam_state()
    work = critic.allreduce_work_floats()
    assert work == (world + 1) * critic.param_floats()
    d_work = h.device_alloc(4 * work)
    state.g.upload(local['dW'], local['db'])
    critic.allreduce_grads_device(state.g, d_work, work)
    summed = state.g.download()
    state.g.upload(local['dW'], local['db'])
    critic.adam_step_allreduce_device(state.g, state, 1e-3, d_work, work)
    twin.adam_step_device(whole, tstate, 1e-3)
    for k in range(2):
        for l in range(2):
            eq_val(summed[k][l], (whole['dW'], whole['db'])[k][l], ('rank', rank, 'all-reduced gradient', k, l))
            assert np.array_equal(AC.bits(state.g.download()[k][l]), AC.bits((local['dW'], local['db'])[k][l])), 'the fused all-reduce wrote grads'
            for a, b in ((state.m, tstate.m), (state.v, tstate.v)):
                assert np.array_equal(AC.bits(a.download()[k][l]), AC.bits(b.download()[k][l])), ('rank', rank, 'm / v', k, l)
            g = (whole['dW'], whole['db'])[k][l]
            p0 = (c['Ws'], c['bs'])[k][l]
            _, _, p64, step = GC.adam_model(p0, g, np.zeros_like(g), np.zeros_like(g), 1e-3, 0.9, 0.999, 1e-8, 1)
            assert GC.adam_error(critic.parameters()[k][l], p64, step, ('rank', rank, 'p')) <= GC.ADAM_TOL
    assert state.t == 1
    h.device_free(d_work)
    # the normaliser: rows, masked rows, a chunk above 64, the env's rows
    for n, bl in enumerate(RANK_NORM_BATCHES[world]):
        rows = NC.uniform_rows(3710 + n, world * bl, 3)
        mask = None if n == 0 else (np.random.RandomState(3711).uniform(size=world * bl) < 0.8)
        s = slice(rank * bl, (rank + 1) * bl)
        env.normalizer.update_ranks(goal=rows[s], observation=rows[s] * 2, mask=None if mask is None else mask[s])
        ref.normalizer.update(goal=rows, observation=rows * 2, mask=mask)
        for which in (NC.GOAL, NC.OBS):
            same_norm(h, hr, which, ('rank', rank, 'rows', bl))
    if env_rows:
        env.normalizer.update_from_env_ranks()
        ref.normalizer.update_from_env()
        for which in NC.KINDS:
            same_norm(h, hr, which, ('rank', rank, 'env rows'))
    # SAC's temperature from the gathered log-probabilities
    logp = np.random.RandomState(3720).uniform(-6, 2, B).astype(F32)
    st0 = np.array([0.3, 0.01, 0.002, np.exp(F32(0.3))], F32)
    with Dev(h) as dev:
        d_all, d_st = dev.alloc(4 * B), dev.put(st0)
        h.allgather_device(dev.put(logp[mine]), B_local, d_all)
        h.sac_alpha_device(h.sac_alpha_struct(B, d_all, d_st, -3.0, 3e-4, 5))
        got_all, got = dev.get(d_all, B, F32), dev.get(d_st, 4, F32)
    want = SP.device_alpha(hr, logp, st0, -3.0, 3e-4, 5)[0]
    assert np.array_equal(AC.bits(got_all), AC.bits(logp)), ('rank', rank, 'the gathered logp')
    assert np.array_equal(AC.bits(got), AC.bits(want)), ('rank', rank, 'temperature', got, want)
    rdv.barrier()
    env.close()
    ref.close()
    rdv.close()


def run_ranks(world, library_path, timeout=240.0):
    """`world` fresh processes, each with its own time limit; every one must end with status 0"""
    import multiprocessing as mp
    ctx = mp.get_context('spawn')
    port = free_port()
    procs = [ctx.Process(target=rank_worker, args=(r, world, port, library_path)) for r in range(world)]
    for p in procs:
        p.start()
    codes = []
    for p in procs:
        p.join(timeout)
        if p.is_alive():
            p.kill()
            p.join()
            codes.append('timeout')
        else:
            codes.append(p.exitcode)
    assert codes == [0] * world, 'exit status per rank: %s' % codes


# ----------------------------------------------------------------------------------------------------------------------
# 6. what tests/test_dp_wave_order.py runs under every wavefront order
def wave_order_run(library):
    res = {}
    with handle(library, 'reach', num_envs=8) as env:
        h = env.handle
        for name, (widths, bias, R) in {'small': ((5, 51), 'all', 2), 'odd': ((33, 255, 2), 'mixed', 3), 'wide': ((6, 256, 256, 3), 'all', 8)}.items():
            Ws, bs, p, m, v, slots = adam_inputs(widths, bias, R, 3800 + R, 1000)
            grads = [unflatten(s, Ws, bs) for s in slots]
            packed, mW, mb = device_pack_merge(h, Ws, bs, grads, extra=3, shift=1)          # pmg_k_params_pack, pmg_k_params_merge_ranks
            res[name + ' packed'], res[name + ' merged'] = packed, flatten(mW, mb)
            one = device_adam_merge(h, Ws, bs, p, m, v, slots, 1000, True, True, extra=2, shift=2)     # pmg_k_adam_merge_ranks
            for k, t in zip('pmvg', one):
                res[name + ' adam ' + k] = t
    return res


# ----------------------------------------------------------------------------------------------------------------------
# 7. invalid calls
def case_invalid_calls(library):
    lib = library.lib
    lib.pmg_mlp_param_floats.restype = C.c_int64
    lib.pmg_mlp_allreduce_work_floats.restype = C.c_int64
    with handle(library, 'reach', num_envs=64) as env:
        h = env.handle
        Ws, bs = network((9, 16, 1), 'mixed', 3900)
        Wn, _ = network((9, 16, 1), 'none', 3901)
        P = flatten(Ws, bs).size
        assert P == 9 * 16 + 16 + 16
        with Dev(h) as dev:
            net, nobias = Net(h, dev, Ws, bs, 0), Net(h, dev, Wn, None, 0)
            NB = 4096
            outs = [dev.put(np.full(NB, SENTINEL, np.uint8)) for _ in range(12)]    # p, g, m, v (weight 0, bias 0, weight 1 each)
            d_slots = dev.put(np.zeros(3 * (P + 2), F32))
            d_rows, d_mask = dev.put(np.zeros((192, 5), F32)), dev.put(np.ones(192, np.uint8))
            guard = Out(dev, 4 * 4 * P)                                            # flat / workspace of the calls that must not run
            adam = h.adam_struct(1e-3, 1, 0.9, 0.999, 1e-8)

            def mlp(n=net, **kw):
                m = h.mlp_struct(n.widths, n.d_w, n.d_b, 0)
                for k, v in kw.items():
                    if k in ('width', 'd_weight', 'd_bias'):
                        getattr(m, k)[v[0]] = v[1]
                    else:
                        setattr(m, k, v)
                return m

            def params(k, **kw):
                p = h.params_struct([outs[3 * k], outs[3 * k + 2]], [outs[3 * k + 1], None])
                for name, v in kw.items():
                    getattr(p, name)[v[0]] = v[1]
                return p
            by = C.byref
            NULL = object()                                                       # pass NULL where None means "the default"
            none = lambda p: None if p is None or p is NULL else by(p)
            net_of = lambda m: NULL if m is NULL else (m or mlp())

            def pack(m=None, src=0, flat=guard.ptr):
                return lib.pmg_mlp_params_pack_device(h.h, none(net_of(m)), none(src if not isinstance(src, int) else params(src)), C.c_void_p(flat))

            def merge(m=None, slots=d_slots, stride=P + 2, nslots=3, out=1):
                return lib.pmg_mlp_params_merge_device(h.h, none(net_of(m)), C.c_void_p(slots), C.c_int64(stride), C.c_int64(nslots),
                                                       none(out if not isinstance(out, int) else params(out)))

            def fused(m=None, slots=d_slots, stride=P + 2, nslots=3, p=0, g=1, mm=2, v=3, a=adam):
                t = [none(x if not isinstance(x, int) else params(x)) for x in (p, g, mm, v)]
                return lib.pmg_mlp_adam_merge_device(h.h, none(net_of(m)), t[0], C.c_void_p(slots), C.c_int64(stride), C.c_int64(nslots), t[1], t[2], t[3], none(a))

            def reduce_(m=None, g=1, work=guard.ptr, floats=4 * P):
                return lib.pmg_mlp_grad_allreduce_device(h.h, none(net_of(m)), none(g if not isinstance(g, int) else params(g)), C.c_void_p(work), C.c_int64(floats))

            def reduce_adam(m=None, p=0, g=1, mm=2, v=3, a=adam, work=guard.ptr, floats=4 * P):
                t = [none(x if not isinstance(x, int) else params(x)) for x in (p, g, mm, v)]
                return lib.pmg_mlp_adam_allreduce_device(h.h, none(net_of(m)), t[0], t[1], t[2], t[3], none(a), C.c_void_p(work), C.c_int64(floats))

            def gather(src=d_slots, count=4, dst=guard.ptr):
                return lib.pmg_allgather_device(h.h, C.c_void_p(src), C.c_int64(count), C.c_void_p(dst))

            def norm(which=NC.GOAL, rows=d_rows, stride=5, batch=192, mask=d_mask):
                return lib.pmg_norm_update_ranks_device(h.h, C.c_int(which), C.c_void_p(rows), C.c_int64(stride), C.c_int64(batch), C.c_void_p(mask))

            def norm_env(mask=None):
                return lib.pmg_norm_update_env_ranks_device(h.h, C.c_void_p(mask))

            def untouched():
                h.sync()
                guard.read(written=False)
                for o in outs:
                    assert (dev.get(o, NB, np.uint8) == SENTINEL).all()
                return [t.copy() for t in NC.all_totals(h)]
            collectives = (reduce_, reduce_adam, gather, norm, norm_env)
            before = untouched()
            # 1. no communicator: PMG_E_STATE from every collective and from pmg_comm_info; the local entries need none
            rank, nranks = C.c_int32(-7), C.c_int32(-7)
            assert lib.pmg_comm_info(h.h, by(rank), by(nranks)) == E_STATE and (rank.value, nranks.value) == (-7, -7)
            for call in collectives:
                assert call() == E_STATE and 'pmg_comm_init' in h.L.error(h.h), call
            assert lib.pmg_mlp_allreduce_work_floats(h.h, by(mlp())) == 2 * P                 # one rank until pmg_comm_init says otherwise
            # 2. a communicator of two ranks (this process is rank 0; nothing below reaches a collective)
            h.comm_init(0, 2, h.comm_unique_id())
            assert h.comm_info() == (0, 2) and lib.pmg_comm_info(h.h, None, None) == 0
            assert lib.pmg_mlp_allreduce_work_floats(h.h, by(mlp())) == 3 * P == h.mlp_allreduce_work_floats(mlp())
            # under pmg_comm_overlap: PMG_E_STATE
            h.comm_overlap(True)
            for call in collectives:
                assert call() == E_STATE and 'pmg_comm_overlap' in h.L.error(h.h), call
            h.comm_overlap(False)
            bad_nets = [mlp(**kw) for kw in (dict(struct_size=C.sizeof(GC.PmgMlp) - 8), dict(num_layers=0), dict(num_layers=5), dict(width=(1, 257)),
                                             dict(width=(0, 0)), dict(d_weight=(0, None)), dict(d_weight=(1, outs[2] + 2)), dict(out_activation=2))]
            nan, inf = float('nan'), float('inf')
            bad_adams = [None] + [h.adam_struct(**dict(dict(lr=1e-3, step=1), **kw)) for kw in (dict(lr=nan), dict(lr=inf), dict(eps=-1.0), dict(eps=nan),
                                                                                                 dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(step=0))]
            short = h.adam_struct(1e-3, 1)
            short.struct_size -= 8
            bad_adams.append(short)
            bad = []
            for call in (pack, merge, fused, reduce_, reduce_adam):
                bad += [lambda call=call, m=m: call(m) for m in bad_nets]
                bad.append(lambda call=call: call(NULL))
            bad += [lambda: pack(src=None), lambda: pack(src=params(0, d_weight=(1, None))), lambda: pack(src=params(0, d_bias=(0, None))),
                    lambda: pack(src=params(0, d_weight=(0, outs[0] + 1))), lambda: pack(flat=None), lambda: pack(flat=guard.ptr + 2),
                    lambda: merge(out=None), lambda: merge(out=params(1, d_weight=(0, None))), lambda: merge(out=params(1, d_bias=(0, outs[4] + 3))),
                    lambda: merge(slots=None), lambda: merge(slots=d_slots + 1), lambda: merge(stride=P - 1), lambda: merge(stride=0), lambda: merge(nslots=0),
                    lambda: merge(nslots=-1), lambda: merge(nslots=1 << 40),
                    lambda: fused(p=None), lambda: fused(mm=None), lambda: fused(v=None), lambda: fused(g=params(1, d_weight=(1, None))),
                    lambda: fused(v=params(3, d_bias=(0, None))), lambda: fused(slots=None), lambda: fused(slots=d_slots + 2), lambda: fused(stride=P - 1),
                    lambda: fused(nslots=0), lambda: fused(mm=params(2, d_weight=(0, outs[6] + 1))),
                    lambda: reduce_(g=None), lambda: reduce_(g=params(1, d_bias=(0, None))), lambda: reduce_(work=None), lambda: reduce_(work=guard.ptr + 1),
                    lambda: reduce_(floats=3 * P - 1), lambda: reduce_(floats=0), lambda: reduce_(floats=-1),
                    lambda: reduce_adam(g=None), lambda: reduce_adam(p=None), lambda: reduce_adam(mm=None), lambda: reduce_adam(v=None),
                    lambda: reduce_adam(work=None), lambda: reduce_adam(work=guard.ptr + 2), lambda: reduce_adam(floats=3 * P - 1),
                    lambda: gather(src=None), lambda: gather(dst=None), lambda: gather(count=-1), lambda: gather(src=d_slots + 1), lambda: gather(dst=guard.ptr + 3),
                    lambda: norm(which=3), lambda: norm(which=-1), lambda: norm(rows=None), lambda: norm(rows=d_rows + 2), lambda: norm(stride=2), lambda: norm(batch=-1),
                    # two ranks: batch_local must be a multiple of the chunk of the GLOBAL batch (64 here)
                    lambda: norm(batch=1), lambda: norm(batch=63), lambda: norm(batch=65), lambda: norm(batch=191)]
            bad += [lambda a=a: fused(a=a) for a in bad_adams] + [lambda a=a: reduce_adam(a=a) for a in bad_adams]
            for k, call in enumerate(bad):
                assert call() == E_INVALID, k
                assert h.L.error(h.h), k
            assert 'multiple' in (norm(batch=65), h.L.error(h.h))[1]
            assert lib.pmg_mlp_param_floats(None) < 0 and lib.pmg_mlp_allreduce_work_floats(h.h, None) < 0 and lib.pmg_mlp_allreduce_work_floats(None, by(mlp())) < 0
            assert all(lib.pmg_mlp_param_floats(by(m)) < 0 for m in bad_nets[:6]) and lib.pmg_mlp_allreduce_work_floats(h.h, by(bad_nets[3])) < 0
            assert lib.pmg_mlp_param_floats(by(mlp())) == P and lib.pmg_mlp_param_floats(by(mlp(nobias))) == 9 * 16 + 16
            for f in (lib.pmg_comm_info, ):
                assert f(None, None, None) == E_INVALID
            assert lib.pmg_allgather_device(None, C.c_void_p(d_slots), C.c_int64(1), C.c_void_p(guard.ptr)) == E_INVALID
            assert lib.pmg_norm_update_ranks_device(None, 0, C.c_void_p(d_rows), C.c_int64(5), C.c_int64(64), None) == E_INVALID
            assert lib.pmg_norm_update_env_ranks_device(None, None) == E_INVALID
            # successful no-ops that reach no collective: a zero batch, a zero count
            assert norm(batch=0) == 0 and gather(count=0) == 0
            after = untouched()
            for u, v in zip(before, after):
                assert np.array_equal(u, v), 'a refused call changed the normalisers'
            # what is allowed, with exactly sized buffers: a stride of P, a bias pointer where the shape has no bias (ignored), one slot
            exact = Slots(h, dev, 3, P, 0, 1, fill=np.ones((3, P), F32))
            assert merge(slots=exact.ptr, stride=P) == 0 and merge(mlp(nobias), slots=exact.ptr, stride=P, nslots=1) == 0
            flat = Out(dev, 4 * P, 4)
            assert pack(src=1, flat=flat.ptr) == 0
            h.sync()
            exact.read(), flat.read()
        # the env form: the ranks' envs must be the global envs in rank order; PMG_E_STATE before the first reset is pmg_norm_update_env_device's
    with handle(library, 'reach', num_envs=64, env_index_offset=32) as env:
        h = env.handle
        one_rank(h)
        assert h.L.lib.pmg_norm_update_env_ranks_device(h.h, None) == E_INVALID and 'env_index_offset' in h.L.error(h.h)
    with handle(library, 'reach', num_envs=65) as env:                          # two ranks x 65 envs: no multiple of 64
        h = env.handle
        h.comm_init(0, 2, h.comm_unique_id())
        assert h.L.lib.pmg_norm_update_env_ranks_device(h.h, None) == E_INVALID and 'multiple' in h.L.error(h.h)
