"""numpy models of the cross-lane primitives of pmg_wave.h, written from the header's COMMENTS (what each primitive
promises), not from its code -- and the one place that knows the slot layout of the primitive probes
(gpu_probe/pmg_prim_probe.inc).  Two headers answer to them: the shipped
pybullet_multigoal_gym_amd/csrc/pmg_wave.h on a gfx950 (tests/test_gpu_wave_primitives.py) and the emulator's stand-in
tests/emu/pmg_wave.h (tests/test_wave_primitive_models.py).

A model takes the inputs of ONE wavefront, [NIN][64] float32, the set of lanes that execute the call together, and the
run-time lane argument; it returns the outputs [NOUT][64] and a mask of the (slot, lane) pairs for which the contract
DEFINES a result.  Inputs of the bit-exact checks are lane-coded small integers (exact_inputs): every sum and product
stays below 2^24, so float32 is exact in any order of evaluation, and a wrong source lane cannot give the right value."""
import ctypes as C

import numpy as np

NIN, NOUT, LANES = 16, 160, 64
FAMILIES = ['bcast', 'bcast_c', 'fma2_bcast_c', 'half', 'bcast_r0', 'fma2_bcast_r0_c', 'dot6_bcast_r0_c', 'gj9_eliminate_r0_c',
            'gj6_eliminate_r0_c', 'dot6_lanes_r0', 'add_shr2_bank2', 'row_shift', 'reduce', 'predicate', 'lane_id', 'sqrt_rcp']
FAM = {n: i for i, n in enumerate(FAMILIES)}
# the model families (sqrt_rcp is measured against float64, not modelled bit for bit)
MODELLED = FAMILIES[:-1]
# families with primitives that stay inside the caller's 16-lane row in namespace wv too (the model marks which of their
# results a single row defines; the ballots of `predicate` and the wave-wide broadcasts are whole-wave operations there)
WV_ROW_LOCAL = ['half', 'bcast_r0', 'fma2_bcast_r0_c', 'dot6_bcast_r0_c', 'gj9_eliminate_r0_c', 'gj6_eliminate_r0_c', 'dot6_lanes_r0',
                'add_shr2_bank2', 'row_shift', 'reduce', 'lane_id']
SENTINEL = np.float32(-77777.0)
L = np.arange(64)
ROW0 = L < 16


def exact_inputs(seed):
    """[NIN][64]: slot k holds a permutation of 64 k + 1 .. 64 k + 64 with mixed signs: distinct in every lane and slot"""
    rs = np.random.RandomState(seed)
    a = np.zeros((NIN, 64), np.float32)
    for k in range(NIN):
        a[k] = (rs.permutation(64) + 1 + 64 * k) * rs.choice([-1, 1], 64)
    return a


def predicate_inputs(seed, ns, positive):
    """slot 0: the predicate (0 / non-zero), slot 1: a value that is uniform over the env (wave / row), slots 2, 3: distinct"""
    rs = np.random.RandomState(seed)
    a = exact_inputs(seed)
    a[0] = rs.randint(0, 2, 64) * a[0]
    a[0, 16 * rs.randint(4):][:16] = 0                     # one row without any hit
    sign = 1.0 if positive else -1.0
    a[1] = sign * (3.0 if ns == 'wv' else np.repeat([3.0, 5.0, 7.0, 9.0], 16))
    return a


def random_inputs(seed):
    """float32 of mixed magnitude (2^-20 .. 2^20), both signs, with zeros of both signs and denormals sprinkled in"""
    rs = np.random.RandomState(seed)
    a = (rs.choice([-1.0, 1.0], (NIN, 64)) * rs.uniform(1, 2, (NIN, 64)) * 2.0 ** rs.randint(-20, 21, (NIN, 64))).astype(np.float32)
    kind = rs.randint(0, 12, (NIN, 64))
    a[kind == 0] = np.float32(0.0)
    a[kind == 1] = np.float32(-0.0)
    den = (rs.randint(1, 1 << 23, (NIN, 64)).astype(np.uint32) | (rs.randint(0, 2, (NIN, 64)).astype(np.uint32) << 31)).view(np.float32)
    a[kind == 2] = den[kind == 2]
    return a


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _row_lane(ns, s):
    """lane index of `row lane s`: of row 0 in wv, of the caller's own row in wr"""
    return np.full(64, s) if ns == 'wv' else (L & 48) + s


def model(ns, fam, inp, active, src, any_row_mask_per_row=False):
    """-> (out [NOUT][64] float32, defined [NOUT][64] bool).  ns: 'wv' (one env per wavefront) / 'wr' (one per 16-lane row)"""
    name = FAMILIES[fam] if isinstance(fam, int) else fam
    x = inp.astype(np.float64)
    out = np.full((NOUT, 64), SENTINEL, np.float32)
    oi = out.view(np.uint32)
    df = np.zeros((NOUT, 64), bool)
    nl = 64 if ns == 'wv' else 16
    src &= nl - 1
    act = np.asarray(active, bool)
    rowlocal = act if ns == 'wr' else act & ROW0           # where a "row 0" primitive of the namespace defines its result
    xi = inp.view(np.uint32)

    def put(o, val, where):
        out[o] = _f32(val)
        df[o] = where

    def puti(o, val, where):
        oi[o] = np.asarray(val).astype(np.uint32)
        df[o] = where

    def wide(s):                                            # source lane of a wave-wide (wv) / row-wide (wr) broadcast
        return np.full(64, s) if ns == 'wv' else (L & 48) + s

    if name == 'bcast':
        s = wide(src)
        put(0, x[0][s], act & act[s])
        puti(1, xi[1][s], act & act[s])
        for k in range(3):
            put(2 + k, x[k][s], act & act[s])
        for S in range(nl):
            put(8 + S, x[0][wide(S)], act & act[wide(S)])
        for S in range(16):
            puti(72 + S, xi[1][wide(S)], act & act[wide(S)])
    elif name == 'bcast_c':
        for S in range(nl):
            put(S, x[0][wide(S)], act & act[wide(S)])
        if ns == 'wr':
            for S in range(16):
                puti(64 + S, xi[1][wide(S)], act)
    elif name == 'fma2_bcast_c':
        for S in range(nl):
            b = x[0][wide(S)]
            put(2 * S, x[1] + x[3] * b, act & act[wide(S)])
            put(2 * S + 1, x[2] + x[4] * b, act & act[wide(S)])
    elif name == 'half':
        for S in range(8):
            b = x[0][(L & ~7) + S]
            put(S, b, act)
            put(8 + S, x[1] + x[2] * b, act)
    elif name == 'bcast_r0':
        for S in range(16):
            put(S, x[0][_row_lane(ns, S)], rowlocal)
            put(17 + S, x[0][_row_lane(ns, S)], rowlocal)
        s = _row_lane(ns, src & 15)
        put(16, x[0][s], rowlocal)
        put(33, x[0][s], rowlocal)
        put(34, x[1][s], rowlocal)
    elif name == 'fma2_bcast_r0_c':
        for S in range(16):
            b = x[0][_row_lane(ns, S)]
            put(2 * S, x[1] + x[3] * b, rowlocal)
            put(2 * S + 1, x[2] + x[4] * b, rowlocal)
    elif name == 'dot6_bcast_r0_c':
        for S in range(16):
            s = _row_lane(ns, S)
            put(S, sum(x[a][s] * x[6 + a] for a in range(6)), rowlocal)
    elif name == 'gj9_eliminate_r0_c':
        for P in range(9):
            s = _row_lane(ns, P)
            for j in range(9):
                put(9 * P + j, x[j] if j == P else x[j] + x[9] * x[j][s], rowlocal)
    elif name == 'gj6_eliminate_r0_c':
        for P in range(6):
            s = _row_lane(ns, P)
            for j in range(6):
                put(7 * P + j, x[j] if j == P else x[j] + x[7] * x[j][s], rowlocal)
            put(7 * P + 6, x[6] + x[7] * x[6][s], rowlocal)
    elif name == 'dot6_lanes_r0':
        put(0, sum(x[a] * x[6][_row_lane(ns, a)] for a in range(6)), rowlocal)
    elif name == 'add_shr2_bank2':
        rl = L & 15
        put(0, np.where((rl >= 8) & (rl < 12), x[0][np.maximum(L - 2, 0)] + x[1], x[0]), act)
    elif name == 'row_shift':
        rl = L & 15
        for N in range(1, 16):
            put(N - 1, np.where(rl >= N, x[0][np.maximum(L - N, 0)], x[1]), act)
            put(15 + N - 1, np.where(rl + N <= 15, x[0][np.minimum(L + N, 63)], x[1]), act)
    elif name == 'reduce':
        rows = x[0].reshape(4, 16).sum(1)
        rmax = x[1].reshape(4, 16).max(1)
        own = L >> 4
        whole = act if ns == 'wr' else act & bool(act.all())   # a wave-wide result needs the whole wave (wv); a row's its row (wr)
        put(0, rows[own], act)
        put(1, x[0].reshape(8, 8).sum(1)[L >> 3], act)
        put(2, rmax[own], act)
        if ns == 'wv':
            put(3, np.full(64, rows[0]), act & act[0])
            put(4, np.full(64, rmax[0]), act & act[0])
            for NR in range(1, 5):
                put(4 + NR, np.full(64, rows[:NR].sum()), act & bool(act[:16 * NR].all()))
            put(9, np.full(64, rows.sum()), whole)
            put(10, np.full(64, rows.sum()), whole)
            put(11, np.full(64, rmax.max()), whole)
        else:                                               # an env owns exactly one row: every one of them is the row's
            for o in (3, 5, 6, 7, 8, 9, 10):
                put(o, rows[own], act)
            for o in (4, 11):
                put(o, rmax[own], act)
    elif name == 'predicate':
        p = (inp[0] != 0) & act
        bits = sum(1 << int(l) for l in L[p])
        if ns == 'wv':
            puti(0, np.full(64, bits & 0xFFFFFFFF, np.uint32), act)
            puti(1, np.full(64, bits >> 32, np.uint32), act)
            puti(2, np.full(64, bits & 0xFFFF, np.uint32), act)
            puti(3, np.full(64, int(bits != 0), np.uint32), act)
            put(5, np.where(L == (src & 15), x[2], x[3]), act)
        else:
            rowbits = np.array([(bits >> (16 * r)) & 0xFFFF for r in range(4)], np.uint32)
            puti(0, rowbits[L >> 4], act)
            puti(1, np.zeros(64, np.uint32), act)
            anyrow = rowbits[L >> 4] if any_row_mask_per_row else np.full(64, np.bitwise_or.reduce(rowbits), np.uint32)
            puti(2, anyrow, act)
            puti(3, (rowbits[L >> 4] != 0).astype(np.uint32), act)
            put(5, np.where((L & 15) == (src & 15), x[2], x[3]), act)
        puti(4, (inp[1] > 0).astype(np.uint32), act)
    elif name == 'lane_id':
        lane = L if ns == 'wv' else L & 15
        puti(0, lane.astype(np.uint32), act)
        puti(1, lane.astype(np.uint32), act)
        if ns == 'wr':
            puti(2, (L >> 4).astype(np.uint32), act)
    else:
        raise ValueError(name)
    return out, df


# the lane contexts of a probe call: (threads of the workgroup, wavefront that runs the probe, row selector)
CONTEXTS = {
    'full_wave': (64, 0, -1),
    'row_by_row': (64, 0, 4),
    'wave1_of_2': (128, 1, -1),
    'wave2_of_3': (192, 2, -1),
    'row_by_row_wave1_of_2': (128, 1, 4),
}


def expected(ns, fam, inp, rowsel, src, **kw):
    """the model under a row selector (-1: 64 lanes together; k: row k alone; 4: the rows one after the other)"""
    if rowsel < 0:
        return model(ns, fam, inp, np.ones(64, bool), src, **kw)
    out = np.full((NOUT, 64), SENTINEL, np.float32)
    df = np.zeros((NOUT, 64), bool)
    for k in (range(4) if rowsel == 4 else [rowsel]):
        o, d = model(ns, fam, inp, (L >> 4) == k, src, **kw)
        out.view(np.uint32)[d] = o.view(np.uint32)[d]
        df |= d
    return out, df


def run_probe(fn, ns, fam, ctx, src, inp):
    """one call of pmgd_prim / pmge_prim -> out [NOUT][64] (SENTINEL where the probe wrote nothing)"""
    threads, wave, rowsel = CONTEXTS[ctx] if isinstance(ctx, str) else ctx
    fam = FAM[fam] if isinstance(fam, str) else fam
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.full((NOUT, 64), SENTINEL, np.float32)
    rc = fn(C.c_int(ns == 'wr'), C.c_int(fam), C.c_int(threads), C.c_int(wave), C.c_int(rowsel), C.c_int(src),
            inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, 'probe call failed: status %d' % rc
    return out


def sources(ns, fam):
    """run-time lane arguments worth a call: every lane for the families that take one, one call otherwise"""
    name = FAMILIES[fam] if isinstance(fam, int) else fam
    if name == 'bcast':
        return list(range(64 if ns == 'wv' else 16))
    if name in ('bcast_r0', 'predicate'):
        return list(range(16))
    return [0]


def mismatches(got, want, defined):
    """(slot, lane) pairs of the defined results whose BITS differ"""
    bad = (got.view(np.uint32) != want.view(np.uint32)) & defined
    return [(int(o), int(l)) for o, l in zip(*np.nonzero(bad))]


def cases():
    """pytest parameters: one id per namespace x primitive family x lane context"""
    import pytest
    for ns in ('wv', 'wr'):
        for fam in MODELLED:
            for ctx in CONTEXTS:
                if ns == 'wv' and ctx.startswith('row_by_row') and fam not in WV_ROW_LOCAL:
                    continue
                yield pytest.param(ns, fam, ctx, id='%s-%s-%s' % (ns, fam, ctx))


def check_against_model(fn, ns, fam, ctx, defined_filter=None, **kw):
    """every run-time lane argument of the family, exact inputs: the defined results equal the model's BIT FOR BIT, and
    (defined_filter: lanes [64] to which a narrower contract restricts the check)"""
    rowsel = CONTEXTS[ctx][2]
    checked = 0
    for src in sources(ns, fam):
        variants = [exact_inputs(100 + src)] if fam != 'predicate' else [predicate_inputs(src, ns, True), predicate_inputs(50 + src, ns, False)]
        for inp in variants:
            got = run_probe(fn, ns, fam, ctx, src, inp)
            want, defined = expected(ns, fam, inp, rowsel, src, **kw)
            if defined_filter is not None:
                defined &= np.asarray(defined_filter, bool)[None, :]
            bad = mismatches(got, want, defined)
            assert not bad, '%s::%s (%s, src %d): %d wrong results, first (slot, lane) %s: got %r, model %r' % (
                ns, fam, ctx, src, len(bad), bad[:4], got[bad[0]], want[bad[0]])
            checked += int(defined.sum())
    assert checked > 0
    return checked
