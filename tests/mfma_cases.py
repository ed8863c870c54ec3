"""Cases and model of the matrix-pipe primitive wv::mfma_32x32x2 (csrc/pmg_wave.h) -- TEST INFRASTRUCTURE, shared by
tests/test_mfma_emulated.py (the header's PMG_EMULATE branch on the fiber emulator) and tests/test_gpu_mfma.py (its device form,
v_mfma_f32_32x32x2_f32, on the gfx950 build of gpu_probe/).  Both run prim::mfma_chain (gpu_probe/pmg_prim_probe.inc): `steps`
chained calls on one accumulator, one wavefront.

The model is written from the header's comment: lane l hands in a = A[l & 31][l >> 5] and b = B[l >> 5][l & 31]; register r of
lane l is D[8 (r >> 2) + 4 (l >> 5) + (r & 3)][l & 31] = fmaf(A[i][1], B[1][j], fmaf(A[i][0], B[0][j], C[i][j])), every fmaf an
exact float32 fused multiply-add (actor_cases.fmaf), k = 0 first.  The bar is the bit pattern of every one of the 16 x 64 results
of every case: the instruction is documented as an exact f32 fmaf chain, so nothing is left to a tolerance."""
import ctypes as C

import numpy as np

from actor_cases import fmaf

F32 = np.float32
LANE = np.arange(64)
COL, HALF = LANE & 31, LANE >> 5


def model(a, b, c):
    """a, b [n, steps, 64], c [n, 16, 64] -> [n, 16, 64]"""
    n, steps = a.shape[:2]
    out = np.empty_like(c)
    for r in range(16):
        row = 8 * (r >> 2) + 4 * HALF + (r & 3)
        acc = c[:, r, :]
        for s in range(steps):
            for k in range(2):
                acc = fmaf(a[:, s, 32 * k + row], b[:, s, 32 * k + COL], acc).reshape(n, 64)
        out[:, r, :] = acc
    return out


def operand_sets():
    """name -> (a, b, c).  Shapes: one call, the five-step chain of the reach row set-up, the longest chain the probe takes"""
    rs = np.random.RandomState(950)
    sets = {}
    # random values, one call on a random accumulator; then the chain of the kernel from a zero accumulator
    sets['random, one call'] = (rs.normal(size=(4, 1, 64)), rs.normal(size=(4, 1, 64)), rs.normal(size=(4, 16, 64)))
    sets['random, chain of five'] = (rs.normal(size=(4, 5, 64)), rs.normal(size=(4, 5, 64)), np.zeros((4, 16, 64)))
    # the padding the kernel relies on: rows of A beyond 9, columns of B beyond 24 and the upper k of the last step are exact
    # zeros (first product); rows of A beyond 24 (second product)
    a, b = rs.normal(size=(2, 5, 64)), rs.normal(size=(2, 5, 64))
    a[0][:, COL >= 9] = 0; a[1][:, COL >= 24] = 0
    b[:, :, COL >= 24] = 0
    a[:, 4, HALF == 1] = 0; b[:, 4, HALF == 1] = 0
    sets['zero rows, columns and k-steps'] = (a, b, np.zeros((2, 16, 64)))
    # signed zeros in the operands and in the accumulator
    a, b, c = rs.normal(size=(4, 2, 64)), rs.normal(size=(4, 2, 64)), np.zeros((4, 16, 64))
    a[rs.uniform(size=a.shape) < 0.4] = 0; b[rs.uniform(size=b.shape) < 0.4] = 0
    a = np.where(rs.uniform(size=a.shape) < 0.5, -a, a); b = np.where(rs.uniform(size=b.shape) < 0.5, -b, b)      # (-0.0 where the entry is 0)
    c = np.where(rs.uniform(size=c.shape) < 0.5, -c, c)
    sets['signed zeros'] = (a, b, c)
    # magnitudes from 1e-6 to 1e3, both signs
    mag = lambda shape: 10.0 ** rs.uniform(-6, 3, shape) * rs.choice([-1.0, 1.0], shape)
    sets['1e-6 to 1e3'] = (mag((4, 8, 64)), mag((4, 8, 64)), mag((4, 16, 64)))
    return {k: tuple(np.ascontiguousarray(v, F32) for v in t) for k, t in sets.items()}


SETS = operand_sets()


def run(fn, a, b, c):
    """fn: pmge_mfma / pmgd_mfma -> out [n, 16, 64]; the sentinel shows a result the probe did not write"""
    out = np.full(c.shape, np.float32(-7777.0), F32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = fn(C.c_int(a.shape[0]), C.c_int(a.shape[1]), p(a), p(b), p(c), p(out))
    assert rc == 0, rc
    return out


def check(fn, name, out=print):
    a, b, c = SETS[name]
    got, want = run(fn, a, b, c), model(a, b, c)
    assert np.isfinite(want).all()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    out('%-32s %d results, %d differ in their bits' % (name, got.size, len(bad)))
    assert not len(bad), (name, '[case, register, lane] of the first differences', bad[:6].tolist(),
                          [(float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]])
    if name == 'zero rows, columns and k-steps':
        # what the padding must give: exact zeros in the rows and columns that do not exist
        row = 8 * (np.arange(16)[:, None] >> 2) + 4 * HALF[None, :] + (np.arange(16)[:, None] & 3)
        assert (got[0][(row >= 9) | (COL[None, :] >= 24)] == 0).all()
        assert (got[1][(row >= 24) | (COL[None, :] >= 24)] == 0).all()
        assert (got[0][(row < 9) & (COL[None, :] < 24)] != 0).all()


def test_the_model_tells_the_k_order_and_the_row_map_apart():
    """the model with k = 1 first, or with the halves of the row map swapped, gives other bits on the random chain"""
    a, b, c = SETS['random, chain of five']
    want = model(a, b, c)
    swapped_k = model(np.concatenate([a[:, :, 32:], a[:, :, :32]], 2), np.concatenate([b[:, :, 32:], b[:, :, :32]], 2), c)
    assert (swapped_k.view(np.uint32) != want.view(np.uint32)).mean() > 0.05
    assert (want[:, :, :32] != want[:, :, 32:]).mean() > 0.9
