"""The cross-lane primitives of the SHIPPED pybullet_multigoal_gym_amd/csrc/pmg_wave.h, one at a time, on a real gfx950:
every primitive of wv / wr whose result is data, every template argument, in a full wavefront, with one 16-lane row active
at a time, and on the helper wavefronts of two- and three-wavefront workgroups -- against numpy models written from the
header's comments (tests/wave_models.py; tests/test_wave_primitive_models.py holds the emulator's stand-in to the same
models).  A failure names the primitive family and the lane context.

Not probed: as_lds, lds_sync, set_priority, cycles, opaque, chain (no data result) and the internal dpp<CTRL> helper, which
every row_* / *_sum primitive goes through."""
import ctypes as C
import os

import numpy as np
import pytest

import wave_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, 'gpu_probe')


@pytest.fixture(scope='module')
def probe(built):
    """pmgd_prim of the probe library built like the product: the inline-asm DPP paths that ship"""
    lib = C.CDLL(os.path.join(PROBE_DIR, 'libpmg_gpu_probe.so'))
    assert lib.pmgd_variant() == 0
    return lib.pmgd_prim


@pytest.fixture(scope='module')
def probe_plain(built):
    """... and of the second instantiation: -DPMG_NO_R0_DPP -DPMG_NO_DPP_FMAC -DPMG_NO_NEWBCAST, the header's plain C++ branches"""
    lib = C.CDLL(os.path.join(PROBE_DIR, 'libpmg_gpu_probe_plain.so'))
    assert lib.pmgd_variant() == 1
    return lib.pmgd_prim


@pytest.mark.parametrize('ns,fam,ctx', M.cases())
def test_shipped_primitive_matches_model(probe, ns, fam, ctx):
    """lane-coded integer inputs (exact in float32 whatever the order), every run-time lane: uint32-equal to the model in
    every lane for which the contract defines a result"""
    M.check_against_model(probe, ns, fam, ctx)


@pytest.mark.parametrize('ns,fam,ctx', M.cases())
def test_plain_instantiation_matches_model(probe_plain, ns, fam, ctx):
    """the same on the plain C++ branches.  Two of them promise less than the shipped paths, by construction:
    - wr::bcast_c without row_newbcast rotates the source quad into the other quads and "does not write quad 3": lanes
      12..15 of a row are outside its contract (the robot's nine DoFs live in lanes 0..8);
    - wr::dot6_bcast_r0_c / gj9 / gj6 / dot6_lanes_r0 forward to wv::, whose plain branch reads lane SRC of the WAVE
      (v_readlane), i.e. of row 0: only row 0 of a packed wavefront is defined.
    Everything else is held to the full model."""
    M.check_against_model(probe_plain, ns, fam, ctx, defined_filter=_plain_defined(ns, fam))


def _plain_defined(ns, fam):
    keep = np.ones(64, bool)
    if ns == 'wr' and fam in ('bcast_c', 'fma2_bcast_c', 'bcast_r0', 'fma2_bcast_r0_c'):
        keep = (M.L & 15) < 12
    if ns == 'wr' and fam in ('dot6_bcast_r0_c', 'gj9_eliminate_r0_c', 'gj6_eliminate_r0_c', 'dot6_lanes_r0'):
        keep = M.L < 16
    return keep


@pytest.mark.parametrize('ns,fam,ctx', [p for p in M.cases() if p.values[2] in ('full_wave', 'row_by_row', 'wave1_of_2')])
def test_asm_and_plain_instantiations_agree_bit_for_bit_on_random_data(probe, probe_plain, ns, fam, ctx):
    """random float32 of mixed magnitude with zeros of both signs and denormals: the inline-asm DPP path and the plain path
    are the same fmaf / add / mul in the same order, so they agree bit for bit wherever both contracts define a result (the
    plain branches' narrower contracts: test_plain_instantiation_matches_model)."""
    rowsel = M.CONTEXTS[ctx][2]
    keep = _plain_defined(ns, fam)
    compared = 0
    for seed in range(4):
        inp = M.random_inputs(1000 * seed + M.FAM[fam])
        if fam == 'predicate':
            inp[1] = np.float32(2.5) if ns == 'wv' else np.repeat(np.float32([2.5, -1.0, 0.0, 1e-30]), 16)
        for src in M.sources(ns, fam)[::5]:
            a = M.run_probe(probe, ns, fam, ctx, src, inp)
            b = M.run_probe(probe_plain, ns, fam, ctx, src, inp)
            _, defined = M.expected(ns, fam, inp, rowsel, src)
            defined &= keep[None, :]
            bad = M.mismatches(a, b, defined)
            assert not bad, '%s::%s (%s, src %d, seed %d): %d differences, first (slot, lane) %s: asm %r, plain %r' % (
                ns, fam, ctx, src, seed, len(bad), bad[:4], a[bad[0]], b[bad[0]])
            compared += int(defined.sum())
    assert compared > 0


def _ulps(got, exact):
    """|got - exact| in units of the float32 spacing at the exact value"""
    ulp = 2.0 ** (np.floor(np.log2(np.abs(exact))) - 23)
    return np.abs(got.astype(np.float64) - exact) / ulp


@pytest.mark.parametrize('ns', ['wv', 'wr'])
def test_fsqrt_and_rcp_are_within_one_ulp_of_float64(probe, ns):
    """the header: fsqrt and rcp are the hardware instructions alone, 1 ulp.  A logarithmic sweep of NORMAL arguments over the
    whole exponent range for the root, and over 2^-100 .. 2^100 (results normal too), both signs, for the reciprocal."""
    rs = np.random.RandomState(7)
    worst = [0.0, 0.0]
    for batch in range(48):
        inp = np.zeros((M.NIN, 64), np.float32)
        inp[0] = (rs.uniform(1, 2, 64) * 2.0 ** rs.uniform(-126, 127, 64)).astype(np.float32)
        inp[1] = (rs.choice([-1.0, 1.0], 64) * rs.uniform(1, 2, 64) * 2.0 ** rs.uniform(-100, 100, 64)).astype(np.float32)
        if batch == 0:
            inp[0, :8] = np.float32([1.0, 4.0, 2.0, 0.25, 1.17549435e-38, 3.4028235e38, 9.0, 0.5])
            inp[1, :8] = np.float32([1.0, -1.0, 2.0, 0.5, 3.0, -3.0, 1e-30, 1e30])
        out = M.run_probe(probe, ns, 'sqrt_rcp', 'full_wave', 0, inp)
        x = inp.astype(np.float64)
        worst[0] = max(worst[0], _ulps(out[0], np.sqrt(x[0])).max())
        worst[1] = max(worst[1], _ulps(out[1], 1.0 / x[1]).max())
    print('%s: fsqrt worst %.3f ulp, rcp worst %.3f ulp' % (ns, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


def test_fsqrt_flushes_denormal_arguments_to_zero_as_documented(probe):
    """the header: 'no rescaling of denormal arguments: they flush to zero'; zeros keep their sign as IEEE sqrt does"""
    inp = np.zeros((M.NIN, 64), np.float32)
    den = (np.linspace(1, (1 << 23) - 1, 62).astype(np.uint32)).view(np.float32)
    inp[0, :62] = den
    inp[0, 62:] = np.float32([0.0, -0.0])
    inp[1] = 1.0
    assert (inp[0, :62] > 0).all() and (inp[0, :62] < np.float32(1.17549435e-38)).all()
    out = M.run_probe(probe, 'wv', 'sqrt_rcp', 'full_wave', 0, inp)
    assert np.array_equal(out[0, :62], np.zeros(62, np.float32)), out[0, :62]
    assert np.array_equal(out[0, 62:].view(np.uint32), np.float32([0.0, -0.0]).view(np.uint32))
