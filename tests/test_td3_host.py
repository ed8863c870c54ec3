"""TD3's target off the device: the numpy model of tests/td3_cases.py alone (draws, the clipped noise, the model against float64), the
bindings, and Critic.td3_target (pybullet_multigoal_gym_amd/critic.py) over the emulator build of the C ABI."""
import ctypes as C

import numpy as np

import actor_cases as AC
import grad_cases as GC
import td3_cases as T3
from pybullet_multigoal_gym_amd._lib import PmgLibrary, PmgTd3Target

# seeds of test_model_against_float64, chosen on the CPU among 1 .. 12: for all twelve the float32 and the float64 evaluation take the same
# side of every clip and of the min (no predicate sits on an edge); 1, 2 and 5 are the first three for which every predicate -- the
# actor's clip, the noise clip, the clip of the sum, either choice of the min, either clip of y -- is also taken on some row
MODEL_SEEDS = (1, 2, 5)


def test_abi_symbols_and_struct_size():
    for name in ('pmg_td3_target_work_floats', 'pmg_td3_target_device'):
        assert name in PmgLibrary.SYMBOLS
    assert C.sizeof(PmgTd3Target) == 152                               # as sizeof(pmg_td3_target) in include/pmg.h on LP64


def test_model_pinned_draws():
    """the draws of row b under row_offset are those of pmg_act_env_device for global env row_offset + b: actor_cases' pinned integers"""
    p = AC.PINNED
    for off in (0, 1, 32):
        keep = [i for i, g in enumerate(p['g']) if off <= g <= 32]
        rows = [p['g'][i] - off for i in keep]
        u1, u2 = T3.draws(p['seed'], p['counter'], off, max(rows) + 1, p['A'])
        assert [int(x) for x in np.round(u1[rows, 0] * 2 ** 24)] == [AC.PINNED_U1[i] for i in keep]
        assert [int(x) for x in np.round(u2[rows, 1] * 2 ** 24)] == [AC.PINNED_U2[i] for i in keep]
    u1, u2 = T3.draws(p['seed'], p['counter'], 2 ** 31 - 1, 1, p['A'])
    assert int(round(u1[0, 0] * 2 ** 24)) == AC.PINNED_U1[3] and int(round(u2[0, 1] * 2 ** 24)) == AC.PINNED_U2[3]
    e = T3.noise32(u1, u2, T3.SIGMA, T3.NOISE_CLIP)
    assert np.abs(e - T3.noise64(u1, u2, T3.SIGMA, T3.NOISE_CLIP)).max() < 1e-6


def test_model_noise_bounds_and_statistics():
    """e = clip(sigma n, -c, c) over 2^16 draws (16384 rows x 4 columns), sigma = 0.2, c = 0.5 (k = c / sigma = 2.5): always within [-c, c];
    the sample mean, the sample second moment, the standard deviation and the share of clipped draws against the clipped normal's values.
    Bands: 5 standard errors of each statistic at N = 2^16 independent draws -- mean: 5 sqrt(m2 / N); second moment: 5 sqrt((m4 - m2^2) / N)
    (CLT); standard deviation: the second moment's band plus the square of the mean's, taken on the variance; share: 5 sqrt(p (1 - p) / N)
    (binomial) -- with m2, m4 and p the moments and the tail mass of the clipped standard normal.  Five standard errors are passed by a
    correct generator with probability 1 - 6e-7 per statistic."""
    n, A = 16384, 4
    N = n * A
    assert N == 2 ** 16
    sigma, c = float(np.float32(T3.SIGMA)), T3.NOISE_CLIP
    k = c / sigma
    m2, m4, p = T3.clipped_normal_moments(k)
    assert abs(p - 0.0124193) < 1e-6 and 0.9 < m2 < 1.0
    for seed, counter, off in ((0, 0, 0), (12345, 7, 32), (2 ** 63 + 5, 2 ** 40, 2 ** 33)):
        u1, u2 = T3.draws(seed, counter, off, n, A)
        for e in (T3.noise32(u1, u2, sigma, c).astype(np.float64), T3.noise64(u1, u2, sigma, c)):
            assert e.min() >= -c and e.max() <= c
            v = e.ravel() / sigma
            share = (np.abs(e.ravel()) == c).mean()
            print('seed %d counter %d offset %d: mean %.5f (band %.5f), second moment %.5f (want %.5f, band %.5f), clipped %.5f (want %.5f, band %.5f)' % (
                seed, counter, off, v.mean(), 5 * np.sqrt(m2 / N), (v ** 2).mean(), m2, 5 * np.sqrt((m4 - m2 ** 2) / N), share, p, 5 * np.sqrt(p * (1 - p) / N)))
            assert abs(v.mean()) < 5 * np.sqrt(m2 / N)
            assert abs((v ** 2).mean() - m2) < 5 * np.sqrt((m4 - m2 ** 2) / N)
            # the standard deviation of e: its square is the second moment less mean^2 <= 25 m2 / N, and |s - s0| (s + s0) = |s^2 - s0^2|
            std, std0 = e.ravel().std(), sigma * np.sqrt(m2)
            assert abs(std - std0) * (std + std0) < sigma ** 2 * (5 * np.sqrt((m4 - m2 ** 2) / N) + 25 * m2 / N), (std, std0)
            assert abs(share - p) < 5 * np.sqrt(p * (1 - p) / N)
    # an infinite clip leaves the noise alone, a zero clip leaves none
    u1, u2 = T3.draws(1, 2, 3, 64, 3)
    assert np.array_equal(T3.noise32(u1, u2, 0.2, np.inf), np.float32(0.2) * np.sqrt(np.float32(-2) * np.log(u1.astype(np.float32))) * np.cos(T3.TWO_PI32 * u2.astype(np.float32)))
    assert (T3.noise32(u1, u2, 0.2, 0.0) == 0).all()


def test_model_against_float64():
    """the float32 model against float64 torch of the same formula, fed the model's own n: y within grad_cases.MODEL_TOL of the float64 value
    relative to the largest |y64|, the min's choice and every clip predicate equal"""
    worst = 0.0
    for seed in MODEL_SEEDS:
        err, same, used = T3.model_vs_float64(seed)
        print('seed %d: largest |y32 - y64| / max |y64| = %.3g (bar %.3g), predicates equal: %s, every predicate taken: %s' % (seed, err, GC.MODEL_TOL, same, used))
        assert same and used, seed
        worst = max(worst, err)
    assert worst <= GC.MODEL_TOL, worst


def test_env_critic_td3_target_equals_the_model(emu_library):
    T3.case_host_face(emu_library)
