"""SAC's Gaussian head and soft target on the CPU tier: the cases of tests/sac_cases.py on the g++ build of the product sources (pmg_k_sac and
pmg_k_sac_target with the fmaf body of the matrix step) over the fiber emulator, through the C ABI.  The emulator proves the head's column
map, the sum of log pi, the rebuild of x' | a' in front of either critic from d_next_action and from the workspace (the route that avoids
the hand-over hazard of Dx < A), the padding, the min and the soft epilogue; the lane maps of the MFMA and the build's logf / sqrtf / cosf /
expf / tanhf / log1pf are proven by tests/test_gpu_sac.py."""
import numpy as np
import pytest

import sac_cases as SC
import td3_cases as T3
from actor_cases import network
from normalizer_cases import handle
from td_cases import eq_bits


@pytest.mark.parametrize('case', SC.SAMPLE_CASES)
def test_sample(emu_library, case):
    SC.case_sample(emu_library, (case,))


def test_sample_covers_the_clamp_and_saturation(emu_library):
    """over the (cheap) cases without the 3 x 256 networks: log-stds below, inside and above the clamp and saturated actions all occur"""
    seen = set()
    for Dx, A, hidden in SC.SAMPLE_CASES:
        m = SC.sample_case(Dx, A, hidden)
        raw = m['z'][:, A:]
        seen |= {s for s, hit in (('below', raw < SC.LS_LO), ('inside', (raw > SC.LS_LO) & (raw < SC.LS_HI)), ('above', raw > SC.LS_HI)) if hit.any()}
    assert seen == {'below', 'inside', 'above'}
    sat = 0
    with handle(emu_library, 'reach', num_envs=8) as env:
        for k, (Dx, A, hidden) in enumerate(SC.SAMPLE_CASES):
            if len(hidden) > 1:
                continue
            m = SC.sample_case(Dx, A, hidden)
            seed, counter, off = SC.SEEDS(k)
            got = SC.device_sample(env.handle, m['Ws'], m['bs'], m['x'], seed=seed, counter=counter, row_offset=off)
            hit = (np.abs(got['a']) == 1).any(1)
            sat += int(hit.sum())
            assert np.isfinite(got['logp'][hit]).all()
    assert sat > 0


def test_sample_properties(emu_library):
    SC.case_sample_properties(emu_library)


def test_widest_head(emu_library):
    """A = 128 with Dx = 128 (emulator only): the head's pass covers 16 rounds of 256 threads, Dx + A = 256 fills the tile"""
    Dx = A = 128
    Ws, bs = network(1990, (Dx, 2 * A))
    Ws[0] = Ws[0] * np.float32(0.125)
    x = np.random.RandomState(5).uniform(-1, 1, (33, Dx)).astype(np.float32)
    z = SC.forward(x, Ws, bs)
    nets = T3.critics(1991, Dx, A, (33,), ())
    r = np.zeros(33, np.float32)
    with handle(emu_library, 'reach', num_envs=8) as env:
        h = env.handle
        got = SC.device_sample(h, Ws, bs, x, -2.0, 0.5, seed=1, counter=2, row_offset=3)
        SC.check_z(got['z'], z, 'z')
        SC.check_head(got, z, *SC.draws(1, 2, 3, 33, A), -2.0, 0.5, 'A = 128')
        m = {'Ws': Ws, 'bs': bs}
        for null in ((), ('a',)):
            t = SC.device_sac_target(h, Ws, bs, *nets, x=x, r=r, ls_lo=-2.0, ls_hi=0.5, seed=1, counter=2, row_offset=3, null=null)
            if not null:
                SC.check_target(h, t, m, nets, x, r, 0.98, -SC.INF, SC.INF, None, 0.2, (1, 2, 3), 'A = 128', ls=(-2.0, 0.5))
                full = t
            else:
                for k in ('y', 'q1', 'q2', 'logp'):
                    eq_bits(t[k], full[k], ('workspace', k))


@pytest.mark.parametrize('task', ('reach', 'push'))
def test_env_acting(emu_library, task):
    SC.case_env(emu_library, task)


def test_target(emu_library):
    SC.case_target(emu_library)                                  # every pair (Dx, A); q1 < q2 and q2 < q1 both occur


@pytest.mark.parametrize('pair', SC.PAIRS)
def test_target_without_noise_and_temperature_is_td3(emu_library, pair):
    SC.case_target_is_td3(emu_library, (pair,))


def test_epilogue(emu_library):
    SC.case_epilogue(emu_library)


def test_stale_tile_contents(emu_library):
    SC.case_stale_tile(emu_library)


def test_invalid_calls(emu_library):
    SC.case_invalid_calls(emu_library)
