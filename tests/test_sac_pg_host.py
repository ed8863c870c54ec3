"""The fused SAC actor update, CPU only: the numpy model of tests/sac_pg_cases.py against float64 autograd, and the bars of that file
recomputed -- each is 4 x an error measured on the model alone."""
import numpy as np

import sac_pg_cases as SP
from pybullet_multigoal_gym_amd import _lib


def test_the_model_is_the_gradient():
    """model32 (the head, the exact chains, the selection, head_grad) against float64 autograd with the same n: equal ReLU masks, equal clamp
    predicates, equal critic selection (asserted inside), and the error the bar is made of"""
    err = SP.measure_model_bar()
    print('model32 against float64 autograd: %.3g' % err)
    assert 0.5 * SP.SAC_PG_MEASURED <= err <= SP.SAC_PG_MEASURED, err


def test_the_bars_are_the_measured_ones():
    ls, al = SP.measure_ls_bar(), SP.measure_alpha_bar()
    print('g_ls: %.3g, alpha: %.3g' % (ls, al))
    assert 0.5 * SP.SAC_PG_LS_MEASURED <= ls <= SP.SAC_PG_LS_MEASURED, ls
    assert 0.5 * SP.SAC_ALPHA_MEASURED <= al <= SP.SAC_ALPHA_MEASURED, al
    assert SP.SAC_PG_LS_TOL == 4 * SP.SAC_PG_LS_MEASURED and SP.SAC_PG_TOL == 4 * SP.SAC_PG_MEASURED and SP.SAC_ALPHA_TOL == 4 * SP.SAC_ALPHA_MEASURED


def test_head_grad_against_actor_head_grad():
    """head_grad with e = alpha / B is the old recipe's host fix-up up to rounding: the same clamp predicate, zeros outside it"""
    from pybullet_multigoal_gym_amd.sac import actor_head_grad
    rs = np.random.RandomState(3)
    B, A = 37, 4
    a, n, ga = np.tanh(rs.standard_normal((B, A))).astype(np.float32), rs.standard_normal((B, A)).astype(np.float32), (rs.standard_normal((B, A)) / B).astype(np.float32)
    z = (rs.standard_normal((B, 2 * A)) * 3).astype(np.float32)
    g_mu, g_ls, inr, _ = SP.head_grad(a, ga, np.float32(1.0 / B) * np.float32(0.2), n, z, -2.0, 0.5)
    old = actor_head_grad(a, n, z, ga, 0.2, -2.0, 0.5)
    assert inr.any() and not inr.all() and np.array_equal(old[:, A:] == 0, ~inr)
    got = np.concatenate([g_mu, g_ls], 1)
    assert np.abs(got - old).max() <= 1e-6 * np.abs(old).max()


def test_the_temperature_chains():
    """alpha_total is two chains, not numpy's pairwise sum: a case where they differ, and the value of a case small enough to follow by hand"""
    assert SP.alpha_total(np.array([1.0, 2.0, 3.0], np.float32)) == 6.0
    logp = np.full(1000, 0.1, np.float32)
    logp[0] = 1e8
    assert SP.alpha_total(logp) != np.float32(logp.sum(dtype=np.float64))
    g = SP.alpha_g(np.array([-1.0, -3.0], np.float32), -1.5)
    assert g == np.float32(3.5)


def test_the_library_names_the_new_entry_points():
    for name in ('pmg_sac_policy_grad_work_floats', 'pmg_sac_policy_grad_device', 'pmg_sac_alpha_device'):
        assert name in _lib.PmgLibrary.SYMBOLS
    assert _lib.C.sizeof(_lib.PmgSacPolicyGrad) % 8 == 0 and _lib.C.sizeof(_lib.PmgSacAlpha) % 8 == 0
