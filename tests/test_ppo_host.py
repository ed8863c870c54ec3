"""The PPO calls, CPU only: the numpy models of tests/ppo_cases.py against float64 (autograd for the gradient), the bars of that file
recomputed -- each is 4 x an error measured on the model alone --, the margins and the coverage of the cases asserted on the float64 model, and
why GAE takes the successor's value as a table of its own."""
import numpy as np

import ppo_cases as PP
from pybullet_multigoal_gym_amd import _lib

F32, F64 = np.float32, np.float64


def test_the_model_is_the_gradient():
    """model32 (the chain, head32, the exact backward chains) against float64 autograd of the textbook loss: equal ReLU masks, clamp predicates and
    clipped rows (asserted inside), and the error the bar is made of"""
    err = PP.measure_model_bar()
    print('model32 against float64 autograd: %.3g' % err)
    assert 0.5 * PP.PPO_MEASURED <= err <= PP.PPO_MEASURED, err
    assert PP.PPO_TOL == 4 * PP.PPO_MEASURED


def test_the_bars_are_the_measured_ones():
    head, inv = PP.measure_head_bars(), PP.measure_inv_bar()
    print('lr %.3g, rho %.3g, g_mu %.3g, g_ls %.3g; 1 / (std + eps) %.3g' % (tuple(head) + (inv,)))
    for got, const in zip(head + [inv], (PP.PPO_LR_MEASURED, PP.PPO_RHO_MEASURED, PP.PPO_MU_MEASURED, PP.PPO_LS_MEASURED, PP.ADV_INV_MEASURED)):
        assert 0.5 * const <= got <= const, (got, const)
    assert (PP.PPO_LR_TOL, PP.PPO_RHO_TOL, PP.PPO_MU_TOL, PP.PPO_LS_TOL, PP.ADV_INV_TOL) == tuple(
        4 * v for v in (PP.PPO_LR_MEASURED, PP.PPO_RHO_MEASURED, PP.PPO_MU_MEASURED, PP.PPO_LS_MEASURED, PP.ADV_INV_MEASURED))


def test_every_row_keeps_its_margins_and_the_cases_cover_every_branch():
    """on the float64 model: no rho within RHO_MARGIN of an end of the clip, no raw log-std of either policy within LS_MARGIN of an end of the
    clamp, no |adv| below ADV_MARGIN -- every row of every case, none left out; and clipped rows on both sides, unclipped rows on both sides of 1
    and log-stds below, inside and above the clamp for both policies all occur"""
    for c in [PP.ppo_case(k) for k in range(len(PP.CASES))] + [PP.model_case(k) for k in range(len(PP.MODEL_NETS))]:
        w = PP.head64(c['z'], *PP.head_args(c))
        near, tight, small = PP.margins_ok(w, c['adv'], c['lo'], c['hi'])
        assert not near.any() and not tight and not small
        assert w['rho'].shape == (c['x'].shape[0],) and np.isfinite(w['rho']).all()
    assert PP.model_coverage() == PP.COVERAGE


def test_gae_model_against_the_textbook_recursion():
    """the fmaf chain against delta_t + gamma lambda (1 - cut_t) A_{t+1} in float64, with terminals"""
    c = PP.gae_inputs(7, 65)
    gamma, lam = 0.98, 0.95
    adv, ret = PP.gae_model(c['r'], c['vtab'][:7], c['succ'], gamma, lam, c['cut'], c['term'])
    run, want = np.zeros(65), np.zeros((7, 65))
    g, gl = float(F32(gamma)), float(F32(F32(gamma) * F32(lam)))
    for t in range(6, -1, -1):
        delta = c['r'][t].astype(F64) + g * np.where(c['term'][t] != 0, 0.0, c['succ'][t].astype(F64)) - c['vtab'][t].astype(F64)
        run = delta + (0.0 if t == 6 else gl * np.where(c['cut'][t] != 0, 0.0, run))
        want[t] = run
    assert np.abs(adv - want).max() <= 1e-5 and np.abs(ret - (want + c['vtab'][:7])).max() <= 1e-5
    assert PP.gae_model(c['r'], c['vtab'][:7], c['succ'], 0.0, lam)[0].tolist() == (c['r'] - c['vtab'][:7]).tolist()       # gamma = 0: r - V


def test_a_reset_style_store_needs_the_successor_table():
    """With a store whose row t + 1 holds the NEW episode's first state behind an episode's end, the shifted value table bootstraps the finished
    episode from the wrong state; the successor table gives the per-episode reference.  This is why pmg_gae_device takes d_value_next."""
    r, vtab, succ, cut, gamma, lam, want = PP.reset_store_case()
    right = PP.gae_model(r, vtab[:5], succ, gamma, lam, cut)[0][:, 0]
    wrong = PP.gae_model(r, vtab[:5], vtab[1:6], gamma, lam, cut)[0][:, 0]
    assert np.abs(right - want).max() <= 1e-6
    assert np.abs(wrong - want)[:3].min() > 0.5                     # every step of the finished episode inherits the error: gamma (2.0 - (-0.7)) at its end
    assert np.abs(wrong - want)[3:].max() <= 1e-6                   # the episode behind it is not touched
    no_cut = PP.gae_model(r, vtab[:5], succ, gamma, lam)[0][:, 0]
    assert np.abs(no_cut - want)[:3].max() > 1e-3                   # and the cut is needed beside it


def test_the_chains_are_chains():
    """chain256 is two levels of ascending sums, not numpy's pairwise sum; stats_model's mean of a case small enough to follow by hand"""
    x = np.full(1000, 0.1, F32)
    x[0] = 1e8
    assert PP.chain256(x, F32) != F32(x.sum(dtype=F64))
    mean, inv, inv64 = PP.stats_model(np.array([1.0, 2.0, 3.0, 6.0], F32), 0.0, 1)
    assert mean == 3.0 and abs(inv64 - 1.0 / np.sqrt(14.0 / 3.0)) < 1e-15 and inv == F32(inv64)
    s = PP.ppo_stats_model(np.array([1.0, 2.0], F32), np.array([0.0, 0.5], F32), np.array([0, 3]), np.array([1.0, -1.0], F32), 0.8, 1.2)
    assert s.tolist() == [0.25, 0.5, -0.5, 0.25]                   # ((0) + (1 - 0.5)) / 2; 1 of 2; (min(1, 1) + min(-2, -1.2)) / 2; 0.5 / 2


def test_the_library_names_the_new_entry_points():
    for name in ('pmg_gae_device', 'pmg_adv_stats_device', 'pmg_adv_apply_device', 'pmg_ppo_policy_grad_work_floats', 'pmg_ppo_policy_grad_device',
                 'pmg_ppo_stats_device'):
        assert name in _lib.PmgLibrary.SYMBOLS
    for s in (_lib.PmgGae, _lib.PmgAdvStats, _lib.PmgPpoPolicyGrad, _lib.PmgPpoStats):
        assert _lib.C.sizeof(s) % 8 == 0
    assert _lib.C.sizeof(_lib.PmgGae) == 32 + 7 * 24 and _lib.C.sizeof(_lib.PmgAdvStats) == 40
