#!/usr/bin/env python3
"""The documented PPO recipe (pybullet_multigoal_gym_amd/ppo.py) end to end on dense-reward reach: a device-resident rollout of
N envs x T steps with the Gaussian actor, the recorded rows through the normaliser, the value network, GAE with reward and done read in place
from the recorded packed rows, advantage normalisation, then K epochs of minibatches of policy_grad + Adam on the actor and
grad(d_target = ret) + Adam on the value network.  Nothing is computed on the host between the reset and the end of an iteration; the host
only reads back, once per iteration, the rewards (for the mean episode return printed here) and the minibatch statistics.

Evidence that the calls compose, not a test and not a tuned learner: no pass bar.
`ppo_reach.py [--envs 256] [--iters 20] [--out profiles/ppo_reach.txt] [--library tests/emu/libpmg_emu.so]`"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pybullet_multigoal_gym_amd as pmg
from pybullet_multigoal_gym_amd.actor import Actor

ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=256)
ap.add_argument('--steps', type=int, default=50, help='T: steps per rollout = steps per episode, so every rollout is one episode per env')
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--epochs', type=int, default=4)
ap.add_argument('--minibatch', type=int, default=3200)
ap.add_argument('--hidden', type=int, default=64)
ap.add_argument('--lr', type=float, default=1e-3)
ap.add_argument('--gamma', type=float, default=0.98)
ap.add_argument('--lam', type=float, default=0.95)
ap.add_argument('--clip', type=float, default=0.2)
ap.add_argument('--ent-coef', type=float, default=0.0)
ap.add_argument('--vf-coef', type=float, default=0.5)
ap.add_argument('--out', default=None)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
N, T, B = args.envs, args.steps, args.minibatch
assert (N * T) % B == 0, 'the minibatch must divide the rollout'

from pybullet_multigoal_gym_amd._lib import PMG_NORM_POLICY_STATE, PmgLibrary
env = pmg.make_env(task='reach', num_envs=N, binary_reward=False, max_episode_steps=T, seed=1, seed_stride=1,
                   **({'_library': PmgLibrary(args.library)} if args.library else {}))
h, dims = env.handle, env.dims
A, P = dims.action_dim, dims.packed_dim
Ds, G = dims.policy_state_dim, dims.goal_dim
Dx = Ds + G
so, dgo = dims.observation_dim, dims.observation_dim + Ds + G                     # columns of policy_state and desired_goal in a packed row
col_r = dims.observation_dim + Ds + 2 * G                                           # reward | goal_achieved | done
col_done = col_r + 2
rs = np.random.RandomState(0)


def net(widths, last_scale):
    Ws = [(rs.uniform(-1, 1, (widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32) for l in range(len(widths) - 1)]
    Ws[-1] *= np.float32(last_scale)
    return Ws, [np.zeros(w.shape[0], np.float32) for w in Ws]


pi, vf, ppo = env.gaussian_actor, Actor(env), env.ppo
Wp, bp = net([Dx, args.hidden, args.hidden, 2 * A], 0.01)
bp[-1][A:] = -0.5                                                                   # initial std about 0.6
pi.load(Wp, bp)
vf.load(*net([Dx, args.hidden, args.hidden, 1], 1.0), out_activation='identity')
sa, sv = pi.adam_state(), vf.adam_state()
LS = (-3.0, 0.5)
f4 = lambda n: h.device_alloc(4 * int(n))
d_act, d_rows, d_succ = f4(N * A), f4(T * N * P), f4(T * N * P)
d_n, d_zo, d_x, d_xs = f4(T * N * A), f4(T * N * 2 * A), f4(T * N * Dx), f4(T * N * Dx)
d_v, d_vs, d_adv, d_ret, d_stats = f4(T * N), f4(T * N), f4(T * N), f4(T * N), f4(2)
d_rho, d_lr, d_cl, d_st = f4(B), f4(B), h.device_alloc(B), f4(4)
R = 256 if B >= 1024 else None
pwork, vwork = ppo.policy_grad_work_floats(pi, B, R), vf.grad_work_floats(B, R)
d_pwork, d_vwork = f4(pwork), f4(vwork)
lines = ['# tools/ppo_reach.py: PPO on dense-reward reach, %d envs x %d steps per iteration, %d epochs of minibatches of %d, actor %d -> 2 x %d -> %d, lr %g, clip %g, '
         'gamma %g, lambda %g' % (N, T, args.epochs, B, Dx, args.hidden, 2 * A, args.lr, args.clip, args.gamma, args.lam),
         '# iteration: mean episode return (sum of the %d rewards of an episode, mean over the envs) | mean final distance | approximate KL, clip fraction of the last minibatch | s' % T]
counter = 0
env.reset()                                                                         # T = max_episode_steps: every rollout starts and ends with its episodes
for t in range(T):                                                                  # the normaliser sees one rollout of the initial policy, then stays fixed
    h.norm_update_env_device()
    pi.act_device(d_act, seed=5, counter=t, ls_lo=LS[0], ls_hi=LS[1])
    h.step_device(d_act)
    h.reset_done_device()
for it in range(args.iters):
    t0 = time.perf_counter()
    for t in range(T):
        h.device_copy(d_rows + 4 * t * N * P, h.device_ptr(), 4 * N * P)           # s_t: the rows the action is drawn from
        pi.act_device(d_act, seed=7, counter=counter, d_noise=d_n + 4 * t * N * A, d_preact=d_zo + 4 * t * N * 2 * A, ls_lo=LS[0], ls_hi=LS[1])
        counter += 1
        h.step_device(d_act)
        h.device_copy(d_succ + 4 * t * N * P, h.device_ptr(), 4 * N * P)           # s'_t, reward, done: BEFORE any reset
        h.reset_done_device()
    h.policy_input_device(PMG_NORM_POLICY_STATE, d_rows + 4 * so, P, d_rows + 4 * dgo, P, T * N, d_x)
    h.policy_input_device(PMG_NORM_POLICY_STATE, d_succ + 4 * so, P, d_succ + 4 * dgo, P, T * N, d_xs)
    h.mlp_forward_device(vf._loaded(), d_x, Dx, T * N, d_v, 1)
    h.mlp_forward_device(vf._loaded(), d_xs, Dx, T * N, d_vs, 1)
    ppo.gae_device(T, N, (d_succ + 4 * col_r, N * P, P), (d_v, N, 1), (d_vs, N, 1), (d_adv, N, 1), args.gamma, args.lam,
                   cut=(d_succ + 4 * col_done, N * P, P), ret=(d_ret, N, 1))
    ppo.normalize_advantages_device(d_adv, T * N, d_stats)
    for epoch in range(args.epochs):
        for lo in range(0, T * N, B):
            ppo.policy_grad_device(pi, B, d_x + 4 * lo * Dx, d_zo + 4 * lo * 2 * A, d_n + 4 * lo * A, d_adv + 4 * lo, d_pwork, pwork, args.clip, args.ent_coef,
                                   grads=sa.g, d_ratio=d_rho, d_logratio=d_lr, d_clipped=d_cl, ls_lo=LS[0], ls_hi=LS[1], chunk_rows=R)
            pi.adam_step_device(sa.g, sa, args.lr)
            vf.grad_device(B, d_x + 4 * lo * Dx, Dx, d_vwork, vwork, d_target=d_ret + 4 * lo, gscale=args.vf_coef / B, grads=sv.g, chunk_rows=R)
            vf.adam_step_device(sv.g, sv, args.lr)
    ppo.stats_device(B, d_rho, d_lr, d_cl, d_adv + 4 * (T * N - B), d_st, args.clip)
    h.sync()
    rows, st = np.empty((T, N, P), np.float32), np.empty(4, np.float32)
    h.download(rows, d_succ)
    h.download(st, d_st)
    assert rows[-1, :, col_done].all() and not rows[:-1, :, col_done].any()
    lines.append('%3d: %8.3f | %.4f | %.4f %.3f | %.2f' % (it, rows[:, :, col_r].sum(0).mean(), -rows[-1, :, col_r].mean(), st[0], st[1], time.perf_counter() - t0))
    print(lines[-1], flush=True)
env.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
