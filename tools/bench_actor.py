#!/usr/bin/env python3
"""Time of the actor on the device (pmg_act_env_device / pmg_mlp_forward_device: pmg_k_mlp) next to its yardsticks,
existing code timed in the SAME process: the step alone (pmg_step_device on uploaded U(-1, 1) actions, eight tables in turn), step +
act (the rollout of two calls per step), and pmg_policy_input_env_device as the floor of a single launch over the same rows.  Both
rollouts run bench.py's workload: 50-step episodes, pmg_reset_done_device after every step inside the timed region; step + act runs
with random_eps = 1, so that its actions are U(-1, 1) like the yardstick's (the network and the noise are evaluated all the same) and
the two step the same distribution of states.

  networks: policy_state | goal -> 256 -> 256 -> 256 -> action_dim (tanh), for reach, push and block_stack-4, at 4096 and
  131072 envs; noise_eps = 0.2, random_eps = 0.3, the counter advances with every launch.  pmg_mlp_forward_device: the same
  network shape on B = 2^20 contiguous rows.

Reported: ms per launch (median round [lowest .. highest]) and the FLOP rate (2 x weights per row) against the 157.3 TF f32
matrix peak.  `bench_actor.py [--out profiles/actor_forward.txt] [--rounds 5] [--reps 20]`"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pybullet_multigoal_gym_amd as pmg
from pybullet_multigoal_gym_amd._lib import PMG_NORM_GOAL, PMG_NORM_POLICY_STATE

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'actor_forward.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--envs', type=int, nargs='+', default=[4096, 131072])
ap.add_argument('--batch', type=int, default=1 << 20)
ap.add_argument('--hidden', type=int, default=256)
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'
PEAK_TF = 157.3


def timed(h, launch):
    """-> ms per launch of every round"""
    for _ in range(args.warmup):
        launch()
    h.sync()
    out = []
    for _ in range(args.rounds):
        h.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            launch()
        h.sync()
        out.append((time.perf_counter() - t0) / args.reps * 1e3)
    return out


def stats(ms):
    return {'ms_median': float(np.median(ms)), 'ms_min': float(min(ms)), 'ms_max': float(max(ms))}


def upload_net(h, widths, rs):
    d_w, d_b = [], []
    for l in range(len(widths) - 1):
        w = (rs.uniform(-1, 1, (widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32)
        b = rs.uniform(-0.1, 0.1, widths[l + 1]).astype(np.float32)
        for a, out in ((w, d_w), (b, d_b)):
            p = h.device_alloc(a.nbytes)
            h.upload(p, a)
            out.append(p)
    return h.mlp_struct(widths, d_w, d_b, 1), d_w + d_b


def flops(widths):
    return 2 * sum(widths[l] * widths[l + 1] for l in range(len(widths) - 1))


def bench(task, kw, N):
    env = pmg.make_env(task=task, num_envs=N, seed=0, seed_stride=1, max_episode_steps=50, **kw)
    h, d = env.handle, env.handle.dims
    rs = np.random.RandomState(0)
    kind, A = PMG_NORM_POLICY_STATE, d.action_dim
    W0 = d.policy_state_dim + d.goal_dim
    h.norm_update(kind, rs.uniform(-1, 1, (4096, d.policy_state_dim)).astype(np.float32))
    h.norm_update(PMG_NORM_GOAL, rs.uniform(-1, 1, (4096, d.goal_dim)).astype(np.float32))
    widths = [W0] + [args.hidden] * 3 + [A]
    mlp, ptrs = upload_net(h, widths, rs)
    env.reset()
    d_act, d_x = h.device_alloc(4 * N * A), h.device_alloc(4 * N * W0)
    d_fix = [h.device_alloc(4 * N * A) for _ in range(8)]
    for p in d_fix:
        h.upload(p, rs.uniform(-1, 1, (N, A)).astype(np.float32))
    ex, ex_all = h.explore_struct(0.2, 0.3, 1, 0), h.explore_struct(0.2, 1.0, 2, 0)
    turn = [0]

    def act():
        ex.counter += 1
        h.act_env_device(mlp, kind, d_act, None, ex)

    def step():
        turn[0] += 1
        h.step_device(d_fix[turn[0] % 8])
        h.reset_done_device()

    def step_act():
        ex_all.counter += 1
        h.act_env_device(mlp, kind, d_act, None, ex_all)
        h.step_device(d_act)
        h.reset_done_device()
    res = {'task': task, 'N': N, 'widths': widths, 'flop_per_row': flops(widths)}
    res['policy_input'] = stats(timed(h, lambda: h.policy_input_env_device(kind, d_x)))
    res['act'] = stats(timed(h, act))
    res['act']['TF'] = N * flops(widths) / (res['act']['ms_median'] * 1e-3) / 1e12
    env.reset()
    res['step'] = stats(timed(h, step))
    env.reset()
    res['step_act'] = stats(timed(h, step_act))
    for p in ptrs + d_fix + [d_act, d_x]:
        h.device_free(p)
    env.close()
    return res


def bench_forward(B):
    env = pmg.make_env(task='reach', num_envs=64)
    h = env.handle
    rs = np.random.RandomState(1)
    widths = [6] + [args.hidden] * 3 + [3]
    mlp, ptrs = upload_net(h, widths, rs)
    d_in, d_out = h.device_alloc(4 * B * widths[0]), h.device_alloc(4 * B * widths[-1])
    a = rs.uniform(-1, 1, (1 << 16, widths[0])).astype(np.float32)
    for o in range(0, B, 1 << 16):
        h.upload(d_in + 4 * o * widths[0], a[:min(1 << 16, B - o)])
    res = {'B': B, 'widths': widths, 'flop_per_row': flops(widths)}
    res['forward'] = stats(timed(h, lambda: h.mlp_forward_device(mlp, d_in, widths[0], B, d_out, widths[-1])))
    res['forward']['TF'] = B * flops(widths) / (res['forward']['ms_median'] * 1e-3) / 1e12
    for p in ptrs + [d_in, d_out]:
        h.device_free(p)
    env.close()
    return res


fmt = lambda s: '%.4f ms [%.4f .. %.4f]' % (s['ms_median'], s['ms_min'], s['ms_max'])
res = {'act': [bench(t, kw, N) for t, kw in (('reach', {}), ('push', {}), ('block_stack', {'num_block': 4})) for N in args.envs],
       'forward': bench_forward(args.batch)}
lines = ['# tools/bench_actor.py: pmg_act_env_device (policy_state | goal -> 3 x %d -> action_dim, tanh, noise_eps 0.2, random_eps 0.3) next to' % args.hidden,
         '# the step alone, step + act, and pmg_policy_input_env_device (the floor of one launch over the same rows), same process',
         '# median of %d rounds x %d launches [lowest .. highest round]; TF against the %.1f TF f32 matrix peak' % (args.rounds, args.reps, PEAK_TF)]
for r in res['act']:
    lines.append('%s x %d (%s, %d FLOP per env): act %s = %.2f TF (%.1f %% of peak); policy_input %s; step %s; step + act %s = step + %.4f ms (%.1f %%)' %
                 (r['task'], r['N'], ' -> '.join(str(w) for w in r['widths']), r['flop_per_row'], fmt(r['act']), r['act']['TF'], 100 * r['act']['TF'] / PEAK_TF,
                  fmt(r['policy_input']), fmt(r['step']), fmt(r['step_act']), r['step_act']['ms_median'] - r['step']['ms_median'],
                  100 * (r['step_act']['ms_median'] / r['step']['ms_median'] - 1)))
f = res['forward']
lines.append('pmg_mlp_forward_device B = %d (%s): %s = %.2f TF (%.1f %% of peak)' %
             (f['B'], ' -> '.join(str(w) for w in f['widths']), fmt(f['forward']), f['forward']['TF'], 100 * f['forward']['TF'] / PEAK_TF))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
