#!/usr/bin/env python3
"""HBM throughput of the policy-input kernel (pmg_k_policy_input) next to its yardstick, the G = 3 reward
kernel, measured in the SAME process; and the cost of a normaliser update of the env rows next to one batched step.

  policy input: contiguous state | goal rows resident in HBM, push (7 | 3, policy_state) and block_stack-4 (72 | 12,
                observation); B chosen so that a call moves >= 1 GiB; algorithmic bytes = 2 * 4 * B * (Ds + Dg)
  reward:       pmg_compute_reward_device, G = 3, 64 Mi pairs, 8 G + 5 bytes per pair
  env update:   pmg_norm_update_env_device at 4096 envs (reach) against pmg_step_device

Every figure: ROUNDS rounds of REPS launches each (after WARMUP launches), a round bracketed by a device sync and a host
clock; reported as the median round with the lowest and highest (the run-to-run spread).
`bench_norm.py [--out profiles/norm_policy_input.txt] [--rounds 5] [--reps 20]`"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pybullet_multigoal_gym_amd as pmg
from pybullet_multigoal_gym_amd._lib import PMG_NORM_OBSERVATION, PMG_NORM_POLICY_STATE

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'norm_policy_input.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--reward-pairs', type=int, default=1 << 26)
args = ap.parse_args()
assert args.reps >= 20, 'at least 20 timed repetitions per round'


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


def summary(ms, nbytes):
    tb = sorted(nbytes / (m * 1e-3) / 1e12 for m in ms)
    return {'ms_median': float(np.median(ms)), 'TB_per_s_median': float(np.median(tb)), 'TB_per_s_min': tb[0], 'TB_per_s_max': tb[-1],
            'spread_TB_per_s': tb[-1] - tb[0], 'bytes_per_call': int(nbytes), 'rounds': args.rounds, 'launches_per_round': args.reps}


def fill(h, d_ptr, rows, width, rs, chunk=1 << 20):
    """random float32 rows on the device, one host chunk uploaded over and over (the values do not matter to the bandwidth)"""
    a = rs.uniform(-3, 3, (min(chunk, rows), width)).astype(np.float32)
    for o in range(0, rows, chunk):
        n = min(chunk, rows - o)
        h.upload(d_ptr + 4 * o * width, a[:n])
    return a


def bench_policy_input(task, kw, kind, name):
    env = pmg.make_env(task=task, num_envs=64, **kw)
    h = env.handle
    Ds, Dg = h.norm_width(kind), h.dims.goal_dim
    W = Ds + Dg
    B = -(-(1 << 30) // (8 * W))
    B = -(-B // 4096) * 4096                                  # >= 1 GiB per call
    rs = np.random.RandomState(0)
    h.norm_update(kind, rs.uniform(-3, 3, (4096, Ds)).astype(np.float32))
    h.norm_update(2, rs.uniform(-3, 3, (4096, Dg)).astype(np.float32))
    d_s, d_g, d_o = h.device_alloc(4 * B * Ds), h.device_alloc(4 * B * Dg), h.device_alloc(4 * B * W)
    s0, g0 = fill(h, d_s, B, Ds, rs), fill(h, d_g, B, Dg, rs)
    ms = timed(h, lambda: h.policy_input_device(kind, d_s, Ds, d_g, Dg, B, d_o))
    n = min(len(s0), 1 << 16)                                 # spot check against the host variant (bit-equal)
    got = np.empty((n, W), np.float32)
    h.download(got, d_o)
    assert np.array_equal(got, h.policy_input(kind, s0[:n], g0[:n]))
    for p in (d_s, d_g, d_o):
        h.device_free(p)
    env.close()
    return dict(summary(ms, 8 * B * W), kernel='pmg_k_policy_input', case=name, rows=B, state_width=Ds, goal_width=Dg,
                row_width_multiple_of_4=(W % 4 == 0))


def bench_reward(B):
    env = pmg.make_env(task='reach', num_envs=64)
    h = env.handle
    rs = np.random.RandomState(1)
    d_a, d_d, d_r, d_k = h.device_alloc(12 * B), h.device_alloc(12 * B), h.device_alloc(4 * B), h.device_alloc(B)
    fill(h, d_a, B, 3, rs)
    fill(h, d_d, B, 3, rs)
    lib = h.L.lib

    def launch():
        assert lib.pmg_compute_reward_device(h.h, C.c_void_p(d_a), C.c_void_p(d_d), C.c_int64(B), C.c_void_p(d_r), C.c_void_p(d_k)) == 0
    ms = timed(h, launch)
    for p in (d_a, d_d, d_r, d_k):
        h.device_free(p)
    env.close()
    return dict(summary(ms, B * 29), kernel='pmg_k_reward3', pairs=B)


def bench_env_update(N=4096):
    env = pmg.make_env(task='reach', num_envs=N, seed=0, seed_stride=1)
    h = env.handle
    env.reset()
    d_act = h.device_alloc(4 * N * 3)
    h.upload(d_act, np.random.RandomState(2).uniform(-1, 1, (N, 3)).astype(np.float32))
    d_out = h.device_alloc(4 * N * 6)
    # bench.py's loop: a step, then the device-side reset of the envs whose TimeLimit ran out
    step = timed(h, lambda: (h.step_device(d_act), h.reset_done_device()))
    both = timed(h, lambda: (h.step_device(d_act), h.reset_done_device(), h.norm_update_env_device(None)))
    upd = timed(h, lambda: h.norm_update_env_device(None))
    pin = timed(h, lambda: h.policy_input_env_device(PMG_NORM_POLICY_STATE, d_out))
    h.device_free(d_act)
    h.device_free(d_out)
    env.close()
    med = lambda v: float(np.median(v))
    return {'envs': N, 'task': 'reach', 'step_device_ms': med(step), 'step_plus_norm_update_env_ms': med(both),
            'norm_update_env_device_alone_ms': med(upd), 'policy_input_env_device_alone_ms': med(pin), 'step_ms_rounds': step, 'step_plus_update_ms_rounds': both,
            'update_alone_ms_rounds': upd, 'launches_per_update': 6}


res = {'policy_input': [bench_policy_input('push', {}, PMG_NORM_POLICY_STATE, 'push 7 | 3 (policy_state | goal)'),
                        bench_policy_input('block_stack', {'num_block': 4}, PMG_NORM_OBSERVATION, 'block_stack-4 72 | 12 (observation | goal)')],
       'reward_G3': bench_reward(args.reward_pairs)}
res['env_update'] = bench_env_update()
rw = res['reward_G3']
lines = ['# tools/bench_norm.py: policy-input kernel against the G = 3 reward kernel, same process (TB/s, algorithmic bytes)',
         '# median of %d rounds x %d launches [lowest .. highest round]' % (args.rounds, args.reps),
         'reward G=3, %d pairs, %d B per call: %.3f TB/s [%.3f .. %.3f], spread %.3f' %
         (rw['pairs'], rw['bytes_per_call'], rw['TB_per_s_median'], rw['TB_per_s_min'], rw['TB_per_s_max'], rw['spread_TB_per_s'])]
for p in res['policy_input']:
    lines.append('policy input %s, %d rows, %d B per call: %.3f TB/s [%.3f .. %.3f], spread %.3f = %.2f x reward (short by %.3f TB/s; reward spread %.3f)' %
                 (p['case'], p['rows'], p['bytes_per_call'], p['TB_per_s_median'], p['TB_per_s_min'], p['TB_per_s_max'], p['spread_TB_per_s'],
                  p['TB_per_s_median'] / rw['TB_per_s_median'], rw['TB_per_s_median'] - p['TB_per_s_median'], rw['spread_TB_per_s']))
eu = res['env_update']
lines.append('reach x %d (step = pmg_step_device + pmg_reset_done_device): step %.4f ms, step + norm_update_env_device %.4f ms, '
             'norm_update_env_device alone %.4f ms, policy_input_env_device alone %.4f ms per call' %
             (eu['envs'], eu['step_device_ms'], eu['step_plus_norm_update_env_ms'], eu['norm_update_env_device_alone_ms'], eu['policy_input_env_device_alone_ms']))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
