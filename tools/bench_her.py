#!/usr/bin/env python3
"""Time of one HER minibatch (pmg_her_sample_device: pmg_k_her_draw + pmg_k_her_rows) next to its yardstick,
existing code timed in the SAME process: pmg_policy_input_device twice on CONTIGUOUS rows of the same widths and B, and
pmg_compute_reward_device on B pairs -- the unfused chain without its gather, a lower bound of what a caller could do
before.

  push (policy_state 7 | goal 3, packed rows of 36 floats) and block_stack-4 (observation 72 | goal 12, 115 floats),
  B = 2^20, T = 50, time-major tables [T + 1, E, P]: one that fits an XCD's L2 share (<= 2 MiB) and one of >= 512 MiB,
  beyond the Infinity Cache.  Every output is requested; the counter advances with every launch.

Reported: ms per minibatch (median round [lowest .. highest]), the ratio sampler / yardstick, and the sampler's fetched
bytes per useful input byte, counting the distinct 128-byte lines under the five segments a sample gathers (state(e, t),
state(e, t + 1), g', achieved_goal(e, t + 1), action(e, t)), from the indices the device wrote.
`bench_her.py [--out profiles/her_sample.txt] [--rounds 5] [--reps 20]`"""
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
from pybullet_multigoal_gym_amd._lib import PMG_NORM_GOAL, PMG_NORM_OBSERVATION, PMG_NORM_POLICY_STATE

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'her_sample.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batch', type=int, default=1 << 20)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--small-bytes', type=int, default=2 << 20)
ap.add_argument('--large-bytes', type=int, default=512 << 20)
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'


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
    return {'ms_median': float(np.median(ms)), 'ms_min': float(min(ms)), 'ms_max': float(max(ms)), 'ms_rounds': [float(m) for m in ms]}


def fill(h, d_ptr, floats, rs, chunk=1 << 22):
    """random float32 values on the device, one host chunk uploaded over and over (the values do not matter to the time)"""
    a = rs.uniform(-3, 3, min(chunk, floats)).astype(np.float32)
    for o in range(0, floats, chunk):
        h.upload(d_ptr + 4 * o, a[:min(chunk, floats - o)])


def lines_per_sample(index, d, kind, E, T):
    """distinct 128-byte lines under the segments one sample gathers, and their useful bytes -> (mean lines, useful bytes)"""
    P, A, G = d.packed_dim, d.action_dim, d.goal_dim
    so, Ds = (0, d.observation_dim) if kind == PMG_NORM_OBSERVATION else (d.observation_dim, d.policy_state_dim)
    ago = d.observation_dim + d.policy_state_dim
    e, t, f = (index[:, k].astype(np.int64) for k in range(3))
    row = lambda tt: 4 * ((tt * E + e) * P)                  # byte offset of row (e, tt), time-major
    goal = np.where(f >= 0, row(np.maximum(f, 0)) + 4 * ago, row(t) + 4 * (ago + G))
    act_base = 1 << 50                                        # another allocation: its lines never coincide with the rows'
    segs = [(row(t) + 4 * so, 4 * Ds), (row(t + 1) + 4 * so, 4 * Ds), (goal, 4 * G), (row(t + 1) + 4 * ago, 4 * G),
            (act_base + 4 * ((t * E + e) * A), 4 * A)]
    ids = []
    for start, nbytes in segs:
        first, last = start // 128, (start + nbytes - 1) // 128
        for k in range((nbytes + 126) // 128 + 1):
            ids.append(np.where(first + k <= last, first + k, -1))
    ids = np.sort(np.stack(ids, 1), 1)
    distinct = ((ids[:, 1:] != ids[:, :-1]) & (ids[:, 1:] >= 0)).sum(1) + (ids[:, 0] >= 0)
    return float(distinct.mean()), sum(n for _, n in segs)


def bench(task, kw, kind, name):
    env = pmg.make_env(task=task, num_envs=64, **kw)
    h, d, lib = env.handle, env.handle.dims, env.handle.L.lib
    B, T = args.batch, args.steps
    P, A, G, Ds = d.packed_dim, d.action_dim, d.goal_dim, h.norm_width(kind)
    W = Ds + G
    rs = np.random.RandomState(0)
    h.norm_update(kind, rs.uniform(-3, 3, (4096, Ds)).astype(np.float32))
    h.norm_update(PMG_NORM_GOAL, rs.uniform(-3, 3, (4096, G)).astype(np.float32))
    outs = [h.device_alloc(n) for n in (4 * B * W, 4 * B * W, 4 * B * A, 4 * B, B, 12 * B)]
    d_x, d_xn, d_a, d_r, d_ok, d_ix = outs
    res = {'case': name, 'task': task, 'B': B, 'T': T, 'packed_dim': P, 'state_width': Ds, 'goal_width': G, 'action_dim': A}
    # the yardstick: contiguous rows, no gather
    d_s, d_g, d_ag = h.device_alloc(4 * B * Ds), h.device_alloc(4 * B * G), h.device_alloc(4 * B * G)
    for p, n in ((d_s, B * Ds), (d_g, B * G), (d_ag, B * G)):
        fill(h, p, n, rs)
    vp, i64 = C.c_void_p, C.c_int64

    def chain():
        assert lib.pmg_policy_input_device(h.h, kind, vp(d_s), i64(Ds), vp(d_g), i64(G), i64(B), vp(d_x)) == 0
        assert lib.pmg_policy_input_device(h.h, kind, vp(d_s), i64(Ds), vp(d_g), i64(G), i64(B), vp(d_xn)) == 0
        assert lib.pmg_compute_reward_device(h.h, vp(d_ag), vp(d_g), i64(B), vp(d_r), vp(d_ok)) == 0
    yard = stats(timed(h, chain))
    yard['bytes'] = 2 * 8 * B * W + B * (8 * G + 5)
    res['yardstick'] = yard
    for p in (d_s, d_g, d_ag):
        h.device_free(p)
    res['tables'] = []
    for label, nbytes in (('fits an XCD L2 share', args.small_bytes), ('beyond the Infinity Cache', args.large_bytes)):
        per_episode = 4 * (T + 1) * P
        E = nbytes // per_episode if label.startswith('fits') else -(-nbytes // per_episode)
        d_rows, d_acts = h.device_alloc(E * per_episode), h.device_alloc(4 * T * E * A)
        fill(h, d_rows, E * (T + 1) * P, rs)
        fill(h, d_acts, E * T * A, rs)
        src, out = h.her_structs(d_rows, E, T, P, E * P, B, d_acts, A, E * A, state_kind=kind, raw=False, future_p=0.8, seed=1, counter=0,
                                 d_x=d_x, d_x_next=d_xn, d_action=d_a, d_reward=d_r, d_goal_achieved=d_ok, d_index=d_ix)

        def launch():
            out.counter += 1
            assert lib.pmg_her_sample_device(h.h, C.byref(src), C.byref(out)) == 0
        ms = stats(timed(h, launch))
        index = np.empty((min(B, 1 << 16), 3), np.int32)
        h.download(index, d_ix)
        lines, useful_in = lines_per_sample(index, d, kind, E, T)
        useful_out = 8 * W + 4 * A + 4 + 1 + 12
        ms.update(table=label, table_bytes=E * per_episode, episodes=E, lines_128B_per_sample=lines, fetched_bytes_per_sample=128 * lines,
                  useful_input_bytes_per_sample=useful_in, fetched_per_useful_input_byte=128 * lines / useful_in,
                  output_bytes_per_sample=useful_out, over_yardstick=ms['ms_median'] / yard['ms_median'],
                  TB_per_s_fetched_plus_written=B * (128 * lines + useful_out) / (ms['ms_median'] * 1e-3) / 1e12)
        res['tables'].append(ms)
        h.device_free(d_rows)
        h.device_free(d_acts)
    for p in outs:
        h.device_free(p)
    env.close()
    return res


res = [bench('push', {}, PMG_NORM_POLICY_STATE, 'push 7 | 3 (policy_state | goal)'),
       bench('block_stack', {'num_block': 4}, PMG_NORM_OBSERVATION, 'block_stack-4 72 | 12 (observation | goal)')]
lines = ['# tools/bench_her.py: one HER minibatch (pmg_her_sample_device, every output) against the unfused chain without its gather',
         '# (2 x pmg_policy_input_device on contiguous rows + pmg_compute_reward_device), same process; B = %d, T = %d' % (args.batch, args.steps),
         '# median of %d rounds x %d launches [lowest .. highest round]' % (args.rounds, args.reps)]
for r in res:
    y = r['yardstick']
    lines.append('%s: yardstick %.4f ms [%.4f .. %.4f], %.3f TB/s algorithmic' %
                 (r['case'], y['ms_median'], y['ms_min'], y['ms_max'], y['bytes'] / (y['ms_median'] * 1e-3) / 1e12))
    for t in r['tables']:
        lines.append('  table %s (%d episodes, %.1f MiB): sampler %.4f ms [%.4f .. %.4f] = %.2f x yardstick; %.2f lines of 128 B per sample = '
                     '%.2f fetched bytes per useful input byte (%d B useful in, %d B out per sample); %.3f TB/s fetched + written' %
                     (t['table'], t['episodes'], t['table_bytes'] / 2 ** 20, t['ms_median'], t['ms_min'], t['ms_max'], t['over_yardstick'],
                      t['lines_128B_per_sample'], t['fetched_per_useful_input_byte'], t['useful_input_bytes_per_sample'],
                      t['output_bytes_per_sample'], t['TB_per_s_fetched_plus_written']))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
