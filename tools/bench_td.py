#!/usr/bin/env python3
"""Time of the fused TD target (pmg_td_target_device: pmg_k_td_target) next to its yardstick, existing code timed in the
SAME process: pmg_mlp_forward_device of the target actor on [B, Dx] plus pmg_mlp_forward_device of the target critic on a pre-built
[B, Dx + A] table.  The concatenation and the elementwise pass a caller of the two-call path needs as well are left out of the
yardstick, which favours it.  pmg_q_device on the two tables is timed beside the critic forward on the pre-built table.

  networks: actor Dx -> 3 x 256 -> A (tanh), critic Dx + A -> 3 x 256 -> 1, for the input widths of reach (6, 3) and block_stack-4
  (28, 4); B = 256, 4096, 65536; gamma 0.98, clips [-50, 0], d_terminal, d_q_next and d_next_action given.

Reported: ms per launch (median round [lowest .. highest]) and the FLOP rate of the fused call (2 x weights of both networks per row)
against the 157.3 TF f32 matrix peak.  `bench_td.py [--out profiles/td_target.txt] [--rounds 5] [--reps 20]`"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pybullet_multigoal_gym_amd as pmg

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'td_target.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096, 65536])
ap.add_argument('--hidden', type=int, default=256)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'
PEAK_TF = 157.3
SHAPES = (('reach', 6, 3), ('block_stack-4', 28, 4))


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


def upload_net(h, widths, rs, out_act):
    d_w, d_b = [], []
    for l in range(len(widths) - 1):
        w = (rs.uniform(-1, 1, (widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32)
        b = rs.uniform(-0.1, 0.1, widths[l + 1]).astype(np.float32)
        for a, out in ((w, d_w), (b, d_b)):
            p = h.device_alloc(a.nbytes)
            h.upload(p, a)
            out.append(p)
    return h.mlp_struct(widths, d_w, d_b, out_act), d_w + d_b


def flops(widths):
    return 2 * sum(widths[l] * widths[l + 1] for l in range(len(widths) - 1))


def bench(h, name, Dx, A, B):
    rs = np.random.RandomState(0)
    aw, cw = [Dx] + [args.hidden] * 3 + [A], [Dx + A] + [args.hidden] * 3 + [1]
    actor, pa = upload_net(h, aw, rs, 1)
    critic, pc = upload_net(h, cw, rs, 0)
    bufs = {'x': (B, Dx), 'xa': (B, Dx + A), 'a': (B, A), 'r': (B,), 'y': (B,), 'q': (B,), 'na': (B, A), 'qf': (B,)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    d['t'] = h.device_alloc(B)
    for k in ('x', 'xa', 'a'):
        h.upload(d[k], rs.uniform(-1, 1, bufs[k]).astype(np.float32))
    h.upload(d['r'], -rs.randint(0, 2, B).astype(np.float32))
    h.upload(d['t'], (rs.uniform(0, 1, B) < 0.1).astype(np.uint8))
    td = h.td_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, d['t'], d['q'], d['na'])
    res = {'shape': name, 'B': B, 'actor': aw, 'critic': cw, 'flop_per_row': flops(aw) + flops(cw)}
    res['fused'] = stats(timed(h, lambda: h.td_target_device(actor, critic, td)))
    res['actor_forward'] = stats(timed(h, lambda: h.mlp_forward_device(actor, d['x'], Dx, B, d['na'], A)))
    res['critic_forward'] = stats(timed(h, lambda: h.mlp_forward_device(critic, d['xa'], Dx + A, B, d['qf'], 1)))

    def two_calls():
        h.mlp_forward_device(actor, d['x'], Dx, B, d['na'], A)
        h.mlp_forward_device(critic, d['xa'], Dx + A, B, d['qf'], 1)
    res['two_calls'] = stats(timed(h, two_calls))
    res['q'] = stats(timed(h, lambda: h.q_device(critic, d['x'], Dx, Dx, d['a'], A, A, B, d['qf'], 1)))
    res['fused']['TF'] = B * res['flop_per_row'] / (res['fused']['ms_median'] * 1e-3) / 1e12
    for p in pa + pc + list(d.values()):
        h.device_free(p)
    return res


from pybullet_multigoal_gym_amd._lib import PmgLibrary
env = pmg.make_env(task='reach', num_envs=64, **({'_library': PmgLibrary(args.library)} if args.library else {}))
h = env.handle
fmt = lambda s: '%.4f ms [%.4f .. %.4f]' % (s['ms_median'], s['ms_min'], s['ms_max'])
res = [bench(h, name, Dx, A, B) for name, Dx, A in SHAPES for B in args.batches]
env.close()
lines = ['# tools/bench_td.py: pmg_td_target_device (actor Dx -> 3 x %d -> A tanh, critic Dx + A -> 3 x %d -> 1; gamma 0.98, clips [-50, 0], every output) next to' % (args.hidden, args.hidden),
         '# pmg_mlp_forward_device of the actor on [B, Dx] + pmg_mlp_forward_device of the critic on a pre-built [B, Dx + A] table (two calls back to back), same process',
         '# median of %d rounds x %d launches [lowest .. highest round]; TF of the fused call against the %.1f TF f32 matrix peak' % (args.rounds, args.reps, PEAK_TF)]
for r in res:
    two, fused = r['two_calls'], r['fused']
    lines.append('%s (Dx %d, A %d) B = %d, %d FLOP per row: fused %s = %.2f TF (%.1f %% of peak); two calls %s (actor alone %s, critic alone %s); fused - two calls = %+.4f ms (%+.1f %%); q_device %s' %
                 (r['shape'], r['actor'][0], r['actor'][-1], r['B'], r['flop_per_row'], fmt(fused), fused['TF'], 100 * fused['TF'] / PEAK_TF, fmt(two), fmt(r['actor_forward']),
                  fmt(r['critic_forward']), fused['ms_median'] - two['ms_median'], 100 * (fused['ms_median'] / two['ms_median'] - 1), fmt(r['q'])))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
