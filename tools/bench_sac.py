#!/usr/bin/env python3
"""Time of SAC's fused soft target (pmg_sac_target_device: pmg_k_sac_target) and of the Gaussian head (pmg_sac_sample_device:
pmg_k_sac) next to their yardsticks, existing code timed in the SAME process on the same rows:

  target:  pmg_td3_target_device with two critics and sigma 0.2 on the A-wide tanh actor -- the same three networks' worth of matrix work
           bar the actor's last layer (2 A units here against A there), one tile rebuild per 32 rows fewer and no log pi;
  sample:  pmg_mlp_forward_device of the same Gaussian network (its 2 A outputs stored), i.e. the head's arithmetic and outputs are the extra.

  networks: actor Dx -> 3 x 256 -> 2 A (SAC) / A tanh (TD3), two critics Dx + A -> 3 x 256 -> 1, for the input widths of reach (6, 3) and
  block_stack-4 (28, 4); B = 256, 4096, 65536; gamma 0.98, clips [-50, 0], alpha 0.2, d_terminal, every output given.

Variants, timed in turn within every round so that drift of the machine meets all of them alike:
  td3      pmg_td3_target_device, two critics, sigma 0.2, noise_clip 0.5         (the target's yardstick)
  sac      pmg_sac_target_device, two critics, sampling, d_next_action and d_logp given
  sac_ws   the same with d_next_action NULL: a' kept in the workspace
  sac_mode the same as sac without sampling (what the draws cost: sac - sac_mode)
  fwd      pmg_mlp_forward_device of the Gaussian actor                           (the sample call's yardstick)
  sample   pmg_sac_sample_device, a, log pi and n given
  sample_a pmg_sac_sample_device, the action alone (a rollout's call)

Reported: ms per launch (median round [lowest .. highest]), and for each comparison the difference of the medians next to the spread of the
rounds (highest - lowest, the larger of the two variants').  No bar is fixed: the figures and an account of the differences go to DESIGN.md 3.15.
`bench_sac.py [--out profiles/sac_target.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sac_target.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096, 65536])
ap.add_argument('--hidden', type=int, default=256)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'
SHAPES = (('reach', 6, 3), ('block_stack-4', 28, 4))
ORDER = ('td3', 'sac', 'sac_ws', 'sac_mode', 'fwd', 'sample', 'sample_a')


def timed(h, launches):
    """{name: launch} -> {name: ms per launch of every round}; the variants take turns within a round"""
    for launch in launches.values():
        for _ in range(args.warmup):
            launch()
    h.sync()
    out = {k: [] for k in launches}
    for _ in range(args.rounds):
        for k, launch in launches.items():
            h.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                launch()
            h.sync()
            out[k].append((time.perf_counter() - t0) / args.reps * 1e3)
    return out


def stats(ms):
    return {'ms_median': float(np.median(ms)), 'ms_min': float(min(ms)), 'ms_max': float(max(ms))}


def upload_net(h, widths, rs, out_act, last_scale=1.0):
    d_w, d_b = [], []
    for l in range(len(widths) - 1):
        w = (rs.uniform(-1, 1, (widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32)
        b = rs.uniform(-0.1, 0.1, widths[l + 1]).astype(np.float32)
        if l == len(widths) - 2:
            w, b = (w * last_scale).astype(np.float32), (b * last_scale).astype(np.float32)
        for a, out in ((w, d_w), (b, d_b)):
            p = h.device_alloc(a.nbytes)
            h.upload(p, a)
            out.append(p)
    return h.mlp_struct(widths, d_w, d_b, out_act), d_w + d_b


def flops(widths):
    return 2 * sum(widths[l] * widths[l + 1] for l in range(len(widths) - 1))


def bench(h, name, Dx, A, B):
    rs = np.random.RandomState(0)
    gw, aw, cw = [Dx] + [args.hidden] * 3 + [2 * A], [Dx] + [args.hidden] * 3 + [A], [Dx + A] + [args.hidden] * 3 + [1]
    gauss, pg = upload_net(h, gw, rs, 0)
    actor, pa = upload_net(h, aw, rs, 1)
    c1, p1 = upload_net(h, cw, rs, 0)
    c2, p2 = upload_net(h, cw, rs, 0)
    bufs = {'x': (B, Dx), 'r': (B,), 'y': (B,), 'qmin': (B,), 'q1': (B,), 'q2': (B,), 'na': (B, A), 'work': (B, A), 'lp': (B,), 'n': (B, A), 'z': (B, 2 * A)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    d['t'] = h.device_alloc(B)
    h.upload(d['x'], rs.uniform(-1, 1, bufs['x']).astype(np.float32))
    h.upload(d['r'], -rs.randint(0, 2, B).astype(np.float32))
    h.upload(d['t'], (rs.uniform(0, 1, B) < 0.1).astype(np.uint8))
    kw = dict(d_terminal=d['t'], d_q_min=d['qmin'], d_q1=d['q1'], d_q2=d['q2'])
    td3 = h.td3_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.2, 0.5, 1, 2, 0, d_next_action=d['na'], **kw)
    sac = h.sac_target_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.2, -20.0, 2.0, 1, 1, 2, 0, d_next_action=d['na'], d_logp=d['lp'], **kw)
    sac_ws = h.sac_target_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.2, -20.0, 2.0, 1, 1, 2, 0, d_logp=d['lp'], d_work=d['work'], work_floats=B * A, **kw)
    sac_mode = h.sac_target_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.2, -20.0, 2.0, 0, 1, 2, 0, d_next_action=d['na'], d_logp=d['lp'], **kw)
    smp = h.sac_sample_struct(B, d['x'], Dx, d['na'], A, d['lp'], d['n'], A, None, 0, -20.0, 2.0, 1, 1, 2, 0)
    smp_a = h.sac_sample_struct(B, d['x'], Dx, d['na'], A, None, None, 0, None, 0, -20.0, 2.0, 1, 1, 2, 0)
    ms = timed(h, {'td3': lambda: h.td3_target_device(actor, c1, c2, td3), 'sac': lambda: h.sac_target_device(gauss, c1, c2, sac),
                   'sac_ws': lambda: h.sac_target_device(gauss, c1, c2, sac_ws), 'sac_mode': lambda: h.sac_target_device(gauss, c1, c2, sac_mode),
                   'fwd': lambda: h.mlp_forward_device(gauss, d['x'], Dx, B, d['z'], 2 * A), 'sample': lambda: h.sac_sample_device(gauss, smp),
                   'sample_a': lambda: h.sac_sample_device(gauss, smp_a)})
    res = {'shape': name, 'B': B, 'gaussian_actor': gw, 'td3_actor': aw, 'critic': cw, 'flop_per_row_sac': flops(gw) + 2 * flops(cw), 'flop_per_row_td3': flops(aw) + 2 * flops(cw)}
    res.update({k: stats(v) for k, v in ms.items()})
    for p in pg + pa + p1 + p2 + list(d.values()):
        h.device_free(p)
    return res


def versus(r, new, old):
    a, b = r[new], r[old]
    spread = max(a['ms_max'] - a['ms_min'], b['ms_max'] - b['ms_min'])
    diff = a['ms_median'] - b['ms_median']
    return '%s - %s = %+.4f ms (%+.1f %%), spread of the rounds %.4f ms: %s' % (new, old, diff, 100 * diff / b['ms_median'], spread,
                                                                               'within' if abs(diff) <= spread else ('slower' if diff > 0 else 'faster'))


from pybullet_multigoal_gym_amd._lib import PmgLibrary
env = pmg.make_env(task='reach', num_envs=64, **({'_library': PmgLibrary(args.library)} if args.library else {}))
h = env.handle
fmt = lambda s: '%.4f ms [%.4f .. %.4f]' % (s['ms_median'], s['ms_min'], s['ms_max'])
res = [bench(h, name, Dx, A, B) for name, Dx, A in SHAPES for B in args.batches]
env.close()
lines = ['# tools/bench_sac.py: pmg_sac_target_device and pmg_sac_sample_device (Gaussian actor Dx -> 3 x %d -> 2 A, critics Dx + A -> 3 x %d -> 1; gamma 0.98, clips [-50, 0], alpha 0.2, d_terminal, every output)' % (args.hidden, args.hidden),
         '# td3 = pmg_td3_target_device, two critics, sigma 0.2, on the A-wide tanh actor: the target\'s yardstick; fwd = pmg_mlp_forward_device of the Gaussian actor: the sample call\'s; same process, same rows',
         '# sac = two critics, sampling, d_next_action; sac_ws = a\' kept in the workspace; sac_mode = no sampling; sample = a, log pi, n; sample_a = the action alone',
         '# median of %d rounds x %d launches [lowest .. highest round], the variants taking turns within a round' % (args.rounds, args.reps)]
for r in res:
    lines.append('%s (Dx %d, A %d) B = %d: ' % (r['shape'], r['td3_actor'][0], r['td3_actor'][-1], r['B']) + '; '.join('%s %s' % (k, fmt(r[k])) for k in ORDER))
    lines.append('    ' + '; '.join((versus(r, 'sac', 'td3'), versus(r, 'sac_ws', 'sac'), versus(r, 'sac', 'sac_mode'), versus(r, 'sample', 'fwd'), versus(r, 'sample_a', 'fwd'))))
    lines.append('    sac: %.2f TF of f32 matrix work (%d FLOP per row; td3: %d)' % (r['B'] * r['flop_per_row_sac'] / (r['sac']['ms_median'] * 1e-3) / 1e12, r['flop_per_row_sac'],
                                                                                     r['flop_per_row_td3']))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
