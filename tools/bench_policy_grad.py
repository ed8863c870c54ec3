#!/usr/bin/env python3
"""Time of the actor's half of an update in one call (pmg_policy_grad_device: pmg_k_policy_grad_rows + the weights kernel or the partials /
merge pair) next to its yardstick, existing code timed in the SAME process on the SAME rows: the three calls it replaces,
back to back -- pmg_mlp_forward_device of the actor, the input-only pmg_mlp_grad_device of the critic (constant head, d_ga), the full
pmg_mlp_grad[_chunked]_device of the actor from d_gout = d_ga.  The host fix-up that sequence would need for the L2 and clip terms is left
out, which favours the sequence.

  networks: actor Dx -> 3 x 256 -> A tanh, critic Dx + A -> 3 x 256 -> 1, for the input widths of reach (6, 3) and block_stack-4 (28, 4);
  B = 256, 4096, 65536 with chunk_rows None, 256, 1024 (DESIGN.md 3.12's recommendations) on both sides; the fused call with grads NULL
  (rows kernel alone: action, out, q, gaction) next to forward + input-only critic gradient.

Reported: ms per launch (median round [lowest .. highest]), the difference fused - sequence and the rounds' own spread (the larger of the two
highest - lowest).  The bar: the difference is not above that spread.  `bench_policy_grad.py [--out profiles/policy_grad.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'policy_grad.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096, 65536])
ap.add_argument('--chunks', type=int, nargs='+', default=[0, 256, 1024], help='chunk_rows per batch (0: one chain)')
ap.add_argument('--hidden', type=int, default=256)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'
assert len(args.chunks) == len(args.batches)
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


class Tensors:
    def __init__(self, h, widths, rs):
        self.h, self.d_w, self.d_b = h, [], []
        for l in range(len(widths) - 1):
            w = (rs.uniform(-1, 1, (widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32)
            b = rs.uniform(-0.1, 0.1, widths[l + 1]).astype(np.float32)
            for a, out in ((w, self.d_w), (b, self.d_b)):
                p = h.device_alloc(a.nbytes)
                h.upload(p, a)
                out.append(p)
        self.struct = h.params_struct(self.d_w, self.d_b)

    def free(self):
        for p in self.d_w + self.d_b:
            self.h.device_free(p)


def bench(h, name, Dx, A, B, R):
    rs = np.random.RandomState(0)
    aw, cw = [Dx] + [args.hidden] * 3 + [A], [Dx + A] + [args.hidden] * 3 + [1]
    actor, critic, grads = Tensors(h, aw, rs), Tensors(h, cw, rs), Tensors(h, aw, rs)
    pa, pc = h.mlp_struct(aw, actor.d_w, actor.d_b, 1), h.mlp_struct(cw, critic.d_w, critic.d_b, 0)
    bufs = {'x': (B, Dx), 'pi': (B, A), 'ga': (B, A), 'q': (B,)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    h.upload(d['x'], rs.uniform(-1, 1, bufs['x']).astype(np.float32))
    work = max(h.policy_grad_work_floats(pa, pc, B, R), h.mlp_grad_work_floats(pc, B))
    d['work'] = h.device_alloc(4 * work)
    g_critic = h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, d_a=d['pi'], a_stride=A, a_dim=A, gscale=-1.0 / B, d_ga=d['ga'], ga_stride=A)
    g_actor = h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, d_gout=d['ga'], gout_stride=A, grads=grads.struct)
    fused = h.policy_grad_struct(B, d['x'], Dx, d['work'], work, -1.0 / B, 2.0 / (B * A), grads=grads.struct)
    rows = h.policy_grad_struct(B, d['x'], Dx, d['work'], work, -1.0 / B, 2.0 / (B * A), d_action=d['pi'], action_stride=A, d_q=d['q'], d_gaction=d['ga'], gaction_stride=A)

    def two():
        h.mlp_forward_device(pa, d['x'], Dx, B, d['pi'], A)
        h.mlp_grad_device(pc, g_critic)

    def three():
        two()
        if R:
            h.mlp_grad_chunked_device(pa, g_actor, R)
        else:
            h.mlp_grad_device(pa, g_actor)
    res = {'shape': name, 'B': B, 'chunk_rows': R or None, 'actor': aw, 'critic': cw, 'work_MB': 4 * work / 1e6}
    res['sequence'] = stats(timed(h, three))
    res['fused'] = stats(timed(h, lambda: h.policy_grad_device(pa, pc, fused, R)))
    res['sequence_rows'] = stats(timed(h, two))
    res['fused_rows'] = stats(timed(h, lambda: h.policy_grad_device(pa, pc, rows, 0)))
    for k, a, b in (('full', 'fused', 'sequence'), ('rows', 'fused_rows', 'sequence_rows')):
        res[k + '_difference_ms'] = res[a]['ms_median'] - res[b]['ms_median']
        res[k + '_spread_ms'] = max(res[a]['ms_max'] - res[a]['ms_min'], res[b]['ms_max'] - res[b]['ms_min'])
    for t in (actor, critic, grads):
        t.free()
    for p in d.values():
        h.device_free(p)
    return res


from pybullet_multigoal_gym_amd._lib import PmgLibrary
env = pmg.make_env(task='reach', num_envs=64, **({'_library': PmgLibrary(args.library)} if args.library else {}))
h = env.handle
fmt = lambda s: '%.4f ms [%.4f .. %.4f]' % (s['ms_median'], s['ms_min'], s['ms_max'])
res = [bench(h, name, Dx, A, B, R) for name, Dx, A in SHAPES for B, R in zip(args.batches, args.chunks)]
env.close()
lines = ['# tools/bench_policy_grad.py: pmg_policy_grad_device (actor Dx -> 3 x %d -> A tanh through the critic Dx + A -> 3 x %d -> 1, grads given) next to the' % (args.hidden, args.hidden),
         '# three calls it replaces, back to back in the same process: pmg_mlp_forward_device + input-only pmg_mlp_grad_device of the critic + full',
         '# pmg_mlp_grad[_chunked]_device of the actor; "rows": the fused call with grads NULL next to the first two of those calls',
         '# median of %d rounds x %d launches [lowest .. highest round]; bar: fused - sequence <= the rounds\' own spread (the larger highest - lowest)' % (args.rounds, args.reps)]
for r in res:
    for k, a, b in (('full', 'fused', 'sequence'), ('rows', 'fused_rows', 'sequence_rows')):
        diff, spread = r[k + '_difference_ms'], r[k + '_spread_ms']
        lines.append('%s B = %d chunk_rows %s %s: fused %s; sequence %s; fused / sequence = %.2f; difference %+.4f ms, spread %.4f ms: %s' %
                     (r['shape'], r['B'], r['chunk_rows'] if k == 'full' else None, k, fmt(r[a]), fmt(r[b]), r[a]['ms_median'] / r[b]['ms_median'], diff, spread,
                      'within the bar' if diff <= spread else '**BAR MISSED**'))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
