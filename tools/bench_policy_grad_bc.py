#!/usr/bin/env python3
"""Time of the actor's half of an update with the behaviour-cloning term in one call (pmg_policy_grad_bc_device: pmg_k_policy_grad_bc_rows +
the weights kernel or the partials / merge pair) next to two yardsticks of existing code, timed in the SAME process on the
SAME rows, alternating round by round:

  (a) the sequence it replaces, back to back: pmg_mlp_forward_device of the actor, pmg_q_device on x | clip(o) and on the demonstration rows
      x | ad, the input-only pmg_mlp_grad_device of the critic (constant head, d_ga), the full pmg_mlp_grad[_chunked]_device of the actor from
      d_gout.  The host fix-up that sequence needs for the filter and the head (a sync, a download and an upload) is left out, which favours
      the sequence;
  (b) pmg_policy_grad_device itself, next to the new call with demo_begin = B (no demonstration row: the extra pass never runs).

  networks: actor Dx -> 3 x 256 -> A tanh, critic Dx + A -> 3 x 256 -> 1, for the input widths of reach (6, 3) and block_stack-4 (28, 4);
  B = 1024 with the last 128 rows demonstrations (baselines' split) and B = 4096 with 512, chunk_rows None and 256.

Reported: ms per launch (median round [lowest .. highest]), the difference new - yardstick and the rounds' own spread (the larger of the two
highest - lowest).  The bar, both times: the difference is not above that spread.
`bench_policy_grad_bc.py [--out profiles/policy_grad_bc.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'policy_grad_bc.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batches', type=int, nargs='+', default=[1024, 4096])
ap.add_argument('--demos', type=int, nargs='+', default=[128, 512], help='demonstration rows per batch, the last ones')
ap.add_argument('--chunks', type=int, nargs='+', default=[0, 256], help='chunk_rows, every batch with each (0: one chain)')
ap.add_argument('--hidden', type=int, default=256)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'
assert len(args.demos) == len(args.batches)
SHAPES = (('reach', 6, 3), ('block_stack-4', 28, 4))


def timed_alternating(h, launches):
    """-> per launch function, ms per launch of every round; the functions take turns within a round"""
    for f in launches:
        for _ in range(args.warmup):
            f()
    h.sync()
    out = [[] for _ in launches]
    for _ in range(args.rounds):
        for f, ms in zip(launches, out):
            h.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                f()
            h.sync()
            ms.append((time.perf_counter() - t0) / args.reps * 1e3)
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


def bench(h, name, Dx, A, B, demos, R):
    rs = np.random.RandomState(0)
    aw, cw = [Dx] + [args.hidden] * 3 + [A], [Dx + A] + [args.hidden] * 3 + [1]
    actor, critic, grads = Tensors(h, aw, rs), Tensors(h, cw, rs), Tensors(h, aw, rs)
    pa, pc = h.mlp_struct(aw, actor.d_w, actor.d_b, 1), h.mlp_struct(cw, critic.d_w, critic.d_b, 0)
    b0 = B - demos
    bufs = {'x': (B, Dx), 'ad': (B, A), 'pi': (B, A), 'ga': (B, A), 'q': (B,), 'qd': (B,)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    d['f'] = h.device_alloc(B)
    h.upload(d['x'], rs.uniform(-1, 1, bufs['x']).astype(np.float32))
    h.upload(d['ad'], rs.uniform(-1, 1, bufs['ad']).astype(np.float32))
    work = max(h.policy_grad_work_floats(pa, pc, B, R), h.mlp_grad_work_floats(pc, B))
    d['work'] = h.device_alloc(4 * work)
    g_critic = h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, d_a=d['pi'], a_stride=A, a_dim=A, gscale=-1.0 / B, d_ga=d['ga'], ga_stride=A)
    g_actor = h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, d_gout=d['ga'], gout_stride=A, grads=grads.struct)
    fused = h.policy_grad_struct(B, d['x'], Dx, d['work'], work, -1.0 / B, 2.0 / (B * A), grads=grads.struct, d_q=d['q'])
    with_demos = h.policy_bc_struct(b0, d['ad'], A, 2 * 0.0078, 1, d['qd'], d['f'])
    without = h.policy_bc_struct(B, None, 0, 2 * 0.0078, 1, None, None)

    def sequence():
        h.mlp_forward_device(pa, d['x'], Dx, B, d['pi'], A)
        h.q_device(pc, d['x'], Dx, Dx, d['pi'], A, A, B, d['q'], 1)
        h.q_device(pc, d['x'] + 4 * b0 * Dx, Dx, Dx, d['ad'] + 4 * b0 * A, A, A, demos, d['qd'] + 4 * b0, 1)
        h.mlp_grad_device(pc, g_critic)
        if R:
            h.mlp_grad_chunked_device(pa, g_actor, R)
        else:
            h.mlp_grad_device(pa, g_actor)
    res = {'shape': name, 'B': B, 'demos': demos, 'chunk_rows': R or None, 'actor': aw, 'critic': cw}
    ms = timed_alternating(h, [sequence, lambda: h.policy_grad_bc_device(pa, pc, fused, with_demos, R),
                               lambda: h.policy_grad_device(pa, pc, fused, R), lambda: h.policy_grad_bc_device(pa, pc, fused, without, R)])
    for k, v in zip(('sequence', 'fused', 'plain', 'fused_no_demos'), ms):
        res[k] = stats(v)
    for k, a, b in (('a', 'fused', 'sequence'), ('b', 'fused_no_demos', 'plain')):
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
res = [bench(h, name, Dx, A, B, demos, R) for name, Dx, A in SHAPES for B, demos in zip(args.batches, args.demos) for R in args.chunks]
env.close()
lines = ['# tools/bench_policy_grad_bc.py: pmg_policy_grad_bc_device (actor Dx -> 3 x %d -> A tanh through the critic Dx + A -> 3 x %d -> 1, grads and d_q given,' % (args.hidden, args.hidden),
         '# the last `demos` rows demonstrations, q_filter 1, d_q_demo and d_filter given) next to (a) the sequence it replaces, back to back in the same',
         '# process: pmg_mlp_forward_device + pmg_q_device on x | a + pmg_q_device on the demonstration rows + input-only pmg_mlp_grad_device of the critic',
         '# + full pmg_mlp_grad[_chunked]_device of the actor, without the host fix-up; (b) pmg_policy_grad_device next to the new call with demo_begin = B',
         '# median of %d rounds x %d launches [lowest .. highest round], the four taking turns within a round; bar: new - yardstick <= the rounds\' own' % (args.rounds, args.reps),
         '# spread (the larger highest - lowest)']
for r in res:
    for k, a, b, what in (('a', 'fused', 'sequence', 'sequence'), ('b', 'fused_no_demos', 'plain', 'pmg_policy_grad_device')):
        diff, spread = r[k + '_difference_ms'], r[k + '_spread_ms']
        lines.append('%s B = %d demos %d chunk_rows %s (%s): fused %s; %s %s; ratio %.2f; difference %+.4f ms, spread %.4f ms: %s' %
                     (r['shape'], r['B'], r['demos'] if k == 'a' else 0, r['chunk_rows'], k, fmt(r[a]), what, fmt(r[b]), r[a]['ms_median'] / r[b]['ms_median'], diff,
                      spread, 'within the bar' if diff <= spread else '**BAR MISSED**'))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
