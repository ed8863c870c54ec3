#!/usr/bin/env python3
"""Time of SAC's actor half in one call (pmg_sac_policy_grad_device: pmg_k_sac_policy_grad_rows + the weights kernel or the partials / merge
pair) next to its yardstick, existing code timed in the SAME process on the SAME rows: the six calls it replaces, back to back --
pmg_sac_sample_device (a, logp, n, z), pmg_q_device of either critic, the input-only pmg_mlp_grad_device of either critic (constant head, d_ga),
the full pmg_mlp_grad[_chunked]_device of the actor from a d_gout.  The download, the numpy fix-up, the upload and the sync that sequence needs
in the middle are left out, which favours the sequence.  The temperature step (pmg_sac_alpha_device) is timed alone at the same batches.

  networks: actor Dx -> 3 x 256 -> 2 A, critics Dx + A -> 3 x 256 -> 1, for the input widths of reach (6, 3) and block_stack-4 (28, 4);
  B = 256, 4096, 65536 with chunk_rows None, 256, 1024 (DESIGN.md 3.12's recommendations) on both sides.

Reported: ms per launch (median round [lowest .. highest]), the rounds of the two variants taking turns, the difference fused - sequence and
the rounds' own spread (the larger of the two highest - lowest).  The bar: the difference is not above that spread.
`bench_sac_policy_grad.py [--out profiles/sac_policy_grad.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sac_policy_grad.txt'))
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


def timed_in_turns(h, launches):
    """-> ms per launch of every round, per variant; the variants take turns round by round"""
    for launch in launches:
        for _ in range(args.warmup):
            launch()
    h.sync()
    out = [[] for _ in launches]
    for _ in range(args.rounds):
        for k, launch in enumerate(launches):
            h.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                launch()
            h.sync()
            out[k].append((time.perf_counter() - t0) / args.reps * 1e3)
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
    aw, cw = [Dx] + [args.hidden] * 3 + [2 * A], [Dx + A] + [args.hidden] * 3 + [1]
    actor, c1, c2, grads = Tensors(h, aw, rs), Tensors(h, cw, rs), Tensors(h, cw, rs), Tensors(h, aw, rs)
    pa, p1, p2 = h.mlp_struct(aw, actor.d_w, actor.d_b, 0), h.mlp_struct(cw, c1.d_w, c1.d_b, 0), h.mlp_struct(cw, c2.d_w, c2.d_b, 0)
    bufs = {'x': (B, Dx), 'a': (B, A), 'n': (B, A), 'z': (B, 2 * A), 'logp': (B,), 'q1': (B,), 'q2': (B,), 'ga1': (B, A), 'ga2': (B, A), 'gout': (B, 2 * A), 'state': (4,)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    h.upload(d['x'], rs.uniform(-1, 1, bufs['x']).astype(np.float32))
    h.upload(d['gout'], (rs.uniform(-1, 1, bufs['gout']) / B).astype(np.float32))
    h.upload(d['state'], np.array([np.log(0.2), 0, 0, 0.2], np.float32))
    work = max(h.sac_policy_grad_work_floats(pa, 1, 1, B, R), h.mlp_grad_work_floats(p1, B), h.mlp_grad_chunked_work_floats(pa, B, R) if R else h.mlp_grad_work_floats(pa, B))
    d['work'] = h.device_alloc(4 * work)
    smp = h.sac_sample_struct(B, d['x'], Dx, d['a'], A, d['logp'], d['n'], A, d['z'], 2 * A, seed=1, counter=2)
    g_c = [h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, d_a=d['a'], a_stride=A, a_dim=A, gscale=-1.0 / B, d_ga=d[k], ga_stride=A) for k in ('ga1', 'ga2')]
    g_actor = h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, d_gout=d['gout'], gout_stride=2 * A, grads=grads.struct)
    fused = h.sac_policy_grad_struct(B, d['x'], Dx, d['work'], work, -1.0 / B, 1.0 / B, 0.2, seed=1, counter=2, grads=grads.struct, d_action=d['a'], action_stride=A,
                                     d_logp=d['logp'])
    alpha = h.sac_alpha_struct(B, d['logp'], d['state'], -float(A), 3e-4, 1)

    def sequence():
        h.sac_sample_device(pa, smp)
        h.q_device(p1, d['x'], Dx, Dx, d['a'], A, A, B, d['q1'])
        h.q_device(p2, d['x'], Dx, Dx, d['a'], A, A, B, d['q2'])
        h.mlp_grad_device(p1, g_c[0])
        h.mlp_grad_device(p2, g_c[1])
        if R:
            h.mlp_grad_chunked_device(pa, g_actor, R)
        else:
            h.mlp_grad_device(pa, g_actor)
    res = {'shape': name, 'B': B, 'chunk_rows': R or None, 'actor': aw, 'critic': cw, 'work_MB': 4 * work / 1e6}
    t_fused, t_seq = timed_in_turns(h, (lambda: h.sac_policy_grad_device(pa, p1, p2, fused, R), sequence))
    res['fused'], res['sequence'] = stats(t_fused), stats(t_seq)
    res['alpha'] = stats(timed_in_turns(h, (lambda: h.sac_alpha_device(alpha),))[0])
    res['difference_ms'] = res['fused']['ms_median'] - res['sequence']['ms_median']
    res['spread_ms'] = max(res['fused']['ms_max'] - res['fused']['ms_min'], res['sequence']['ms_max'] - res['sequence']['ms_min'])
    for t in (actor, c1, c2, grads):
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
lines = ['# tools/bench_sac_policy_grad.py: pmg_sac_policy_grad_device (actor Dx -> 3 x %d -> 2 A through two critics Dx + A -> 3 x %d -> 1, grads given) next to the' % (args.hidden, args.hidden),
         '# six calls it replaces, back to back in the same process: pmg_sac_sample_device + 2 x pmg_q_device + 2 x input-only pmg_mlp_grad_device of a critic +',
         '# full pmg_mlp_grad[_chunked]_device of the actor (the host fix-up, its two transfers and its sync are NOT in the sequence\'s time)',
         '# calls: fused 1, sequence 6; launches: fused 2 (chunked: 3), sequence 7 (chunked: 8); forwards: fused 1 actor + 2 critic, sequence 2 actor + 4 critic',
         '# median of %d rounds x %d launches [lowest .. highest round], the variants taking turns; bar: fused - sequence <= the rounds\' own spread' % (args.rounds, args.reps)]
for r in res:
    lines.append('%s B = %d chunk_rows %s: fused %s; sequence %s; fused / sequence = %.2f; difference %+.4f ms, spread %.4f ms: %s; alpha step %s' %
                 (r['shape'], r['B'], r['chunk_rows'], fmt(r['fused']), fmt(r['sequence']), r['fused']['ms_median'] / r['sequence']['ms_median'], r['difference_ms'],
                  r['spread_ms'], 'within the bar' if r['difference_ms'] <= r['spread_ms'] else '**BAR MISSED**', fmt(r['alpha'])))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
