#!/usr/bin/env python3
"""Time of PPO's actor update in one call (pmg_ppo_policy_grad_device: pmg_k_ppo_policy_grad_rows + the weights kernel or the partials / merge
pair) next to its yardstick, existing code timed in the SAME process on the SAME rows: pmg_mlp_forward_device +
pmg_mlp_grad_chunked_device(d_gout) of the same actor -- the unfused chain WITHOUT its head (ratio, clip, head gradient), which a caller would
have had to compute on the host behind a sync.  It is a lower bound of what could be done before, as DESIGN.md 3.8 used one.  Beside it:
pmg_gae_device at T = 50, N = 4096 and 131072 (time-major tables), and pmg_adv_stats_device + pmg_adv_apply_device at M = 204800, each alone.

  actor Dx = 13 -> 3 x 256 -> 2 A, A = 4; B = 4096, 32768, 204800 with chunk_rows 256, 1024, 1024 on both sides.

Reported: ms per launch (median round [lowest .. highest]), the rounds of the variants taking turns, and the rounds' own spread.  No pass bar.
`bench_ppo.py [--out profiles/ppo_policy_grad.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ppo_policy_grad.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batches', type=int, nargs='+', default=[4096, 32768, 204800])
ap.add_argument('--chunks', type=int, nargs='+', default=[256, 1024, 1024], help='chunk_rows per batch (0: one chain)')
ap.add_argument('--gae-envs', type=int, nargs='+', default=[4096, 131072])
ap.add_argument('--gae-steps', type=int, default=50)
ap.add_argument('--stats-count', type=int, default=204800)
ap.add_argument('--hidden', type=int, default=256)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
assert len(args.chunks) == len(args.batches)
DX, A = 13, 4


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


def bench_grad(h, B, R):
    rs = np.random.RandomState(0)
    aw = [DX] + [args.hidden] * 3 + [2 * A]
    actor, grads = Tensors(h, aw, rs), Tensors(h, aw, rs)
    pa = h.mlp_struct(aw, actor.d_w, actor.d_b, 0)
    bufs = {'x': (B, DX), 'zo': (B, 2 * A), 'n': (B, A), 'adv': (B,), 'rho': (B,), 'lr': (B,), 'gout': (B, 2 * A), 'z': (B, 2 * A), 'st': (4,)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    d['cl'] = h.device_alloc(B)
    x = rs.uniform(-1, 1, bufs['x']).astype(np.float32)
    h.upload(d['x'], x)
    h.upload(d['n'], rs.standard_normal(bufs['n']).astype(np.float32))
    h.upload(d['adv'], rs.standard_normal(B).astype(np.float32))
    h.upload(d['gout'], (rs.uniform(-1, 1, bufs['gout']) / B).astype(np.float32))
    work = max(h.ppo_policy_grad_work_floats(pa, B, R), h.mlp_grad_chunked_work_floats(pa, B, R) if R else h.mlp_grad_work_floats(pa, B))
    d['work'] = h.device_alloc(4 * work)
    h.mlp_forward_device(pa, d['x'], DX, B, d['zo'], 2 * A)       # the recorded policy: the same weights, so rho is near 1 and nothing is clipped away
    g_actor = h.grad_struct(B, d['x'], DX, DX, d['work'], work, d_gout=d['gout'], gout_stride=2 * A, grads=grads.struct)
    fused = h.ppo_policy_grad_struct(B, d['x'], DX, d['zo'], 2 * A, d['n'], A, d['adv'], -1.0 / B, -0.01 / B, 0.8, 1.2, grads=grads.struct, d_ratio=d['rho'],
                                     d_logratio=d['lr'], d_clipped=d['cl'], d_work=d['work'], work_floats=work)
    st = h.ppo_stats_struct(B, d['rho'], d['lr'], d['cl'], d['adv'], d['st'], 0.8, 1.2)

    def sequence():
        h.mlp_forward_device(pa, d['x'], DX, B, d['z'], 2 * A)
        if R:
            h.mlp_grad_chunked_device(pa, g_actor, R)
        else:
            h.mlp_grad_device(pa, g_actor)
    res = {'B': B, 'chunk_rows': R or None, 'actor': aw, 'work_MB': 4 * work / 1e6}
    t_fused, t_seq = timed_in_turns(h, (lambda: h.ppo_policy_grad_device(pa, fused, R), sequence))
    res['fused'], res['sequence'] = stats(t_fused), stats(t_seq)
    res['ppo_stats'] = stats(timed_in_turns(h, (lambda: h.ppo_stats_device(st),))[0])
    res['difference_ms'] = res['fused']['ms_median'] - res['sequence']['ms_median']
    res['spread_ms'] = max(res['fused']['ms_max'] - res['fused']['ms_min'], res['sequence']['ms_max'] - res['sequence']['ms_min'])
    out = np.empty(4, np.float32)
    h.sync()
    h.download(out, d['st'])
    res['stats_of_the_batch'] = [float(v) for v in out]
    for t in (actor, grads):
        t.free()
    for p in d.values():
        h.device_free(p)
    return res


def bench_gae(h, T, N):
    rs = np.random.RandomState(1)
    d = {k: h.device_alloc(4 * (T + 1) * N) for k in ('r', 'v', 'cut', 'adv', 'ret')}
    h.upload(d['r'], rs.uniform(-1, 1, T * N).astype(np.float32))
    h.upload(d['v'], rs.standard_normal((T + 1) * N).astype(np.float32))
    h.upload(d['cut'], (rs.uniform(0, 1, T * N) < 0.02).astype(np.float32))
    g = h.gae_struct(T, N, 0.98, 0.95, (d['r'], N, 1), (d['v'], N, 1), (d['v'] + 4 * N, N, 1), (d['adv'], N, 1), cut=(d['cut'], N, 1), ret=(d['ret'], N, 1))
    res = {'T': T, 'N': N, 'gae': stats(timed_in_turns(h, (lambda: h.gae_device(g),))[0]), 'bytes': 4 * 6 * T * N}
    for p in d.values():
        h.device_free(p)
    return res


def bench_norm(h, M):
    rs = np.random.RandomState(2)
    d_x, d_y, d_s = h.device_alloc(4 * M), h.device_alloc(4 * M), h.device_alloc(8)
    h.upload(d_x, rs.standard_normal(M).astype(np.float32))
    s = h.adv_stats_struct(M, d_x, d_s)
    t_s, t_a = timed_in_turns(h, (lambda: h.adv_stats_device(s), lambda: h.adv_apply_device(d_x, M, d_s, d_y)))
    for p in (d_x, d_y, d_s):
        h.device_free(p)
    return {'M': M, 'stats': stats(t_s), 'apply': stats(t_a)}


from pybullet_multigoal_gym_amd._lib import PmgLibrary
env = pmg.make_env(task='reach', num_envs=64, **({'_library': PmgLibrary(args.library)} if args.library else {}))
h = env.handle
fmt = lambda s: '%.4f ms [%.4f .. %.4f]' % (s['ms_median'], s['ms_min'], s['ms_max'])
grad = [bench_grad(h, B, R) for B, R in zip(args.batches, args.chunks)]
gae = [bench_gae(h, args.gae_steps, N) for N in args.gae_envs]
norm = bench_norm(h, args.stats_count)
env.close()
lines = ['# tools/bench_ppo.py: pmg_ppo_policy_grad_device (actor %d -> 3 x %d -> %d, grads, d_ratio, d_logratio and d_clipped given) next to' % (DX, args.hidden, 2 * A),
         '# pmg_mlp_forward_device + pmg_mlp_grad[_chunked]_device(d_gout) of the same actor in the same process: the unfused chain WITHOUT its head (a lower',
         '# bound of the old route, whose head needs a host sync); launches: fused 3 (one chain: 2), yardstick 4 (3); forwards: fused 1, yardstick 2',
         '# median of %d rounds x %d launches [lowest .. highest round], the variants taking turns; no pass bar' % (args.rounds, args.reps)]
for r in grad:
    lines.append('B = %d chunk_rows %s: fused %s; forward + grad %s; fused / yardstick = %.2f; difference %+.4f ms, spread %.4f ms; pmg_ppo_stats_device %s' %
                 (r['B'], r['chunk_rows'], fmt(r['fused']), fmt(r['sequence']), r['fused']['ms_median'] / r['sequence']['ms_median'], r['difference_ms'], r['spread_ms'],
                  fmt(r['ppo_stats'])))
for r in gae:
    lines.append('pmg_gae_device T = %d N = %d (time-major, d_cut and d_ret given, %d bytes moved): %s = %.0f GB/s' %
                 (r['T'], r['N'], r['bytes'], fmt(r['gae']), r['bytes'] / r['gae']['ms_median'] / 1e6))
lines.append('M = %d: pmg_adv_stats_device %s; pmg_adv_apply_device %s' % (norm['M'], fmt(norm['stats']), fmt(norm['apply'])))
lines.append(json.dumps({'grad': grad, 'gae': gae, 'norm': norm}))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
