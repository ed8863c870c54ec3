#!/usr/bin/env python3
"""Time of the data-parallel merge on ONE GPU with R = 2, 4, 8 ranks simulated as slots, next to its yardstick, pmg_k_adam alone
(pmg_mlp_adam_device), timed in the SAME process on the SAME tensors.

  networks: HER's actor Dx -> 3 x 256 -> A and critic Dx + A -> 3 x 256 -> 1 at the widths of reach (6, 3)
  separate: pmg_mlp_params_pack_device + pmg_mlp_params_merge_device + pmg_mlp_adam_device          (3 launches)
  fused:    pmg_mlp_params_pack_device + pmg_mlp_adam_merge_device                                  (2 launches)
  adam:     pmg_mlp_adam_device                                                                     (1 launch)

The all-gather between pack and merge is NOT part of any row: with one GPU there is none to time, and the all-gather at nranks > 1 is unmeasured
on hardware.  Every round times the three variants one after the other, so that a drift of the machine meets all of them.  Reported per row: ms
per call sequence (median round [lowest .. highest]), the ratio to adam's median, and the bytes the sweeps of the row move by their formulas
over the median time (fused: pack reads P and writes P, the sweep reads (R + 3) P and writes 3 P floats).
`bench_dp.py [--out profiles/dp_merge.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dp_merge.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--ranks', type=int, nargs='+', default=[2, 4, 8])
ap.add_argument('--hidden', type=int, default=256)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'
Dx, A = 6, 3


def tensors(h, widths, rs, lo, hi):
    d_w, d_b = [], []
    for l in range(len(widths) - 1):
        for shape, out in (((widths[l + 1], widths[l]), d_w), ((widths[l + 1],), d_b)):
            a = rs.uniform(lo, hi, shape).astype(np.float32)
            p = h.device_alloc(a.nbytes)
            h.upload(p, a)
            out.append(p)
    return d_w, d_b


def bench(h, kind, R):
    rs = np.random.RandomState(0)
    widths = [Dx + A] + [args.hidden] * 3 + [1] if kind == 'critic' else [Dx] + [args.hidden] * 3 + [A]
    sets = {k: tensors(h, widths, rs, lo, hi) for k, (lo, hi) in {'p': (-0.1, 0.1), 'g': (-0.1, 0.1), 'm': (-0.05, 0.05), 'v': (1e-3, 1e-2), 'sum': (0, 0)}.items()}
    mlp = h.mlp_struct(widths, sets['p'][0], sets['p'][1], 0)
    S = {k: h.params_struct(*t) for k, t in sets.items()}
    P = h.mlp_param_floats(mlp)
    slots = rs.uniform(-0.1 / R, 0.1 / R, (R, P)).astype(np.float32)
    d_work = h.device_alloc(4 * (R + 1) * P)                       # the layout of the all-reduce: this rank's flat gradient, then R slots
    h.upload(d_work + 4 * P, slots)
    adam = h.adam_struct(1e-3, 1000)
    d_slots = d_work + 4 * P

    def separate():
        h.mlp_params_pack_device(mlp, S['g'], d_work)
        h.mlp_params_merge_device(mlp, d_slots, P, R, S['sum'])
        h.mlp_adam_device(mlp, S['p'], S['sum'], S['m'], S['v'], adam)

    def fused():
        h.mlp_params_pack_device(mlp, S['g'], d_work)
        h.mlp_adam_merge_device(mlp, S['p'], d_slots, P, R, None, S['m'], S['v'], adam)

    def alone():
        h.mlp_adam_device(mlp, S['p'], S['g'], S['m'], S['v'], adam)
    variants = (('separate', separate, 3, (2 + R + 1 + 4 + 3) * P), ('fused', fused, 2, (2 + R + 3 + 3) * P), ('adam', alone, 1, 7 * P))
    for _, launch, _, _ in variants:
        for _ in range(args.warmup):
            launch()
    h.sync()
    ms = {name: [] for name, _, _, _ in variants}
    for _ in range(args.rounds):
        for name, launch, _, _ in variants:
            h.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                launch()
            h.sync()
            ms[name].append((time.perf_counter() - t0) / args.reps * 1e3)
    res = {'kind': kind, 'widths': widths, 'P': P, 'R': R, 'runs': []}
    for name, _, launches, floats in variants:
        med = float(np.median(ms[name]))
        res['runs'].append({'variant': name, 'launches': launches, 'ms_median': med, 'ms_min': float(min(ms[name])), 'ms_max': float(max(ms[name])),
                            'MB': 4 * floats / 1e6, 'GBps': 4 * floats / (med * 1e-3) / 1e9})
    base = res['runs'][-1]['ms_median']
    for s in res['runs']:
        s['ratio'] = s['ms_median'] / base
    for t in sets.values():
        for p in t[0] + t[1]:
            h.device_free(p)
    h.device_free(d_work)
    return res


from pybullet_multigoal_gym_amd._lib import PmgLibrary
env = pmg.make_env(task='reach', num_envs=64, **({'_library': PmgLibrary(args.library)} if args.library else {}))
h = env.handle
res = [bench(h, kind, R) for kind in ('actor', 'critic') for R in args.ranks]
env.close()
lines = ['# tools/bench_dp.py: one Adam step from the gradients of R ranks simulated as slots on ONE GPU, actor %d -> 3 x %d -> %d and critic %d -> 3 x %d -> 1:' % (Dx, args.hidden, A, Dx + A, args.hidden),
         '# separate = pack + pmg_k_params_merge_ranks + pmg_k_adam, fused = pack + pmg_k_adam_merge_ranks, adam = pmg_k_adam alone (the yardstick), same process, same tensors',
         '# host clock around %d call sequences that end in a synchronise; median of %d rounds [lowest .. highest round], the variants alternating within a round;' % (args.reps, args.rounds),
         '# ratio = median / adam\'s median; MB = the floats the row\'s sweeps read and write by their formulas, GB/s = that over the median',
         '# NOT in any row: the all-gather between pack and merge.  The all-gather itself at nranks > 1 is unmeasured on hardware.']
for r in res:
    for s in r['runs']:
        lines.append('%s %s P = %d R = %d %-8s (%d launches): %.4f ms [%.4f .. %.4f], ratio %.2f, %.2f MB, %.1f GB/s' %
                     (r['kind'], '-'.join(map(str, r['widths'])), r['P'], r['R'], s['variant'], s['launches'], s['ms_median'], s['ms_min'], s['ms_max'], s['ratio'], s['MB'], s['GBps']))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
