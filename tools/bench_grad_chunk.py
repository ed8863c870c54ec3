#!/usr/bin/env python3
"""Time of the chunked batch reduction (pmg_mlp_grad_chunked_device: pmg_k_mlp_grad_rows + pmg_k_mlp_grad_partials + pmg_k_mlp_grad_merge;
DESIGN.md 3.12) next to its yardstick, the single chain (pmg_mlp_grad_device) timed in the SAME process on the SAME rows.

  networks, batches, rounds and reps of tools/bench_grad.py: critic Dx + A -> 3 x 256 -> 1 on cat rows (MSE head), actor Dx -> 3 x 256 -> A tanh
  on raw rows (d_gout head), for the input widths of reach (6, 3) and block_stack-4 (28, 4); B = 256, 4096, 65536; the full gradient (grads,
  d_gx / d_ga, d_out) with the single chain and with chunk_rows = 128, 256, 512, 1024.

Reported per row: ms per launch (median round [lowest .. highest]), the ratio to the single chain's median, the workspace bytes and the FLOP
rate of the full gradient (3 x the forward's FLOPs against the 157.3 TF f32 matrix peak); `faster` says whether the HIGHEST round lies below
the single chain's LOWEST.  `bench_grad_chunk.py [--out profiles/mlp_grad_chunked.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mlp_grad_chunked.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096, 65536])
ap.add_argument('--chunks', type=int, nargs='+', default=[128, 256, 512, 1024])
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


def tensors(h, widths, rs):
    d_w, d_b = [], []
    for l in range(len(widths) - 1):
        for a, out in (((rs.uniform(-1, 1, (widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32), d_w),
                       (rs.uniform(-0.1, 0.1, widths[l + 1]).astype(np.float32), d_b)):
            p = h.device_alloc(a.nbytes)
            h.upload(p, a)
            out.append(p)
    return d_w, d_b


def bench(h, name, Dx, A, B, kind):
    rs = np.random.RandomState(0)
    cat = kind == 'critic'
    widths = [Dx + A] + [args.hidden] * 3 + [1] if cat else [Dx] + [args.hidden] * 3 + [A]
    out_w = widths[-1]
    net, grads = tensors(h, widths, rs), tensors(h, widths, rs)
    mlp = h.mlp_struct(widths, net[0], net[1], 0 if cat else 1)
    gstruct = h.params_struct(*grads)
    bufs = {'x': (B, Dx), 'a': (B, A), 'head': (B, out_w), 'gx': (B, Dx), 'ga': (B, A), 'out': (B, out_w)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    for k in ('x', 'a', 'head'):
        h.upload(d[k], (rs.uniform(-1, 1, bufs[k]) * (1.0 / B if k == 'head' and not cat else 1.0)).astype(np.float32))
    works = {R: h.mlp_grad_chunked_work_floats(mlp, B, R) for R in args.chunks}
    works[0] = h.mlp_grad_work_floats(mlp, B)
    room = max(works.values())
    d['work'] = h.device_alloc(4 * room)
    common = dict(d_a=d['a'] if cat else None, a_stride=A if cat else 0, a_dim=A if cat else 0, d_gx=d['gx'], gx_stride=Dx, d_ga=d['ga'] if cat else None,
                  ga_stride=A if cat else 0)
    head = dict(d_target=d['head'], target_stride=out_w, gscale=2.0 / B) if cat else dict(d_gout=d['head'], gout_stride=out_w)
    full = h.grad_struct(B, d['x'], Dx, Dx, d['work'], room, grads=gstruct, d_out=d['out'], out_stride=out_w, **common, **head)
    flop = 3 * B * 2 * sum(widths[l] * widths[l + 1] for l in range(len(widths) - 1))
    res = {'shape': name, 'kind': kind, 'B': B, 'widths': widths, 'runs': []}
    for R in [0] + list(args.chunks):
        s = stats(timed(h, (lambda: h.mlp_grad_device(mlp, full)) if R == 0 else (lambda: h.mlp_grad_chunked_device(mlp, full, R))))
        s.update(R=R, chunks=1 if R == 0 else -(-B // R), work_MB=4 * works[R] / 1e6, TF=flop / (s['ms_median'] * 1e-3) / 1e12)
        res['runs'].append(s)
    single = res['runs'][0]
    for s in res['runs']:
        s['ratio'] = s['ms_median'] / single['ms_median']
        s['faster'] = bool(s['R'] and s['ms_max'] < single['ms_min'])
    for p in net[0] + net[1] + grads[0] + grads[1] + list(d.values()):
        h.device_free(p)
    return res


from pybullet_multigoal_gym_amd._lib import PmgLibrary
env = pmg.make_env(task='reach', num_envs=64, **({'_library': PmgLibrary(args.library)} if args.library else {}))
h = env.handle
res = [bench(h, name, Dx, A, B, kind) for name, Dx, A in SHAPES for kind in ('critic', 'actor') for B in args.batches]
env.close()
lines = ['# tools/bench_grad_chunk.py: the full gradient (grads, d_gx / d_ga, d_out) of critic Dx + A -> 3 x %d -> 1 (cat rows, MSE head) and actor Dx -> 3 x %d -> A' % (args.hidden, args.hidden),
         '# (tanh, raw rows, d_gout head) with the single chain (pmg_mlp_grad_device) and with pmg_mlp_grad_chunked_device at chunk_rows = %s, same process, same rows' % ', '.join(map(str, args.chunks)),
         '# median of %d rounds x %d launches [lowest .. highest round]; ratio = median / the single chain\'s median; TF = 3 x the forward FLOPs against the %.1f TF' % (args.rounds, args.reps, PEAK_TF),
         '# f32 matrix peak; faster = the highest round lies below the single chain\'s lowest round']
for r in res:
    for s in r['runs']:
        lines.append('%s %s %s B = %d %s: %.4f ms [%.4f .. %.4f], ratio %.3f, workspace %.1f MB, %.2f TF (%.1f %% of peak)%s' %
                     (r['shape'], r['kind'], '-'.join(map(str, r['widths'])), r['B'], 'single chain' if not s['R'] else 'chunk_rows %d (%d chunks)' % (s['R'], s['chunks']),
                      s['ms_median'], s['ms_min'], s['ms_max'], s['ratio'], s['work_MB'], s['TF'], 100 * s['TF'] / PEAK_TF, '' if not s['R'] else ', faster' if s['faster'] else ', not faster'))
for B in args.batches:
    ok = all(any(s['faster'] for s in r['runs']) for r in res if r['B'] == B)
    lines.append('# B = %d: %s' % (B, 'some chunk_rows is faster than the single chain for every network' if ok else 'NO chunk_rows is faster than the single chain for some network'))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
