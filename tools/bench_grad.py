#!/usr/bin/env python3
"""Time of back-propagation, Adam and Polyak (pmg_mlp_grad_device: pmg_k_mlp_grad_rows + pmg_k_mlp_grad_weights; pmg_mlp_adam_device;
pmg_mlp_polyak_device) next to their yardsticks, existing code timed in the SAME process on the SAME rows: pmg_q_device /
pmg_mlp_forward_device (the forward alone) for the gradient, pmg_device_copy of the network's bytes for the elementwise sweeps.

  networks: critic Dx + A -> 3 x 256 -> 1 on cat rows (MSE head), actor Dx -> 3 x 256 -> A tanh on raw rows (d_gout head), for the input
  widths of reach (6, 3) and block_stack-4 (28, 4); B = 256, 4096, 65536; the full gradient (grads, d_gx / d_ga, d_out) and the input-only
  gradient (grads NULL).

Reported: ms per launch (median round [lowest .. highest]); the FLOP rate of the full gradient counts 3 x the forward's FLOPs (forward, the
transposed chain, dW) against the 157.3 TF f32 matrix peak.  `bench_grad.py [--out profiles/mlp_grad.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mlp_grad.txt'))
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


class Tensors:
    def __init__(self, h, widths, rs, scale):
        self.h, self.d_w, self.d_b, self.floats = h, [], [], 0
        for l in range(len(widths) - 1):
            w = (rs.uniform(-1, 1, (widths[l + 1], widths[l])) * scale / np.sqrt(widths[l])).astype(np.float32)
            b = (rs.uniform(-0.1, 0.1, widths[l + 1]) * scale).astype(np.float32)
            for a, out in ((w, self.d_w), (b, self.d_b)):
                p = h.device_alloc(a.nbytes)
                h.upload(p, np.abs(a) if scale < 0 else a)
                out.append(p)
                self.floats += a.size
        self.struct = h.params_struct(self.d_w, self.d_b)

    def free(self):
        for p in self.d_w + self.d_b:
            self.h.device_free(p)


def flops(widths):
    return 2 * sum(widths[l] * widths[l + 1] for l in range(len(widths) - 1))


def bench(h, name, Dx, A, B, kind):
    rs = np.random.RandomState(0)
    widths = [Dx + A] + [args.hidden] * 3 + [1] if kind == 'critic' else [Dx] + [args.hidden] * 3 + [A]
    out_w = widths[-1]
    net, grads, m, v, target = (Tensors(h, widths, rs, s) for s in (1.0, 1.0, 0.1, -0.01, 1.0))
    mlp = h.mlp_struct(widths, net.d_w, net.d_b, 0 if kind == 'critic' else 1)
    bufs = {'x': (B, Dx), 'a': (B, A), 'head': (B, out_w), 'gx': (B, Dx), 'ga': (B, A), 'out': (B, out_w), 'q': (B, out_w)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    for k in ('x', 'a', 'head'):
        h.upload(d[k], (rs.uniform(-1, 1, bufs[k]) * (1.0 / B if k == 'head' and kind == 'actor' else 1.0)).astype(np.float32))
    work = h.mlp_grad_work_floats(mlp, B)
    d['work'] = h.device_alloc(4 * work)
    cat = kind == 'critic'
    common = dict(d_a=d['a'] if cat else None, a_stride=A if cat else 0, a_dim=A if cat else 0, d_gx=d['gx'], gx_stride=Dx, d_ga=d['ga'] if cat else None,
                  ga_stride=A if cat else 0)
    head = dict(d_target=d['head'], target_stride=out_w, gscale=2.0 / B) if cat else dict(d_gout=d['head'], gout_stride=out_w)
    full = h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, grads=grads.struct, d_out=d['out'], out_stride=out_w, **common, **head)
    inputs = h.grad_struct(B, d['x'], Dx, Dx, d['work'], work, **common, **head)
    res = {'shape': name, 'kind': kind, 'B': B, 'widths': widths, 'flop_per_row_forward': flops(widths), 'work_MB': 4 * work / 1e6, 'param_floats': net.floats}
    res['full'] = stats(timed(h, lambda: h.mlp_grad_device(mlp, full)))
    res['input_only'] = stats(timed(h, lambda: h.mlp_grad_device(mlp, inputs)))
    if cat:
        res['forward'] = stats(timed(h, lambda: h.q_device(mlp, d['x'], Dx, Dx, d['a'], A, A, B, d['q'], 1)))
    else:
        res['forward'] = stats(timed(h, lambda: h.mlp_forward_device(mlp, d['x'], Dx, B, d['q'], out_w)))
    res['full']['TF'] = 3 * B * res['flop_per_row_forward'] / (res['full']['ms_median'] * 1e-3) / 1e12
    if B == args.batches[0]:
        adam = h.adam_struct(1e-3, 7)
        res['adam'] = stats(timed(h, lambda: h.mlp_adam_device(mlp, net.struct, grads.struct, m.struct, v.struct, adam)))
        res['polyak'] = stats(timed(h, lambda: h.mlp_polyak_device(mlp, target.struct, 0.05)))
        nbytes = 4 * net.floats
        src, dst = h.device_alloc(nbytes), h.device_alloc(nbytes)
        res['copy'] = stats(timed(h, lambda: h.device_copy(dst, src, nbytes)))
        h.device_free(src)
        h.device_free(dst)
    for t in (net, grads, m, v, target):
        t.free()
    for p in d.values():
        h.device_free(p)
    return res


from pybullet_multigoal_gym_amd._lib import PmgLibrary
env = pmg.make_env(task='reach', num_envs=64, **({'_library': PmgLibrary(args.library)} if args.library else {}))
h = env.handle
fmt = lambda s: '%.4f ms [%.4f .. %.4f]' % (s['ms_median'], s['ms_min'], s['ms_max'])
res = [bench(h, name, Dx, A, B, kind) for name, Dx, A in SHAPES for kind in ('critic', 'actor') for B in args.batches]
env.close()
lines = ['# tools/bench_grad.py: pmg_mlp_grad_device (critic Dx + A -> 3 x %d -> 1 on cat rows, MSE head; actor Dx -> 3 x %d -> A tanh on raw rows, d_gout head):' % (args.hidden, args.hidden),
         '# the full gradient (grads, d_gx / d_ga, d_out) and the input-only gradient (grads NULL) next to the forward alone on the same rows (pmg_q_device /',
         '# pmg_mlp_forward_device), same process; pmg_mlp_adam_device and pmg_mlp_polyak_device per network next to pmg_device_copy of the same bytes',
         '# median of %d rounds x %d launches [lowest .. highest round]; TF of the full gradient = 3 x the forward FLOPs against the %.1f TF f32 matrix peak' % (args.rounds, args.reps, PEAK_TF)]
for r in res:
    lines.append('%s %s %s B = %d (workspace %.1f MB): full %s = %.2f TF (%.1f %% of peak); input-only %s; forward %s; full / forward = %.2f, input-only / forward = %.2f' %
                 (r['shape'], r['kind'], '-'.join(map(str, r['widths'])), r['B'], r['work_MB'], fmt(r['full']), r['full']['TF'], 100 * r['full']['TF'] / PEAK_TF, fmt(r['input_only']),
                  fmt(r['forward']), r['full']['ms_median'] / r['forward']['ms_median'], r['input_only']['ms_median'] / r['forward']['ms_median']))
    if 'adam' in r:
        lines.append('%s %s %d parameters (%.2f MB): adam %s; polyak %s; device_copy of the same bytes %s' %
                     (r['shape'], r['kind'], r['param_floats'], 4 * r['param_floats'] / 1e6, fmt(r['adam']), fmt(r['polyak']), fmt(r['copy'])))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
