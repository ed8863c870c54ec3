#!/usr/bin/env python3
"""Time of TD3's fused target (pmg_td3_target_device: pmg_k_td3_target) next to its yardstick, existing code timed in the
SAME process on the same rows: pmg_td_target_device (with d_next_action) followed by one pmg_q_device on (x', a') -- the least a caller does
today for two target critics, without the noise, the host min and the second epilogue, which favours the yardstick.

  networks: actor Dx -> 3 x 256 -> A (tanh), two critics Dx + A -> 3 x 256 -> 1, for the input widths of reach (6, 3) and block_stack-4
  (28, 4); B = 256, 4096, 65536; gamma 0.98, clips [-50, 0], d_terminal, every output given.

Variants, timed in turn within every round so that drift of the machine meets all of them alike:
  pair      pmg_td_target_device + pmg_q_device                                   (the yardstick)
  twin      pmg_td3_target_device, two critics, sigma 0
  twin_n    the same with sigma 0.2, noise_clip 0.5                               (what the noise costs: twin_n - twin)
  twin_ws   twin_n with d_next_action NULL: a~ kept in the workspace
  td        pmg_td_target_device alone
  one       pmg_td3_target_device, one critic, sigma 0                            (expected: td within the spread)

Reported: ms per launch (median round [lowest .. highest]), and for each comparison the difference of the medians next to the spread of the
rounds (highest - lowest, the larger of the two variants').  Bar: twin is not slower than pair by more than that spread.
`bench_td3.py [--out profiles/td3_target.txt] [--rounds 5] [--reps 20]`"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'td3_target.txt'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096, 65536])
ap.add_argument('--hidden', type=int, default=256)
ap.add_argument('--library', default=None, help='another build of the C ABI (tests/emu/libpmg_emu.so: a dry run of this script off the GPU)')
args = ap.parse_args()
assert args.rounds >= 5 and args.reps >= 20, 'at least 5 rounds of at least 20 launches'
SHAPES = (('reach', 6, 3), ('block_stack-4', 28, 4))
ORDER = ('pair', 'twin', 'twin_n', 'twin_ws', 'td', 'one')


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
    c1, p1 = upload_net(h, cw, rs, 0)
    c2, p2 = upload_net(h, cw, rs, 0)
    bufs = {'x': (B, Dx), 'r': (B,), 'y': (B,), 'qmin': (B,), 'q1': (B,), 'q2': (B,), 'na': (B, A), 'work': (B, A)}
    d = {k: h.device_alloc(4 * int(np.prod(s))) for k, s in bufs.items()}
    d['t'] = h.device_alloc(B)
    h.upload(d['x'], rs.uniform(-1, 1, bufs['x']).astype(np.float32))
    h.upload(d['r'], -rs.randint(0, 2, B).astype(np.float32))
    h.upload(d['t'], (rs.uniform(0, 1, B) < 0.1).astype(np.uint8))
    old = h.td_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, d['t'], d['q1'], d['na'])
    kw = dict(d_terminal=d['t'], d_q_min=d['qmin'], d_q1=d['q1'], d_q2=d['q2'])
    twin = h.td3_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.0, 0.5, 1, 2, 0, d_next_action=d['na'], **kw)
    twin_n = h.td3_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.2, 0.5, 1, 2, 0, d_next_action=d['na'], **kw)
    twin_ws = h.td3_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.2, 0.5, 1, 2, 0, d_work=d['work'], work_floats=B * A, **kw)
    one = h.td3_struct(B, d['x'], Dx, d['r'], d['y'], 0.98, -50.0, 0.0, 0.0, 0.5, 1, 2, 0, d_terminal=d['t'], d_q1=d['q1'], d_next_action=d['na'])

    def pair():
        h.td_target_device(actor, c1, old)
        h.q_device(c2, d['x'], Dx, Dx, d['na'], A, A, B, d['q2'], 1)
    ms = timed(h, {'pair': pair, 'twin': lambda: h.td3_target_device(actor, c1, c2, twin), 'twin_n': lambda: h.td3_target_device(actor, c1, c2, twin_n),
                   'twin_ws': lambda: h.td3_target_device(actor, c1, c2, twin_ws), 'td': lambda: h.td_target_device(actor, c1, old),
                   'one': lambda: h.td3_target_device(actor, c1, None, one)})
    res = {'shape': name, 'B': B, 'actor': aw, 'critic': cw, 'flop_per_row_twin': flops(aw) + 2 * flops(cw)}
    res.update({k: stats(v) for k, v in ms.items()})
    for p in pa + p1 + p2 + list(d.values()):
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
lines = ['# tools/bench_td3.py: pmg_td3_target_device (actor Dx -> 3 x %d -> A tanh, critics Dx + A -> 3 x %d -> 1; gamma 0.98, clips [-50, 0], d_terminal, every output)' % (args.hidden, args.hidden),
         '# pair = pmg_td_target_device (with d_next_action) + pmg_q_device of the second critic on (x\', a\'): the yardstick, same process, same rows',
         '# twin = two critics, sigma 0; twin_n = sigma 0.2, noise_clip 0.5; twin_ws = twin_n with a~ kept in the workspace; td = pmg_td_target_device alone; one = one critic, sigma 0',
         '# median of %d rounds x %d launches [lowest .. highest round], the variants taking turns within a round' % (args.rounds, args.reps)]
for r in res:
    lines.append('%s (Dx %d, A %d) B = %d: ' % (r['shape'], r['actor'][0], r['actor'][-1], r['B']) + '; '.join('%s %s' % (k, fmt(r[k])) for k in ORDER))
    lines.append('    ' + '; '.join((versus(r, 'twin', 'pair'), versus(r, 'one', 'td'), versus(r, 'twin_n', 'twin'), versus(r, 'twin_ws', 'twin_n'))))
    lines.append('    twin: %.2f TF of f32 matrix work (%d FLOP per row)' % (r['B'] * r['flop_per_row_twin'] / (r['twin']['ms_median'] * 1e-3) / 1e12, r['flop_per_row_twin']))
lines.append(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
print('\n'.join(lines[:-1]))
