"""Which wavefront ends a reach step, where it ran and who shared its SIMD?  (GPU box; PMG_WAVE_TRACE=1 is set here.)
   python tools/wave_trace.py [--case bench|one_pressed|pressed64|all] [--steps 32] [--lib L]
bench: bench.py's loop (4096 envs, seed 0, random-policy table of seed 12345, staggered 50-step episodes, reset_done_device), the
trace read back after each of the last --steps steps.  one_pressed: env 0 of 4096 pressed onto the table (a_z = -1 for 12 steps,
then held), the others hovering; pressed64: 64 envs, all pressed.  `all` starts one fresh process per case.
Times are the constant-rate clock's (100 MHz: 10 ns a tick) relative to the step's first wavefront."""
import argparse
import collections
import os
import subprocess
import sys

os.environ['PMG_WAVE_TRACE'] = '1'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

TICK_US = 0.01
ROLE = 'WHPR'     # wavefront 0 of a list-0 env, its helper, packed, redo


def simd_key(r):
    hw = r['hw'].astype(np.int64)
    return ((r['xcc'].astype(np.int64) & 15) << 12) | (((hw >> 13) & 7) << 9) | (((hw >> 12) & 1) << 8) | (((hw >> 8) & 15) << 4) | ((hw >> 4) & 3)


def place(key):
    return 'xcd %d se %d sh %d cu %2d simd %d' % (key >> 12, (key >> 9) & 7, (key >> 8) & 1, (key >> 4) & 15, key & 3)


def analyse(rec, n_simds, out):
    """One step's records -> a dict of figures; `out` gets the step's lines."""
    r = rec[rec['role'] >= 0]
    if len(r) == 0:
        return None
    t_begin = r['t0'].min()
    t0, t1 = (r['t0'] - t_begin) * TICK_US, (r['t1'] - t_begin) * TICK_US
    dur = t1 - t0
    key = simd_key(r)
    last = int(t1.argmax())
    same = r['role'] == r['role'][last]
    med = float(np.median(dur[same]))
    mates = [j for j in np.nonzero(key == key[last])[0] if j != last and min(t1[j], t1[last]) > max(t0[j], t0[last])]
    mate_s = ', '.join('%s env %d nc %d for %.0f us' % (ROLE[r['role'][j]], r['env'][j], r['nc'][j], min(t1[j], t1[last]) - max(t0[j], t0[last])) for j in mates) or 'nobody'
    res = collections.Counter()
    for k in np.unique(key):
        res[''.join(sorted(ROLE[x] for x in r['role'][key == k]))] += 1
    used = sum(res.values())
    contact = (r['role'] == 0) & (r['nc'] > 0)
    w0_end = float(t1[contact].max()) if contact.any() else float('nan')
    w0_dur = float(dur[contact].max()) if contact.any() else float('nan')
    out('  ends last: %s env %d nc %d on %s | ran %.1f us (cycles %d), its role\'s median %.1f us | started +%.1f us | SIMD shared with: %s'
        % (ROLE[r['role'][last]], r['env'][last], r['nc'][last], place(int(key[last])), dur[last], r['c1'][last] - r['c0'][last], med, t0[last], mate_s))
    out('  step %.1f us first start to last end | slowest contact wavefront 0 ends %.1f us (ran %.1f): %.1f us before the step | wavefronts %s | SIMDs by residents: idle %d %s'
        % (t1.max(), w0_end, w0_dur, t1.max() - w0_end, dict(collections.Counter(ROLE[x] for x in r['role'])), max(0, n_simds - used),
           ' '.join('%s:%d' % kv for kv in sorted(res.items(), key=lambda kv: (len(kv[0]), kv[0])))))
    return dict(step_us=float(t1.max()), last_role=ROLE[r['role'][last]], last_nc=int(r['nc'][last]), last_shared=len(mates), last_dur=float(dur[last]), role_median=med,
                gap_us=float(t1.max() - w0_end), w0_dur=w0_dur, doubled=sum(v for k, v in res.items() if len(k) >= 2), late_us=float(t0[last]))


def run_case(case, steps, lib):
    import pybullet_multigoal_gym_amd as pmg
    from pybullet_multigoal_gym_amd._lib import PmgLibrary
    bench = case == 'bench'
    N, T = (64 if case == 'pressed64' else 4096), 50
    env = pmg.make_env(task='reach', num_envs=N, num_block=4, device=0, seed=0, seed_stride=1, env_index_offset=0,
                       max_episode_steps=T if bench else 1000000, binary_reward=True, _library=PmgLibrary(lib) if lib else None)
    h, A = env.handle, env.dims.action_dim
    n_simds = 1024
    W = 50 if bench else 30                                  # bench.py's warm-up; pressed: 12 steps down, then held
    P = T if bench else 0
    if bench:
        table = np.random.RandomState(12345).uniform(-1, 1, (P + W + steps, N, A)).astype(np.float32)
        m = np.stack([((np.arange(N) + p) % T == 0) for p in range(T)]).astype(np.uint8)
        masks = h.device_alloc(m.nbytes)
        h.upload(masks, m)
    else:
        table = np.zeros((W + steps, N, A), np.float32)
        table[:12, (slice(None) if case == 'pressed64' else 0), 2] = -1.0
    actions = h.device_alloc(table.nbytes)
    h.upload(actions, table)
    stride = N * A * 4
    h.timing_every(1)
    h.reset_device(None)
    figs = []
    print('## %s: %d envs, %d traced steps behind %d others' % (case, N, steps, P + W))
    for t in range(P + W + steps):
        if t == P + W:
            h.sync()
            h.timing_reset()
        h.step_device(actions + t * stride)
        if bench and t < P:
            h.reset_device(masks + ((t + 1) % T) * N)
        elif bench:
            h.reset_done_device()
        if t >= P + W:
            rec, sch = h.wave_trace(), h.schedule()
            print('step %d: list 0 %d, packed %d, redo %d' % (t - P - W, len(sch['prone']), len(sch['free']), len(sch['redo'])))
            f = analyse(rec, n_simds, print)
            if f:
                f['n0'] = len(sch['prone'])
                figs.append(f)
    kmin, kavg, kmax, _ = h.timing_stats()
    env.close()
    c = [f for f in figs if f['n0'] > 0]
    print('# %s summary: HIP-event kernel ms min / avg / max %.4f / %.4f / %.4f (traced, read back every step)' % (case, kmin, kavg, kmax))
    if c:
        print('# contact steps %d of %d: step %.1f us mean | last wavefront by role %s, with a SIMD partner in %d | its run %.1f us against its role\'s median %.1f | '
              'slowest contact wavefront 0 ran %.1f us and ended %.1f us (mean; max %.1f) before the step | SIMDs with >= 2 wavefronts %.0f mean | last wavefront started +%.1f us'
              % (len(c), len(figs), np.mean([f['step_us'] for f in c]), dict(collections.Counter(f['last_role'] for f in c)), sum(f['last_shared'] > 0 for f in c),
                 np.mean([f['last_dur'] for f in c]), np.mean([f['role_median'] for f in c]), np.nanmean([f['w0_dur'] for f in c]), np.nanmean([f['gap_us'] for f in c]),
                 np.nanmax([f['gap_us'] for f in c]), np.mean([f['doubled'] for f in c]), np.mean([f['late_us'] for f in c])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['bench', 'one_pressed', 'pressed64', 'all'])
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--lib', default=None)
    args = ap.parse_args()
    if args.case != 'all':
        return run_case(args.case, args.steps, args.lib)
    for case in ('bench', 'one_pressed', 'pressed64'):       # a fresh process per case, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), '--case', case, '--steps', str(args.steps)] + (['--lib', args.lib] if args.lib else [])
        rc = subprocess.run(cmd, timeout=240).returncode
        if rc != 0:
            sys.exit('wave_trace.py: case %s ended with %d: nothing more is started' % (case, rc))


if __name__ == '__main__':
    main()
