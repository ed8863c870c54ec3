"""The reach contact step through the public API (shared by tests/test_gpu_contact_step.py, the device, and
tests/test_contact_step_emulated.py, the CPU emulator): a batch with every kind of env the step's schedule tells apart -- pressed onto
the table, contact-prone without touching, hovering, and given up by the packed path -- must come out bit for bit the same whichever
kernels carry it (the shipped schedule, PMG_REACH_TWO_WAVES=0, PMG_PACKED=0), whichever batch the env is in, and with the wavefront
trace (PMG_WAVE_TRACE) on or off; and the trace itself must name every live wavefront once.  No numeric bar: bits and integers."""
import os

import numpy as np

import oracle_lib
import schedule_cases as SC
from pybullet_multigoal_gym_amd._lib import PMG_BUF_WAVE_TRACE

DROPPED = 3
# the device's batch: 13 envs, three pressed, two prone, two given up, six hovering; then 1 env and 5 envs, all pressed
DEVICE = dict(N=13, pressed=[1, 6, 10], prone=[4, 8], given_up=[5, 11], small=((1, [0]), (5, [0, 1, 2, 3, 4])), short_all_settings=True)
# the emulator's (a pressed env costs it seconds): 7 envs with every kind, then 1 env and 2 envs; the shorter batch under the shipped schedule only
EMULATED = dict(N=7, pressed=[1, 5], prone=[4], given_up=[6], small=((1, [0]), (2, [0, 1])), short_all_settings=False)
SETTINGS = ({}, {'PMG_REACH_TWO_WAVES': '0'}, {'PMG_PACKED': '0'})
Z_CLIP = 0.175                                            # the lower clip plane of the tip target (kuka.py:209-212)


class _Environ:
    """switches that pmg_create reads from the environment, for the handles made inside"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plant_pressed(st, i):
    """the tip target at the lower clip plane and held there (a_z = -1), the arm posed 1 mm below it: both fingers on the table"""
    q, _ = oracle_lib.ik(st[i, :9].astype(float), [-0.52 + 0.01 * (i % 5), 0.02 * (i % 3), Z_CLIP - 0.001])
    st[i, :7] = q[:7]; st[i, 9:18] = 0; st[i, 18:21] = [-0.52 + 0.01 * (i % 5), 0.02 * (i % 3), Z_CLIP]; st[i, 21:28] = q[:7]


def plant_prone(st, i):
    """the tip target 10 mm above the clip plane (list 0 takes everything within 12 mm), the arm there: the fingers stay clear of the table"""
    q, _ = oracle_lib.ik(st[i, :9].astype(float), [-0.52, 0.03, Z_CLIP + 0.010])
    st[i, :7] = q[:7]; st[i, 9:18] = 0; st[i, 18:21] = [-0.52, 0.03, Z_CLIP + 0.010]; st[i, 21:28] = q[:7]


def batch(N, pressed, prone, given_up):
    """-> state [N, state_dim] and actions [N, 3] of the planted batch (from the reset state of an oracle env: no device needed)"""
    ora = oracle_lib.OracleEnv('reach', N, seed_base=0, seed_stride=1)
    ora.reset()
    ora.reset()
    st = ora.get_state().copy()
    ora.close()
    a = np.random.RandomState(5).uniform(-1, 1, (N, 3)).astype(np.float32)
    a[:, 2] = np.abs(a[:, 2])                              # hovering envs move level or up
    for i in pressed:
        plant_pressed(st, i)
        a[i] = [0, 0, -1]
    for i in prone:
        plant_prone(st, i)
        a[i] = 0
    for i in given_up:
        SC.plant_misplan(st, i)
        a[i] = 0
    return st, a


def step_once(library, st, a, trace=False, **switches):
    """one env step of the batch under the switches -> dict(state, rows, sched, nc, trace or None)"""
    N = len(st)
    env_kw = dict(switches, PMG_ENV_CYCLES='1')
    if trace:
        env_kw['PMG_WAVE_TRACE'] = '1'
    with _Environ(**env_kw):
        env = SC._make(library, 'reach', N, {})
    env.reset()
    env.set_state(st)
    o, r, d, info = env.step(a)
    h = env.handle
    rows = np.empty((N, env.dims.packed_dim), np.float32)
    h.sync()
    h.download(rows, h.device_ptr())
    res = dict(state=env.get_state(), rows=rows, sched=h.schedule(), nc=h.env_cycles()[:, 1].copy(), trace=None, no_trace_buffer=False)
    if trace:
        res['trace'] = h.wave_trace()
    else:
        try:
            h.device_ptr(PMG_BUF_WAVE_TRACE)
        except Exception:
            res['no_trace_buffer'] = True
    env.close()
    return res


def same_bits(x, y, label, rows_x=slice(None), rows_y=slice(None)):
    for k in ('state', 'rows'):
        a, b = SC._bits(x[k][rows_x]), SC._bits(y[k][rows_y])
        assert np.array_equal(a, b), '%s: %s differs in envs %s' % (label, k, np.nonzero((a != b).any(1))[0].tolist())


def check_lists(res, N, pressed, prone, given_up, label, packed=True):
    sch = res['sched']
    SC._partition(sch, N, label)
    if packed:
        assert sorted(sch['prone'].tolist()) == sorted(pressed + prone), (label, sch['prone'])
        assert sorted(sch['redo'].tolist()) == sorted(given_up), (label, sch['redo'])
    assert (res['nc'][pressed] > 0).all(), (label, 'a pressed env without contacts', res['nc'])
    assert (res['nc'][prone] == 0).all(), (label, 'a prone env touched the table', res['nc'])
    assert (res['state'][:, 29] == 1).all(), label          # every env stepped once (elapsed counts from the reset)


def check_shipped_schedule(library=None, case=DEVICE, out=print):
    """The batch (13 envs: 3 pressed, 2 prone, 2 given up, 6 hovering) and the reversed batch without its first three, one step each under the
    shipped schedule, PMG_REACH_TWO_WAVES=0 and PMG_PACKED=0: the same bits everywhere, the redo list = the planted give-ups.  Then 1 env
    pressed and 5 envs all pressed (list 1 empty).  (13 - 5 leaves list 1 at 8 envs; the shorter batch has 6: the ragged last packed wavefront.)"""
    N_FULL, PRESSED, PRONE, GIVEN_UP = case['N'], case['pressed'], case['prone'], case['given_up']
    st, a = batch(N_FULL, PRESSED, PRONE, GIVEN_UP)
    keep = np.arange(N_FULL)[DROPPED:][::-1].copy()
    where = {int(e): j for j, e in enumerate(keep)}
    sub = [[where[i] for i in lst if i in where] for lst in (PRESSED, PRONE, GIVEN_UP)]
    full = [step_once(library, st, a, **sw) for sw in SETTINGS]
    short = [step_once(library, st[keep], np.ascontiguousarray(a[keep]), **sw) for sw in (SETTINGS if case['short_all_settings'] else SETTINGS[:1])]
    for sw, f in zip(SETTINGS, full):
        out('%-32s %d envs: list 0 %s list 1 %s redo %s' % (sw or 'shipped', N_FULL, f['sched']['prone'].tolist(), f['sched']['free'].tolist(), f['sched']['redo'].tolist()))
        check_lists(f, N_FULL, PRESSED, PRONE, GIVEN_UP, 'full %s' % sw, packed='PMG_PACKED' not in sw)
        same_bits(f, full[0], 'full batch, %s against the shipped schedule' % sw)
    for sw, s in zip(SETTINGS, short):
        out('%-32s %d envs: list 0 %s list 1 %s redo %s' % (sw or 'shipped', len(keep), s['sched']['prone'].tolist(), s['sched']['free'].tolist(), s['sched']['redo'].tolist()))
        check_lists(s, len(keep), *sub, 'short %s' % sw, packed='PMG_PACKED' not in sw)
        same_bits(s, short[0], 'short batch, %s against the shipped schedule' % sw)
        same_bits(full[0], s, 'the same envs in either batch, %s' % sw, rows_x=keep)
    assert len(short[0]['sched']['free']) % 4 != 0 and len(full[0]['sched']['prone']) == len(PRESSED) + len(PRONE)
    for N, pressed in case['small']:
        st1, a1 = batch(N, pressed, [], [])
        runs = [step_once(library, st1, a1, trace=(not sw), **sw) for sw in SETTINGS]
        for sw, r in zip(SETTINGS, runs):
            check_lists(r, N, pressed, [], [], '%d envs %s' % (N, sw), packed='PMG_PACKED' not in sw)
            same_bits(r, runs[0], '%d pressed envs, %s' % (N, sw))
        assert len(runs[0]['sched']['free']) == 0
        roles = runs[0]['trace']['role']
        assert sorted(roles[roles >= 0].tolist()) == [0] * N + [1] * N, roles      # no packed and no redo wavefront did anything
    return full[0]


def _cu(rec):
    return (int(rec['xcc']) & 15, (int(rec['hw']) >> 8) & 0xFF)      # XCC_ID; CU_ID, SH_ID, SE_ID


def _simd(rec):
    return (int(rec['hw']) >> 4) & 3


def check_trace(library=None, case=DEVICE, out=print):
    """PMG_WAVE_TRACE=1 at 13 envs, one step: one record per live wavefront and no other; the switch off: no buffer, the same outputs."""
    N_FULL = case['N']
    st, a = batch(N_FULL, case['pressed'], case['prone'], case['given_up'])
    off, on = step_once(library, st, a), step_once(library, st, a, trace=True)
    assert off['no_trace_buffer']
    same_bits(on, off, 'traced against untraced')
    sch, tr = on['sched'], on['trace']
    l0, l1, redo = sch['prone'].tolist(), sch['free'].tolist(), sch['redo'].tolist()
    n0, groups = len(l0), (len(l1) + 3) // 4
    want = {}
    for b, env in enumerate(l0):                           # (which wavefront of the workgroup is the helper is the kernel's business)
        first = int(tr[2 * b]['role'])
        assert first in (0, 1), (b, tr[2 * b])
        want[2 * b], want[2 * b + 1] = (first, env), (1 - first, env)
    for g in range(groups):
        want[2 * n0 + g] = (2, l1[4 * g])
    for b, env in enumerate(redo):
        want[2 * N_FULL - 1 - b] = (3, env)
    assert len(want) == 2 * n0 + groups + len(redo) and len(tr) == 2 * N_FULL
    fill = np.frombuffer(b'\xff' * tr.dtype.itemsize, tr.dtype)[0]
    for slot in range(2 * N_FULL):
        r = tr[slot]
        if slot not in want:
            assert r.tobytes() == fill.tobytes(), ('an unused record was written', slot, r)
            continue
        assert (int(r['role']), int(r['env'])) == want[slot], (slot, r, want[slot])
        assert 0 <= r['t0'] <= r['t1'] and 0 <= r['c0'] <= r['c1'], (slot, r)
        assert r['kernel'] == (3 if want[slot][0] == 3 else 2), (slot, r)
        if want[slot][0] in (0, 3):
            assert r['nc'] == on['nc'][r['env']], (slot, r)
    for b in range(n0):                                    # wavefront 0 and its helper: one workgroup
        assert _cu(tr[2 * b]) == _cu(tr[2 * b + 1]) and _simd(tr[2 * b]) != _simd(tr[2 * b + 1]), (b, tr[2 * b], tr[2 * b + 1])
    for g in range(0, groups - 1, 2):                      # two packed wavefronts of one workgroup
        x, y = tr[2 * n0 + g], tr[2 * n0 + g + 1]
        assert _cu(x) == _cu(y) and _simd(x) != _simd(y), (g, x, y)
    out('trace: %d records of %d written; list 0 %s, list 1 %s, redo %s' % (len(want), len(tr), l0, l1, redo))
    return on
