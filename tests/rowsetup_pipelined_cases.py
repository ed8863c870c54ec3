"""Cases and checks of the reach row set-up with and without PMG_ROWSETUP_PIPELINE (csrc/pmg_step_body.inc) -- TEST INFRASTRUCTURE,
shared by tests/test_rowsetup_pipelined_emulated.py / tests/test_gpu_rowsetup_pipelined.py (the set-up by itself, through the probe
prim::rowsetup_cases) and tests/test_reach_setup_kernels_emulated.py / tests/test_gpu_reach_setup_kernels.py (the three reach kernels).

The switch moves fetches and replaces branches by selects; it changes no arithmetic.  So a build with the switch on must give the
BITS of a build with the switch off -- every lane's coefficient table c24, response Rm, diagonal den, right-hand side rhs (and
1 / den, mu) at function level; states, observations, goals and rewards at kernel level -- and nothing here has a tolerance.

Function level: the twelve cases of tests/rowsetup_cases.py (six scenes on two poses: 1, 4, 5 and 8 contacts, finger 2 only,
tilted normals) and one with an EMPTY contact list (nc = 0: every lane must come back with exact zeros, the DoF lanes included).
Kernel level: the four pressed states of rowsetup_cases.pressed_states() (both fingers flat on the table, eight contacts), one env
step, on pmg_k_step_reach2, pmg_k_step_reach and pmg_k_redo (the way tests/reach_mfma_cases.py reaches each of them)."""
import ctypes as C

import numpy as np

import oracle_lib as O
import reach_mfma_cases as KC
import rowsetup_cases as RC

N_ENVS = 4
ACT_LOW = np.float32([[0.2, 0.1, -1.0], [-0.3, 0.2, -1.0], [0.1, -0.2, -1.0], [-0.1, -0.1, -1.0]])


def cases():
    """-> (names, dict(q, qd, con, mu, nc)): rowsetup_cases.cases() and the empty list on pose 0"""
    cs = RC.cases()
    names = list(cs['name']) + ['no contact, pose 0']
    out = {k: np.concatenate([cs[k], np.zeros_like(cs[k][:1])]) for k in ('con', 'mu', 'nc')}
    out['q'], out['qd'] = np.concatenate([cs['q'], cs['q'][:1]]), np.concatenate([cs['qd'], cs['qd'][:1]])
    assert sorted(set(out['nc'].tolist())) == [0, 1, 4, 5, 8] and len(names) == 2 * len(RC.SCENES) + 1
    return names, out


def run(fn, cs):
    """fn: pmge_rowsetup / pmgd_rowsetup on the cases `cs` -> dict(coef [n, 64, 24], resp [n, 64, 9], misc [n, 64, 4], S, minv)"""
    n = len(cs['nc'])
    out = dict(coef=np.full((n, 64, 24), -7777.0, np.float32), resp=np.full((n, 64, 9), -7777.0, np.float32), misc=np.full((n, 64, 4), -7777.0, np.float32),
               S=np.zeros((n, 9, 6), np.float32), minv=np.zeros((n, 9, 9), np.float32))
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    rc = fn(C.c_int(n), p(cs['q']), p(cs['qd']), p(cs['con']), p(cs['mu']), p(cs['nc']), p(out['coef']), p(out['resp']), p(out['misc']), p(out['S']), p(out['minv']))
    assert rc == 0, rc
    return out


def check_set_up_bit_equal(fn_on, fn_off, label, out=print):
    """every case through the switch-on and the switch-off probe: the same bits in every lane; the empty list: exact zeros"""
    names, cs = cases()
    on, off = run(fn_on, cs), run(fn_off, cs)
    for k in ('S', 'minv'):                                 # (the operands: the two builds worked from the same numbers)
        assert np.array_equal(on[k].view(np.uint32), off[k].view(np.uint32)), (label, k)
    for i, name in enumerate(names):
        nr = 3 * int(cs['nc'][i])
        for k, what in (('coef', 'c24'), ('resp', 'Rm'), ('misc', 'den / rhs / dinv / mu')):
            a, b = on[k][i], off[k][i]
            assert not (a == np.float32(-7777.0)).any(), (label, name, what, 'a lane wrote nothing')
            same = a.view(np.uint32) == b.view(np.uint32)
            assert same.all(), (label, name, what, 'lanes / entries that differ', np.argwhere(~same)[:6].tolist(),
                                float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))
        # rows that do not exist: exact zeros (as rowsetup_cases.check has it), in the switch-on build by itself
        coef, resp, misc = on['coef'][i], on['resp'][i], on['misc'][i]
        idle = np.concatenate([np.arange(9, 16), np.arange(16 + nr, 64)])
        assert (coef[:, nr:] == 0).all() and (coef[idle] == 0).all() and (misc[idle] == 0).all() and (resp[16 + nr:40] == 0).all(), (label, name)
        if nr == 0:
            assert (coef == 0).all() and (misc == 0).all() and (resp[16:40] == 0).all(), (label, name, 'an empty list leaves something behind')
        else:
            assert (misc[16:16 + nr, 0] > 0).all() and np.isfinite(coef).all() and np.isfinite(resp[16:16 + nr]).all(), (label, name)
        out('%-8s %-52s nc %d  c24, Rm, den, rhs, 1 / den, mu of all 64 lanes: the switch-off build\'s bits' % (label, name, nr // 3))
    return on


def scenes(high):
    """-> states [4, D] float32: the four pressed states; high: tip target 12 cm above the table (the plan's packed list -> pmg_k_redo)"""
    pressed, _ = RC.pressed_states()
    ora = O.OracleEnv('reach', N_ENVS, seed_base=11, seed_stride=1, max_episode_steps=1000)
    ora.reset(), ora.reset()
    st = ora.get_state().copy()
    ora.close()
    st[:] = pressed
    st[:, 29] = 0                                           # elapsed
    if high:
        st[:, 20] = np.float32(0.30)
    return st


def kernel_runs(pmg, library):
    """one env step of the four pressed envs on each reach kernel of `library` -> dict(two, one, redo): KC.step's records"""
    low, high = scenes(False), scenes(True)
    zero = np.zeros((N_ENVS, 3), np.float32)
    two = KC.step(pmg, library, low, ACT_LOW, {'PMG_REACH_TWO_WAVES': '1'})
    one = KC.step(pmg, library, low, ACT_LOW, {'PMG_REACH_TWO_WAVES': '0'})
    redo = KC.step(pmg, library, high, zero, {'PMG_PACKED': '1'})
    full = KC.step(pmg, library, high, zero, {'PMG_PACKED': '0'})
    every = np.arange(N_ENVS)
    assert np.array_equal(two['prone'], every) and np.array_equal(one['prone'], every), (two['prone'], one['prone'])
    assert np.array_equal(redo['redo'], every) and len(redo['prone']) == 0 and len(full['redo']) == 0, (redo['redo'], redo['prone'], full['redo'])
    for r in (two, one, redo, full):
        assert (r['nc'] == 8).all(), r['nc']                # both fingers flat on the table in every run
    return dict(two=two, one=one, redo=redo, full=full)


def check_kernels_bit_equal(pmg, lib_on, lib_off, label, out=print):
    """the three reach kernels agree with each other in the switch-on library, and each gives the switch-off library's bits"""
    on, off = kernel_runs(pmg, lib_on), kernel_runs(pmg, lib_off)
    KC._same_bits(on['two'], on['one'], label + ': pmg_k_step_reach2 against pmg_k_step_reach')
    KC._same_bits(on['redo'], on['full'], label + ': pmg_k_redo against pmg_k_step_reach')
    for k, kernel in (('two', 'pmg_k_step_reach2'), ('one', 'pmg_k_step_reach'), ('redo', 'pmg_k_redo'), ('full', 'pmg_k_step_reach, tip target up')):
        KC._same_bits(on[k], off[k], '%s: %s, switch on against switch off' % (label, kernel))
    assert (on['two']['state'][:, 9:18] != scenes(False)[:, 9:18]).any()      # the step moved the joints
    out('%s: pmg_k_step_reach2 = pmg_k_step_reach, pmg_k_redo = pmg_k_step_reach, and each the bits of the switch-off library (4 envs, 8 contacts each)' % label)
    return on


_EMU_OFF = {}


def emu_library_switch_off(root, tmp_path_factory):
    """the emulator build of the product sources (and the probe) with -DPMG_ROWSETUP_PIPELINE=0, built once per session
    (conftest.emu_library_small_rowspace's recipe) -> its path"""
    import os
    import subprocess
    if 'path' not in _EMU_OFF:
        out = str(tmp_path_factory.mktemp('emu_setup0') / 'libpmg_emu_setup0.so')
        emu, src = os.path.join(root, 'tests', 'emu'), os.path.join(root, 'pybullet_multigoal_gym_amd', 'csrc')
        subprocess.check_call(['g++', '-O2', '-fPIC', '-std=c++17', '-I' + emu, '-I' + src, '-Wno-unknown-pragmas', '-w', '-DPMG_ROWSETUP_PIPELINE=0',
                               '-shared', '-o', out, os.path.join(emu, 'hip_emu.cpp'), os.path.join(emu, 'pmg_probe.cpp'),
                               os.path.join(src, 'pmg_api.cpp'), '-x', 'c++', os.path.join(src, 'pmg_kernels.hip'), '-lrt'])
        _EMU_OFF['path'] = out
    return _EMU_OFF['path']
