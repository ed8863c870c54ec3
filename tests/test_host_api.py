"""CPU tier: host logic of the product package (no GPU compute)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pybullet_multigoal_gym_amd as pmg
from pybullet_multigoal_gym_amd import spaces
from pybullet_multigoal_gym_amd._lib import DEFAULT_LIBRARY, PmgConfig, PmgLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_library_loads_and_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(DEFAULT_LIBRARY)
    hdr = open(os.path.join(ROOT, 'include', 'pmg.h')).read()
    names = set(re.findall(r'\b(pmg_[a-z_]+)\s*\(', hdr))
    assert len(names) >= 23
    for n in sorted(names):
        assert hasattr(lib, n), n
    PmgLibrary()   # the typed binding agrees


def test_config_struct_matches_header_size(built):
    assert ctypes.sizeof(PmgConfig) == 88


def test_product_refuses_to_run_without_a_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(Exception) as e:
        pmg.make_env(task='reach', num_envs=2)
    assert 'HIP' in str(e.value) or 'device' in str(e.value)


def test_make_env_rejects_what_is_outside_the_hot_path(built):
    with pytest.raises(ValueError):
        pmg.make_env(task='fly')
    with pytest.raises(AssertionError):
        pmg.make_env(task='reach', gripper='claw')
    for kw in [dict(task='primitive_push_reach'), dict(task='insertion'), dict(gripper='robotiq85'),
               dict(render=True), dict(image_observation=True), dict(goal_image=True), dict(task_decomposition=True),
               dict(use_curriculum=True), dict(grip_informed_goal=True), dict(primitive='discrete_push')]:
        with pytest.raises(NotImplementedError):
            pmg.make_env(**kw)


def test_spaces():
    b = spaces.Box(-np.ones([4]), np.ones([4]))
    assert b.shape == (4,) and b.contains(np.zeros(4, np.float32)) and not b.contains(np.full(4, 1.5))
    assert b.sample().shape == (4,)
    d = spaces.Dict({'a': b})
    assert list(d.keys()) == ['a'] and d['a'] is b


def test_env_wrapper_shapes_and_errors_on_the_emulator(emu_library):
    """The Python host layer end to end, over the CPU emulator build of the same C ABI."""
    env = pmg.make_env(task='reach', num_envs=None, _library=emu_library)
    assert env.action_space.shape == (3,) and set(env.observation_space.keys()) >= {'observation', 'state', 'desired_goal'}
    with pytest.raises(AssertionError):
        env.step(np.zeros(3, np.float32))            # gym TimeLimit: step before reset
    o = env.reset()
    assert o['observation'].shape == (3,) and o['observation'].dtype == np.float32
    with pytest.raises(AssertionError):
        env.step(np.float32([0, 0, 2]))              # outside Box(-1, 1), kuka.py:168
    with pytest.raises(AssertionError):
        env.step(np.zeros(4, np.float32))
    r, ok = env._compute_reward(np.float32([0, 0, 0]), np.float32([0, 0, 0.01]))
    assert r.shape == () and r == 0 and bool(ok)
    assert env.seed(5) == [5]
    env.close()
    env64 = pmg.make_env(task='reach', num_envs=2, dtype='float64', _library=emu_library)
    assert env64.reset()['observation'].dtype == np.float64 and env64.reset()['observation'].shape == (2, 3)
    env64.close()


def test_integration_stub_config_matches_the_header():
    """The ctypes struct printed in INTEGRATION.md (what a reference maintainer would paste) must stay the pmg_config of
    include/pmg.h: same field names, same order, same size."""
    import ctypes as C
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'INTEGRATION.md')).read()
    ns = {'C': C}
    exec(re.search(r"class PmgConfig\(C.Structure\):.*?\n\n", src, re.S).group(0), ns)
    doc = ns['PmgConfig']
    from pybullet_multigoal_gym_amd._lib import PmgConfig
    assert C.sizeof(doc) == C.sizeof(PmgConfig) == 88
    assert [f[0] for f in doc._fields_] == [f[0] for f in PmgConfig._fields_]
    hdr = open(os.path.join(root, 'include', 'pmg.h')).read()
    body = hdr[hdr.index('typedef struct pmg_config {'):hdr.index('} pmg_config;')]
    names = re.findall(r'^\s+(?:u?int\d+_t|float)\s+(\w+)', body, re.M)
    assert names == [f[0] for f in PmgConfig._fields_]


def test_edge_case_inputs(emu_library):
    """Empty, ragged and degenerate inputs at the boundary (through the emulator build of the C ABI): an empty HER
    batch, goals with leading axes [T, N, G], a single un-batched pair, a reset with an all-false mask, goals exactly
    on the threshold, and shape errors raised before anything reaches the library."""
    import pybullet_multigoal_gym_amd as pmg
    env = pmg.make_env(task='reach', num_envs=3, seed=2, seed_stride=1, _library=emu_library)
    o = env.reset()
    r, ok = env._compute_reward(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert r.shape == (0,) and ok.shape == (0,)
    ag = np.random.RandomState(0).uniform(-0.1, 0.1, (5, 7, 3)).astype(np.float32)
    dg = np.zeros_like(ag)
    r, ok = env._compute_reward(ag, dg)
    d = np.linalg.norm(ag.astype(np.float64), axis=-1)
    assert r.shape == (5, 7) and np.array_equal(ok, ~(d > 0.05)) and np.array_equal(r, -(d > 0.05).astype(np.float32))
    r1, ok1 = env._compute_reward(ag[0, 0], dg[0, 0])
    assert r1.shape == () and ok1.shape == () and r1 == r[0, 0]
    # exactly on the threshold counts as achieved (not_achieved = d > threshold, kuka_single_step_base_env.py:240)
    r2, ok2 = env._compute_reward(np.float32([[0.05, 0, 0]]), np.float32([[0, 0, 0]]))
    assert ok2[0] and r2[0] == 0 and np.signbit(r2[0])                       # -0.0, as the reference's -float32(False)
    with pytest.raises(ValueError):
        env._compute_reward(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32))
    with pytest.raises(AssertionError):                                       # kuka_multi_step_base_env.py:339
        env._compute_reward(np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32))
    # a reset that selects nobody returns the current observations and leaves the state alone
    st = env.get_state()
    o2 = env.reset(mask=np.zeros(3, bool))
    assert all(np.array_equal(o[k], o2[k]) for k in o) and np.array_equal(st, env.get_state())
    with pytest.raises(AssertionError):
        env.step(np.zeros((2, 3), np.float32))                                # ragged batch
    with pytest.raises(AssertionError):
        env.step(np.full((3, 3), 1.5, np.float32))                            # outside the action space (kuka.py:168)
    env.close()
    single = pmg.make_env(task='reach', seed=2, _library=emu_library)         # the reference's un-batched shapes
    o1 = single.reset()
    assert o1['observation'].shape == (3,) and o1['desired_goal'].shape == (3,)
    ob, rr, dd, info = single.step(np.zeros(3, np.float32))
    assert ob['achieved_goal'].shape == (3,) and isinstance(dd, bool) and isinstance(info['goal_achieved'], bool)
    single.close()


def _checkpoint_round_trip(lib, task, N, steps_before, steps_after, **kw):
    """step, checkpoint, roll on with resets, restore (into the same env and into a fresh one) and roll on again:
    observations, goals, rewards, flags and curriculum state must continue bit-identically."""
    import warnings
    def make():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return pmg.make_env(task=task, num_envs=N, seed=3, seed_stride=1, _library=lib, max_episode_steps=4, **kw)
    env = make()
    if kw.get('use_curriculum'):
        env.activate_curriculum_update()
    A = env.dims.action_dim
    rs = np.random.RandomState(0)
    acts = rs.uniform(-1, 1, (steps_before + steps_after, N, A)).astype(np.float32)
    env.reset()
    for t in range(steps_before):
        env.step(acts[t])
    ck = env.get_checkpoint()

    def roll(e):
        out = []
        for t in range(steps_before, steps_before + steps_after):
            if (t - steps_before) == 1:
                out.append(e.reset(mask=np.arange(N) % 2 == 0))           # new goals from the restored RNG streams
            o, r, d, info = e.step(acts[t])
            out.append((o, r, d, info['goal_achieved']))
        if kw.get('use_curriculum'):
            out.append((e.curriculum_prob, e.num_generated_goals_per_curriculum, e.last_curriculum_level))
        return out

    def same(a, b):
        for x, y in zip(a, b):
            if isinstance(x, dict):
                x, y = (x,), (y,)
            for u, v in zip(x, y):
                if isinstance(u, dict):
                    for k in u:
                        assert np.array_equal(u[k], v[k]), k
                else:
                    assert np.array_equal(u, v)
    first = roll(env)
    env.set_checkpoint(ck)
    same(first, roll(env))
    fresh = make()
    fresh.set_checkpoint(ck)
    same(first, roll(fresh))
    bad = ck['rng'].copy()
    bad[0, 624] = 700                                       # a cursor beyond 624 is not an MT19937 state
    with pytest.raises(Exception):
        fresh.handle.set_rng(bad)
    with pytest.raises(ValueError):
        fresh.handle.set_rng(ck['rng'][:, :10])
    env.close(), fresh.close()


@pytest.mark.parametrize('task,kw', [('reach', {}), ('block_stack', {'num_block': 2, 'use_curriculum': True, 'num_goals_to_generate': 20})])
def test_emulated_checkpoint_round_trip(emu_library, task, kw):
    """pmg_get_state / pmg_set_state / pmg_get_rng / pmg_set_rng behind KukaVecEnv.get_checkpoint / set_checkpoint.  The
    packed tail of the LAST step (reward / goal_achieved / done) is not part of a checkpoint: it is undefined until the
    next step or reset, which is why the comparison starts with a step."""
    _checkpoint_round_trip(emu_library, task, 2 if task == 'reach' else 1, 1, 2, **kw)


def test_env_cycle_diagnostics_on_the_emulator(emu_library, monkeypatch):
    """PMG_ENV_CYCLES=1 at creation: every env's wavefront records its cycles and its largest contact count per step
    (PMG_BUF_ENV_CYCLES / h.env_cycles(), tools/env_cycles.py); without it the buffer does not exist."""
    from pybullet_multigoal_gym_amd._lib import PmgError
    env = pmg.make_env(task='push', num_envs=3, seed=2, _library=emu_library)
    env.reset()
    with pytest.raises(PmgError):
        env.handle.env_cycles()
    env.close()
    monkeypatch.setenv('PMG_ENV_CYCLES', '1')
    env = pmg.make_env(task='push', num_envs=3, seed=2, _library=emu_library)
    env.reset()
    a = np.zeros((3, 3), np.float32); a[:, 2] = -1.0                # down onto the table: fingers + block on the table
    for _ in range(3):
        env.step(a)
    c = env.handle.env_cycles()
    assert c.shape == (3, 2) and (c[:, 0] > 0).all()
    assert (c[:, 1] >= 4).all() and (c[:, 1] <= 24).all()           # the block's four table contacts at least
    env.close()


def test_dpp_hazard_checker_recognises_the_sequences():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_dpp_hazards as H
    blk = ';;#ASMSTART\ns_nop 1\nv_fmac_f32_dpp v1, v2, v3 row_newbcast:3 row_mask:0xf bank_mask:0xf\n;;#ASMEND\n'
    assert H.check('v_add_f32 v1, v2, v3\n' + blk) == (1, 0)
    assert H.check('v_cmpx_gt_f32 v1, v2\nv_add_f32 v4, v5, v6\n' + blk) == (1, 1)              # 1 + 2 (s_nop 1) < 5 wait states
    assert H.check('v_cmpx_gt_f32 v1, v2\ns_nop 3\n' + blk) == (1, 0)                           # 4 + 2 >= 5: covered
    assert H.check('s_mov_b64 exec, s[2:3]\nv_add_f32 v4, v5, v6\n' + blk) == (1, 1)
    assert H.check('v_add_f32 v4, v5, v6\n;;#ASMSTART\ns_nop 0\n;;#ASMEND\n') == (0, 0)          # not a DPP block
    # the binary-level walk (llvm-objdump text): every DPP instruction, both hazards
    dpp = 'v_mov_b32_dpp v1, v2 row_shr:1 row_mask:0xf bank_mask:0xf// 0000FFD0: 7E6402FA\n'
    assert H.check_binary('v_add_f32_e32 v9, v3, v4\n' + dpp) == (1, 0, 0, 0)
    assert H.check_binary('v_add_f32_e32 v2, v3, v4\n' + dpp) == (1, 0, 1, 0)                    # source written right before
    assert H.check_binary('v_add_f32_e32 v2, v3, v4\nv_mul_f32_e32 v8, v3, v4\n' + dpp) == (1, 0, 1, 0)   # one wait state: still short
    assert H.check_binary('v_add_f32_e32 v2, v3, v4\ns_nop 1\n' + dpp) == (1, 0, 0, 0)
    assert H.check_binary('v_pk_mul_f32 v[2:3], v[4:5], v[6:7]\ns_nop 0\n' + dpp) == (1, 0, 1, 0)  # register pairs
    assert H.check_binary('v_cmpx_gt_f32_e32 v1, v2\ns_nop 2\n' + dpp) == (1, 1, 0, 1)
    assert H.check_binary('v_cmpx_gt_f32_e32 v1, v2\ns_nop 4\n' + dpp) == (1, 0, 0, 1)


@pytest.mark.skipif(os.environ.get('PMG_SKIP_ISA_CHECK') == '1', reason='PMG_SKIP_ISA_CHECK=1')
def test_no_dpp_hazard_in_the_shipped_binary(built):
    """The inline-asm v_fmac_f32_dpp blocks of pmg_wave.h carry `s_nop 1` for the 2-wait-state hazard (VALU writes a VGPR,
    DPP reads it); the 5-wait-state one (VALU writes EXEC, then a DPP op) is invisible to the compiler's hazard
    recognizer inside inline asm.  tools/check_dpp_hazards.py cuts the gfx950 code objects out of the SHIPPED
    libpmg_hip.so, disassembles them and walks back from every DPP instruction (hand-written and compiler-made alike:
    ~21 000): neither hazard anywhere -- in fact no VALU instruction of the library writes EXEC at all.
    (`tools/check_dpp_hazards.py --compile` is the source-level variant on freshly compiled ISA text, by the ASM markers.)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_dpp_hazards as H
    ndpp, bad_exec, bad_src, valu_exec = H.check_binary(H.disassemble(os.path.join(ROOT, 'pybullet_multigoal_gym_amd', 'csrc', 'libpmg_hip.so')))
    assert ndpp > 10000 and bad_exec == 0 and bad_src == 0, (ndpp, bad_exec, bad_src, valu_exec)


def test_bench_plain_run_is_lean_and_dumps_its_last_step(built, tmp_path):
    """bench.py on the emulator build: a plain run prints the headline line without the secondary measurements, and
    --dump-outputs writes the last timed step's outputs as float32 .npy, the same in two runs with the same arguments;
    --full brings full_episodes / host_api back."""
    import json
    import subprocess
    import sys
    base = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--envs-per-gpu', '4',
            '--episode-steps', '2', '--lib', os.path.join(ROOT, 'tests', 'emu', 'libpmg_emu.so')]
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)

    def run(*extra):
        out = subprocess.run(base + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1
        return json.loads(lines[0])

    dumps = [tmp_path / 'a', tmp_path / 'b']
    for d in dumps:
        line = run('--dump-outputs', str(d))
        assert line['steps'] == 3 and line['roofline']['launches'] == 3
        assert abs(line['value'] - 4 * 3 / (line['ms_per_step'] * 3e-3)) < 1e-6 * line['value']
        for k in ('metric', 'unit', 'higher_is_better', 'dtype'):
            assert k in line, k
        for k in ('full_episodes', 'host_api', 'cpu_baseline'):
            assert k not in line, k
    names = {'observation': 3, 'policy_state': 3, 'achieved_goal': 3, 'desired_goal': 3, 'reward': 1, 'goal_achieved': 1, 'done': 1}
    assert sorted(p.name for p in dumps[0].iterdir()) == sorted(n + '.npy' for n in names)
    for n, width in names.items():
        a, b = np.load(dumps[0] / (n + '.npy')), np.load(dumps[1] / (n + '.npy'))
        assert a.dtype == np.float32 and a.shape[0] == 4 and (a.ndim == 1) == (width == 1), n
        assert np.array_equal(a, b), n
    assert np.isin(np.load(dumps[0] / 'done.npy'), (0.0, 1.0)).all()
    line = run('--full', '--no-cpu-baseline')
    assert line['full_episodes']['steps'] == 4 and line['host_api']['steps'] == 2 and 'cpu_baseline' not in line
