"""CPU tier: the kernels that run several wavefronts per workgroup, under permuted wavefront order.

The fiber emulator's default scheduler resumes the fibers of a workgroup in index order, so every LDS hand-over between two
wavefronts is met under ONE interleaving.  pmge_set_wave_order (tests/emu/hip_emu.cpp) runs the wavefronts by a priority list
instead: each wavefront goes from one workgroup barrier to its next before any wavefront behind it in the list moves.  For a write
in wavefront a and a read in wavefront b between the same two barriers the identity list puts one of them first and the reverse
list the other, so the two together show every such pair that changes a result; kernels of up to three wavefronts run all n!
lists.  A kernel whose hand-overs are all fenced by barriers gives the same bits under every list and under the default
scheduler: that is what every case here requires -- of states, outputs, rewards, dones and the generators' words."""
import contextlib
import ctypes as C
import itertools
import warnings

import numpy as np
import pytest

import actor_cases as AC
import her_cases as HC
import normalizer_cases as NC
import oracle_lib as O
import pybullet_multigoal_gym_amd as pmg
import td_cases as TC
from pybullet_multigoal_gym_amd._lib import PmgHandle

PAIR = ((0, 1), (1, 0))
TRIPLES = tuple(itertools.permutations(range(3)))
FOUR = ((0, 1, 2, 3), (3, 2, 1, 0))
SIXTEEN = (tuple(range(16)), tuple(range(15, -1, -1)))
POSE_BAR, TWIST_BAR = 1e-4, 1e-3         # the free-flight puck against the float64 oracle (test_slide_free_flight_...)


class Waves:
    def __init__(self, emu_library):
        self.lib = C.CDLL(emu_library.path)
        self.lib.pmge_wave_order_launches.restype = C.c_longlong

    def set(self, order):
        arr = (C.c_int * max(len(order), 1))(*order)
        self.lib.pmge_set_wave_order(arr, C.c_int(len(order)))

    def launches(self):
        return int(self.lib.pmge_wave_order_launches())

    @contextlib.contextmanager
    def order(self, order):
        """the launches inside run under `order` (None: the default scheduler); the default scheduler is back afterwards"""
        self.set(order or ())
        try:
            yield
        finally:
            self.set(())


@pytest.fixture(scope='module')
def waves(emu_library):
    w = Waves(emu_library)
    yield w
    w.set(())


def _equal(got, want, label):
    assert list(got) == list(want), (label, list(got), list(want))
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        same = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
        where = [] if same or a.shape != b.shape else np.argwhere(a != b)[:4].tolist()
        worst = 0.0 if same or a.shape != b.shape else float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
        assert same, 'wavefront order %s: %r differs from the default scheduler at %s, by up to %.3g' % (label, k, where, worst)


def _under_orders(waves, orders, run, check=None):
    """run() under the default scheduler and under every list of `orders`: same bits.  `check(result, label)` (the case's own
    assertions) is applied to every run.  -> the default scheduler's result"""
    before = waves.launches()
    base = run()
    assert waves.launches() == before                    # (the default scheduler does not count)
    if check:
        check(base, 'default')
    for order in orders:
        before = waves.launches()
        with waves.order(order):
            got = run()
        assert waves.launches() > before, order          # workgroups of several wavefronts did run under the list
        if check:
            check(got, order)
        _equal(got, base, order)
    return base


# ----------------------------------------------------------------------------------------------------------------------
# the detector itself
def test_the_order_tells_an_unfenced_handover_and_leaves_a_fenced_one_alone(waves):
    """Two probe kernels of the emulator build (tests/emu/pmg_probe.cpp, 128 threads): wavefront 1 writes an LDS word, wavefront 0
    reads it between the same two barriers.  Without a barrier between write and read the lists 01 and 10 give different words (the
    initial 7 when the reader runs first, the writer's 42 otherwise); with one, every list and the default scheduler give 42."""
    def probe(name, order):
        out = (C.c_int * 1)(-1)
        with waves.order(order):
            getattr(waves.lib, name)(out)
        return out[0]
    before = waves.launches()
    assert probe('pmge_probe_handover_racy', (0, 1)) == 7 and probe('pmge_probe_handover_racy', (1, 0)) == 42
    assert probe('pmge_probe_handover_racy', (1,)) == 42            # (a wavefront that is not named follows the named ones)
    assert [probe('pmge_probe_handover_fenced', o) for o in (None, (0, 1), (1, 0))] == [42, 42, 42]
    assert waves.launches() - before == 5                           # the five launches under a list, not the default one
    assert probe('pmge_probe_handover_racy', None) == probe('pmge_probe_handover_racy', (0, 1))   # the default: index order


# ----------------------------------------------------------------------------------------------------------------------
# the step kernels
def _make(emu_library, task, N, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return pmg.make_env(task=task, num_envs=N, seed=3, seed_stride=1, _library=emu_library, **kw)


def _rollout(emu_library, task, N, kw, state, actions, lists=None):
    """N envs of `task` from `state` (an [N, state_dim] array, or a function that edits the state after the reset) through
    `actions` -> everything the steps left behind; lists[t]: the schedule's (prone, free, redo) sizes required of step t"""
    env = _make(emu_library, task, N, **kw)
    try:
        env.reset()
        st = env.get_state().copy()
        if callable(state):
            state(st)
        else:
            st = np.array(state, np.float32)
        env.set_state(st)
        rec = {}
        for t, a in enumerate(actions):
            a = np.float32(a)
            o, r, d, info = env.step(a if a.ndim == 2 else np.tile(a, (N, 1)))
            sch = env.handle.schedule()
            if lists is not None and lists[t] is not None:
                assert tuple(sch[k].size for k in ('prone', 'free', 'redo')) == lists[t], (t, sch)
            for k in o:
                rec['%d %s' % (t, k)] = o[k]
            rec['%d reward' % t], rec['%d done' % t], rec['%d achieved' % t] = r, d, info['goal_achieved']
            for k in sch:
                rec['%d list %s' % (t, k)] = np.sort(sch[k])
        rec['state'], rec['rng'] = env.get_state(), env.handle.get_rng()
        assert np.isfinite(rec['state']).all()
        return rec
    finally:
        env.close()


def _slide_push(st):
    """the scene of test_speculative_double_repeat_is_bit_identical_to_the_serial_repeat, the puck spinning off its axis"""
    n = len(st)
    st[:, 64] = -0.52 + np.float32([0.0, 0.003, -0.002])[:n]; st[:, 65] = 0.045 + np.float32([0.0, -0.002, 0.003])[:n]; st[:, 66] = 0.170
    st[:, 67:71] = [0, 0, 0, 1]; st[:, 71:74] = 0; st[:, 74:77] = (3.0, 0.0, 5.0)


FREE_SPIN = np.float32([(6.0, 2.0, 9.0), (-5.0, 8.0, 3.0)])     # rad/s, neither along the puck's axis nor across it


def _slide_free_flight(st):
    """no contacts: the puck in the air beside the tip target (within near_r, so the env is on list 0), tumbling"""
    st[:, 18:21] = [-0.52, 0.0, 0.40]
    st[:, 64:67] = [-0.52, 0.06, 0.40]; st[:, 67:71] = [0, 0, 0, 1]; st[:, 71:74] = 0; st[:, 74:77] = FREE_SPIN[:len(st)]


def test_slide_pushing_scene_is_bit_equal_under_all_six_orders(emu_library, waves):
    """pmg_k_step_list<1, 24, 0, 1>, three wavefronts (env, float narrowphase, double repeat): the closed fingers push the puck,
    which spins about (3, 0, 5) rad/s, so the gyroscopic term -- the one reader of the puck's rotation on wavefront 0 -- is not
    zero.  Every env on list 0 in both steps."""
    N = 2
    base = _under_orders(waves, TRIPLES, lambda: _rollout(emu_library, 'slide', N, {}, _slide_push, [[0, 1, 0], [0, 1, 0]], [(N, 0, 0)] * 2))
    assert (base['state'][:, 65] > 0.06).all()                   # the puck was pushed


@pytest.fixture(scope='module')
def free_flight_oracles(built):
    """the free-flight scene in the float64 oracle and in the float32-state oracle (oracle_lib.FloorOracle), once"""
    N = 2
    out = []
    for cls in (O.OracleEnv, O.FloorOracle):
        ora = cls('slide', N, seed_base=3, seed_stride=1)
        ora.reset(), ora.reset()
        st = ora.get_state().copy()
        _slide_free_flight(st)
        ora.set_state(st)
        ora.step(np.zeros((N, 3), np.float32))
        s = ora.get_state()
        s.setflags(write=False)
        out.append(s)
    return out


def _puck_errors(s, ref):
    return np.abs(s[:, 64:71] - ref[:, 64:71]).max(), np.abs(s[:, 71:77] - ref[:, 71:77]).max()


def test_slide_free_flight_matches_the_oracle_under_all_six_orders(emu_library, waves, free_flight_oracles):
    """The same kernel on the tumbling puck in free flight, one zero-action step: no contacts, so nothing amplifies rounding and the
    puck's pose and twist are held to the float64 oracle under EVERY list, every env counted -- besides being bit-equal between the
    lists.  Bars: pose 1e-4, twist 1e-3.  They sit between ten times the spread of the float32-state oracle on this scene (pose
    1.2e-7, twist 1.9e-6, asserted below; the kernel itself: 3.6e-7 and 1.0e-6 under every list) and a tenth of what a rotation
    that is one substep stale costs (the kernel that read the helper's copy, under list 012: pose 8.6e-3, twist 6.7e-2)."""
    N = 2
    s64, s32 = free_flight_oracles
    fp, ft = _puck_errors(s32, s64)
    print('float32-state oracle against float64: pose %.3g twist %.3g' % (fp, ft))
    assert 10 * fp <= POSE_BAR and 10 * ft <= TWIST_BAR

    def check(rec, label):
        ep, et = _puck_errors(rec['state'], s64)
        print('list %s: puck pose error %.3g, twist error %.3g' % (label, ep, et))
        assert ep <= POSE_BAR and et <= TWIST_BAR, (label, ep, et)
    _under_orders(waves, TRIPLES, lambda: _rollout(emu_library, 'slide', N, {}, _slide_free_flight, [[0, 0, 0]], [(N, 0, 0)]), check)


def test_one_cube_list_is_bit_equal_under_both_orders(emu_library, waves):
    """pmg_k_step_list<1, 24, 0, 0>, two wavefronts: the palm-block scene of test_emulated_gripper_base_contact_matches_oracle"""
    N = 2

    def scene(st):
        st[:, 64] = -0.52 + np.float32([0.0, 0.002]); st[:, 65] = 0.0; st[:, 66] = 0.25 + 0.0295
    base = _under_orders(waves, PAIR, lambda: _rollout(emu_library, 'pick_and_place', N, {}, scene, [[0, 0, 0, 1], [0, 0, -1, 1]], [(N, 0, 0)] * 2))
    assert (base['state'][:, 66] > 0.25).all()                   # held up by the contacts, not in free fall


def test_multi_block_list_is_bit_equal_under_both_orders(emu_library, waves):
    """pmg_k_step_list<5, 48, 0>, two wavefronts: the stacked scene of test_emulated_stacked_blocks_behind_the_table_run_match_oracle"""
    N = 2

    def scene(st):
        st[:, 64:77] = [-0.52, 0.0, 0.175, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
        st[:, 77:90] = [-0.515, 0.004, 0.175 + 0.0305, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
        st[1, 77:79] += np.float32([-0.003, 0.002])
        st[:, 18:21] = [-0.52, 0.0, 0.26]
    acts = [[0, 0, -1, 1], [0, 0, -1, 1], [0, 0.3, -1, 1]]
    base = _under_orders(waves, PAIR, lambda: _rollout(emu_library, 'block_stack', N, {'num_block': 2}, scene, acts, [(N, 0, 0)] * 3))
    assert (base['state'][:, 79] > 0.19).all()                   # block 1 rests on block 0


@pytest.fixture(scope='module')
def chest_at_the_handle(built):
    """chest_push, two envs: the float32 oracle flies the closed fingers in over the front door, next to its handle (the approach of
    test_emulated_finger_opens_the_door_by_its_handle) -> the state the device takes over"""
    N = 2
    ora = O.OracleEnv('chest_push', N, num_block=1, seed_base=3, seed_stride=1, f32=True)
    ora.reset(), ora.reset()
    for a, n in (([0, 0, 1], 6), ([0, -1, 0], 3), ([-1, 0, 0], 7)):
        for k in range(n):
            act = np.tile(np.float32(a), (N, 1))
            act[1] *= np.float32(0.97)                           # (the second env a little behind the first)
            ora.step(act)
    st = ora.get_state().copy()
    st.setflags(write=False)
    return st


def test_chest_list_is_bit_equal_under_both_orders(emu_library, waves, chest_at_the_handle):
    """pmg_k_step_list<6, 48, 0, 2>, two wavefronts, the helper publishing the door's slot: the fingers at the door's handle push the
    door sideways (finger x handle pairs: cylinder x box, repeated in double by the helper)"""
    N = 2
    base = _under_orders(waves, PAIR, lambda: _rollout(emu_library, 'chest_push', N, {'num_block': 1}, chest_at_the_handle, [[0, 1, 0]] * 2,
                                                       [(N, 0, 0)] * 2))
    assert (base['1 achieved_goal'][:, 0] > 0.005).all()         # the door has begun to open


def test_two_wavefront_reach_kernel_is_bit_equal_under_both_orders(emu_library, waves):
    """pmg_k_step_reach2: six envs, two of them with their fingers driven onto the table (tip target at the table top: list 0, one env
    per workgroup, the helper wavefront colliding), four on the packed list (one workgroup, one wavefront of four rows and one that
    leaves at once)."""
    N = 6

    def scene(st):
        for e, y in ((1, 0.0), (4, 0.05)):
            q = O.ik(st[e, :9].astype(float), [-0.52, y, 0.172])[0]          # the fingers 3 mm inside the table top
            st[e, :7] = q[:7]; st[e, 9:18] = 0; st[e, 18:21] = [-0.52, y, 0.176]; st[e, 21:28] = q[:7]
    acts = [np.float32([[0.3, -0.2, 0.1]] * N), np.float32([[0.0, 0.5, -0.4]] * N)]
    for a in acts:
        a[[1, 4]] = [0.2, 0.1, -1.0]
    base = _under_orders(waves, PAIR, lambda: _rollout(emu_library, 'reach', N, {}, scene, acts, [(2, 4, 0)] * 2))
    assert (base['1 observation'][[1, 4], 2] > 0.17).all()       # the table keeps the fingers out


def test_sub_goal_kernel_is_bit_equal_under_both_orders(emu_library, waves):
    """pmg_k_sub_goal (256 threads, thread 31 of an env stores the level the others must not read back)"""
    N, nb = 3, 3

    def run():
        env = _make(emu_library, 'block_stack', N, num_block=nb, task_decomposition=True)
        try:
            env.reset()
            rec = {'goal %d' % k: env.set_sub_goal(k).copy() for k in (0, 2, 1)}
            rec['state'] = env.get_state()
            return rec
        finally:
            env.close()
    base = _under_orders(waves, FOUR, run)
    assert not np.array_equal(base['goal 0'], base['goal 2'])


# ----------------------------------------------------------------------------------------------------------------------
# the plan kernels: sixteen wavefronts
@pytest.mark.parametrize('nb,frac_down,two_pass', [(1, 0.4, 0), (1, 0.4, 1), (1, 0.05, 1), (0, 0.3, 1)])
def test_plan_kernels_write_the_same_lists_under_both_orders(built, waves, nb, frac_down, two_pass):
    """plan_all (one workgroup) and plan_count / plan_scatter (three workgroups, the last one ragged) on the batch of
    test_two_pass_plan_writes_the_same_lists_as_the_single_workgroup_plan (3 000 envs; reach and one free object, on either side of the
    promotion rule).  Stepping a batch large enough for the launcher to choose two passes by itself (4 096 envs) is out of the
    emulator's reach (a second per env): the plan is run by itself, and what it hands the step kernels is compared.  The lists are compared word for word, in
    order: an env's slot is its rank among the envs of its class (counts per wavefront, prefix sums across them), not the order of
    arrival at an atomic counter -- so the order of the wavefronts must not show at all."""
    lib = waves.lib
    N, adim = 3000, 3
    rs = np.random.RandomState(nb * 7 + int(frac_down * 100))
    hot = np.zeros((N, 32), np.float32)
    hot[:, 18] = rs.uniform(-0.67, -0.37, N); hot[:, 19] = rs.uniform(-0.2, 0.2, N)
    hot[:, 20] = np.where(rs.uniform(0, 1, N) < frac_down, 0.175 + rs.uniform(0, 0.01, N), rs.uniform(0.19, 0.5, N))
    blocks = np.zeros((N, 13 * max(nb, 1)), np.float32)
    blocks[:, 0] = rs.uniform(-0.64, -0.40, N); blocks[:, 1] = rs.uniform(-0.15, 0.15, N); blocks[:, 2] = 0.175; blocks[:, 6] = 1
    near = rs.uniform(0, 1, N) < 0.1
    hot[near, 18:21] = blocks[near, 0:3] + np.float32([0.0, 0.0, 0.02])
    actions = rs.uniform(-1, 1, (N, adim)).astype(np.float32)

    def run():
        sc = np.full(3 + 3 * N, -7, np.int32)
        rc = lib.pmge_probe_plan(C.c_int(N), C.c_int(nb), hot.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p),
                                 actions.ctypes.data_as(C.c_void_p), C.c_int(adim), C.c_int(1536), C.c_int(two_pass), sc.ctypes.data_as(C.c_void_p))
        assert rc in (0, 1)
        return {'sched': sc, 'promoted': np.int32(rc)}
    base = _under_orders(waves, SIXTEEN, run)['sched']
    n0, n1 = int(base[0]), int(base[1])
    assert 0 < n0 < N and n0 + n1 == N
    assert sorted(np.concatenate([base[2:2 + n0], base[2 + N:2 + N + n1]]).tolist()) == list(range(N))


# ----------------------------------------------------------------------------------------------------------------------
# the learner kernels: four wavefronts over shared LDS tiles
@contextlib.contextmanager
def _recorded():
    """everything a case downloads from the device (PmgHandle.download, norm_read) while it runs -> the list it yields"""
    log = []
    download, norm_read = PmgHandle.download, PmgHandle.norm_read

    def rec_download(self, array, d_ptr):
        download(self, array, d_ptr)
        log.append(array.copy())

    def rec_norm_read(self, which):
        r = norm_read(self, which)
        log.extend(np.array(r[k]) for k in sorted(r))
        return r
    PmgHandle.download, PmgHandle.norm_read = rec_download, rec_norm_read
    try:
        yield log
    finally:
        PmgHandle.download, PmgHandle.norm_read = download, norm_read


LEARNER_CASES = {
    # pmg_k_mlp: 3 -> 256 -> 256 -> 256 -> 4 (the deepest a pmg_mlp holds) on 101 rows = three full tiles and five rows, and five more shapes
    'actor_deep': lambda lib: AC.case_deep(lib),
    # pmg_k_td_target: actor 31 -> 256 -> 256 -> 256 -> 4 into critic 35 -> 256 -> 33 -> 1 through one tile, batches 1 .. 101
    'td_batches': lambda lib: TC.case_td_batches(lib),
    # pmg_k_norm_partial / _merge: 1 .. 4097 rows (several chunks, a ragged last one) of the three widths of push
    'norm_update': lambda lib: NC.case_update_against_float64(lib, 'push'),
    # pmg_k_policy_input: 1 .. 4097 rows, float4 body and dword tail, both layouts
    'policy_input': lambda lib: NC.case_policy_input_exact(lib, 'reach'),
    # pmg_k_her_draw / _rows and the reward kernels on the pairs they formed: 257 samples = one workgroup and one item
    'her_reward': lambda lib: HC.case_reward_is_the_reward_kernels(lib, 'push'),
}


@pytest.mark.parametrize('name', list(LEARNER_CASES))
def test_learner_kernels_are_bit_equal_under_both_orders(emu_library, waves, name):
    """One case each of tests/actor_cases.py, td_cases.py, normalizer_cases.py (two) and her_cases.py, under the default scheduler and
    the lists 0123 and 3210: the case's own assertions hold every time (they are exact: the numpy fmaf chain, numpy's float32
    arithmetic, the reward kernels' bits), and every array the case downloaded from the device is the same, byte for byte."""
    def run():
        with _recorded() as log:
            LEARNER_CASES[name](emu_library)
        assert len(log) > 2
        return {'%d' % k: np.ascontiguousarray(a).view(np.uint8) for k, a in enumerate(log)}
    _under_orders(waves, FOUR, run)
