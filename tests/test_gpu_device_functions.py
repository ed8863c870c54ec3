"""The device functions under the step kernels -- fk, tip_frame, body_inertia, mass_inverse, bias_torque, ik_solve, the
box / cylinder narrowphase, fk64_link, cyl_redo64 -- called DIRECTLY on a real gfx950, as hipcc compiles them with the
product's flags (contracted multiply-adds, v_rcp / v_sqrt, 2.5-ulp division, LDS operands, one pair per lane with the lanes
diverging), against the float64 oracle: the cases, checks and bars of the emulated tier (tests/device_cases.py,
tests/test_emulated_kernels.py), which sees the same functions as g++ code on one host thread.  A failure names the
function; the rollout tests (tests/test_gpu_parity.py) can only say "somewhere"."""
import ctypes as C
import os

import numpy as np
import pytest

import device_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


class GpuRunners:
    """the runners of tests/device_cases.py on the device probe library: all cases of a call in one or a few launches"""

    def __init__(self, packed=False, lanes=64):
        self.lib = C.CDLL(os.path.join(ROOT, 'gpu_probe', 'libpmg_gpu_probe.so'))
        self.packed, self.lanes = int(packed), lanes

    def dynamics(self, q, qd, tau):
        n = len(q)
        qdd, mi, tip = np.zeros((n, 9), np.float32), np.zeros((n, 81), np.float32), np.zeros((n, 12), np.float32)
        rc = self.lib.pmgd_dynamics(self.packed, n, _fp(_f32(q)), _fp(_f32(qd)), _fp(_f32(tau)), _fp(qdd), _fp(mi), _fp(tip))
        assert rc == 0, rc
        return qdd, mi, tip

    def ik(self, q, target):
        out = np.zeros((len(q), 9), np.float32)
        rc = self.lib.pmgd_ik(self.packed, len(q), _fp(_f32(q)), _fp(_f32(target)), _fp(out))
        assert rc == 0, rc
        return out

    def narrowphase(self, kind, pairs, lanes=None):
        pairs = _f32(pairs)
        n, out, amb = np.zeros(len(pairs), np.int32), np.zeros((len(pairs), 40), np.float32), np.zeros(len(pairs), np.float32)
        rc = self.lib.pmgd_narrowphase(kind, len(pairs), lanes or self.lanes, _fp(pairs), C.c_float(0.002), _fp(out), _fp(n), _fp(amb))
        assert rc == 0, rc
        return n, out, amb

    def fk64(self, q9, body):
        p, R = np.zeros((len(q9), 3)), np.zeros((len(q9), 9))
        rc = self.lib.pmgd_fk64(len(q9), _fp(_f32(q9)), _fp(np.ascontiguousarray(body, np.int32)), _fp(p), _fp(R))
        assert rc == 0, rc
        return p, R

    def cyl_redo64(self, blks, kc, ck=-1):
        n, out = np.zeros(len(blks), np.int32), np.zeros((len(blks), 40), np.float32)
        q9, door = np.zeros((len(blks), 9), np.float32), np.zeros(len(blks), np.float32)
        rc = self.lib.pmgd_cyl_redo64(len(blks), ck, _fp(q9), _fp(_f32(blks)), _fp(door), _fp(_f32(kc)), C.c_float(0.03), C.c_float(0.01), _fp(out), _fp(n))
        assert rc == 0, rc
        return n, out

    def redo_pairs(self, ck, ids, q9, blk, doorq, kc, lanes=None):
        n, out = np.zeros(len(ids), np.int32), np.zeros((len(ids), 40), np.float32)
        rc = self.lib.pmgd_cyl_redo64_pairs(len(ids), int(ck), lanes or self.lanes, _fp(np.ascontiguousarray(ids, np.int32)), _fp(_f32(q9)), _fp(_f32(blk)),
                                            _fp(_f32(doorq)), _fp(_f32(kc)), C.c_float(D.PUCK_R), C.c_float(D.PUCK_HL), _fp(out), _fp(n))
        assert rc == 0, rc
        return n, out

    def double_maths(self, op, x, y):
        x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
        o0, o1 = np.zeros(len(x)), np.zeros(len(x))
        rc = self.lib.pmgd_double_maths(op, len(x), _fp(x), _fp(y), _fp(o0), _fp(o1))
        assert rc == 0, rc
        return o0, o1


@pytest.fixture(scope='module')
def gpu_run(built):
    return GpuRunners()


@pytest.fixture(scope='module')
def gpu_run_packed(built):
    return GpuRunners(packed=True)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['one_env_per_wave', 'four_envs_per_wave'])
def test_gpu_dynamics_functions_match_oracle(gpu_run, gpu_run_packed, layout):
    """fk / tip_frame / body_inertia / mass_inverse / bias_torque as in pmge_probe_dynamics, in one wavefront (pmg::) and in all
    four rows of a wavefront at once with four different inputs (pmgp::, the packed reach layout).

    The emulated tier's three poses around the start pose: its bars as they are (2e-5 qdd, 1e-5 minv, 1e-6 tip).

    The wide set (those, 256 poses across the joint ranges, the start pose, 18 poses at the joint limits; 279 in all): the
    tip bars as they are; on qdd and minv the device measures 2.90e-5 and 2.35e-5 (both layouts alike) and misses the emulated
    bars -- as the g++ build does on the same poses (3.82e-5, 2.73e-5): far from the start pose the mass matrix is worse
    conditioned than the 1e3 those bars were set for.  The oracle's own float32 mode (every operation correctly rounded)
    strays 3.08e-5 and 3.94e-5 from its float64 mode on these inputs, so the bars in force are max(emulated bar, 4 x that
    spread) = 1.23e-4 and 1.58e-4, computed here from the two oracle modes, never from the device (the factor 4: 1-ulp rcp /
    sqrt, 2.5-ulp division and contracted multiply-adds against 0.5 ulp per operation)."""
    run = gpu_run if layout == 'one_env_per_wave' else gpu_run_packed
    D.check_dynamics(D.dynamics_cases_basic(), run.dynamics)
    cases = D.dynamics_cases_wide()
    assert len(cases) >= 256 + 3 + 2 + 18
    err = D.dynamics_errors(cases, run.dynamics).max(0)
    spread = D.dynamics_errors(cases, None, f32=True).max(0)
    bars = (max(D.DYN_BARS[0], 4 * spread[0]), max(D.DYN_BARS[1], 4 * spread[1]), D.DYN_BARS[2], D.DYN_BARS[3])
    print('%s, %d cases (qdd, minv, tip position, tip rotation): device max %s, float32-oracle spread %s, bars %s' % (layout, len(cases), err, spread, bars))
    D.check_dynamics(cases, run.dynamics, bars=bars)


@pytest.mark.parametrize('layout', ['one_env_per_wave', 'four_envs_per_wave'])
def test_gpu_ik_matches_oracle(gpu_run, gpu_run_packed, layout):
    """ik_solve as in pmge_probe_ik, both layouts (four different targets per wavefront in the packed one, iteration counts
    diverging by row): the emulated tier's two targets, 256 targets in the workspace box from four start poses, its eight
    corners, targets beyond each of its faces and out of the arm's reach; 274 in all.  The emulated tier's bar, 5e-5, as it
    is: the device measures 2.7e-7 (the float32 oracle strays 4.5e-4 on the out-of-reach targets; not needed)."""
    run = gpu_run if layout == 'one_env_per_wave' else gpu_run_packed
    cases = D.ik_cases_wide()
    err = D.ik_errors(cases, run.ik)
    print('%s: device max vs float64 oracle: ik %.3g (%d cases, worst %d)' % (layout, err.max(), len(cases), int(err.argmax())))
    D.check_ik(cases, run.ik)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['box', 'cyl'])
def test_gpu_narrowphase_matches_oracle_on_random_pairs(gpu_run, kind):
    """box_box_fast / cyl_box, one pair per lane, 64 lanes per launch (aligned, tilted and randomly oriented pairs next to
    each other: the lanes diverge), on the random pairs at first touch of the emulated tier: its bars, its caps."""
    worst = D.check_random_pairs(kind, gpu_run.narrowphase)
    print('%s: largest errors of the strictly checked pairs (normal, depth, points): %s' % (kind, worst))


def test_gpu_cyl_box_corner_in_the_side_matches_oracle(gpu_run):
    D.check_corner_in_side(gpu_run.narrowphase)


def test_gpu_cubes_stacked_flush_give_the_oracles_contacts(gpu_run):
    """vertices of the incident face exactly ON the clip planes of the reference face (cubes stacked off-centre with flush
    sides, a cube in the table's corner, a finger flush with a cube): four points, the oracle's, from box_box_fast (its
    box_face_clip passes) and from the general box_box alike"""
    assert D.check_flush_stacks(gpu_run.narrowphase, D.NP_FAST) > 40
    D.check_flush_stacks(gpu_run.narrowphase, D.NP_GENERAL)


def test_gpu_axis_aligned_partner_front_end_agrees_with_the_general_routine(gpu_run):
    """box_box_fast<true, true> (B known to be axis-aligned: sums with exact zeros left out) against the general box_box.  As
    g++ code the two are bit-identical (test_axis_aligned_partner_front_end_is_bit_identical, emulated tier); hipcc contracts
    the multiply-adds of the two instantiations differently, so on the gfx950 build the last bits of some contacts differ
    (measured: 41 of the 463 pairs in contact, by at most 3.0e-8 in depth and in a point; normals equal).  No guarantee of the product rests on the identity: every kernel calls ONE instantiation
    (box_box_fast<true, NB == 0>, collide()) for all its pairs, whatever the batch, the shard or the number of wavefronts;
    box_box alone is not called by any kernel.  What holds, and is asserted: identical contact counts on all 600 pairs, and
    agreement within the strict narrowphase bars (2e-4 normal, 2e-5 depth, 5e-5 points)."""
    n, bits, worst = D.check_two_routines_agree(D.axis_aligned_cases(), gpu_run.narrowphase, D.NP_FAST_ALIGNED, D.NP_GENERAL)
    assert int((n > 0).sum()) > 250


def test_gpu_face_clip_agrees_with_the_general_box_box_routine(gpu_run):
    """box_box_fast (box_face_clip for partial face overlaps) against the general box_box on the gfx950 build: identical
    contact counts on all 900 pairs, same point order, agreement within the strict narrowphase bars; bit-identical as g++
    code (emulated tier), not as hipcc code (measured: 120 of the 791 pairs in contact differ in
    their last bits, by at most 3.0e-8 in depth and 6.0e-8 in a point; normals equal) -- see the test above."""
    n, bits, worst = D.check_two_routines_agree(D.face_clip_cases(), gpu_run.narrowphase, D.NP_FAST, D.NP_GENERAL)
    assert int((n > 0).sum()) > 300 and int((n == 4).sum()) > 100


def _far_apart(n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([D.pack_pair(rs.uniform(-0.1, 0.1, 3) + [0.5, 0, 0], np.eye(3).ravel(), [0.015] * 3, rs.uniform(-0.1, 0.1, 3), np.eye(3).ravel(), [0.015] * 3)
                     for _ in range(n)])


@pytest.mark.parametrize('kind', [D.NP_FAST, D.NP_FAST_ALIGNED, D.NP_GENERAL, D.NP_CYL], ids=['box_box_fast', 'box_box_fast_aligned', 'box_box', 'cyl_box'])
def test_gpu_narrowphase_lanes_reproduce_what_each_pair_gives_alone(gpu_run, kind):
    """pairs of every outcome shuffled together -- face contacts without clipping, clipped faces, edge x edge, no contact --
    so that the lanes of a launch diverge through the clip passes: with 64, 37 and 16 lanes per launch every pair gives, bit
    for bit, what it gives in a launch of its own (count, points, normals, depths, and cyl_box's ambiguity measure)."""
    rs = np.random.RandomState(17)
    if kind == D.NP_CYL:
        pool = [p for _, p in D.random_pairs_at_first_touch('cyl')] + [c[2] for c in D.corner_in_side_cases()]
        far = _far_apart(40, 1)
        far[:, 12:15] = [0.03, 0.03, 0.01]
        pool += list(far)
    else:
        pool = [p for _, p in D.random_pairs_at_first_touch('box')] + list(D.face_clip_cases()[::3]) + list(D.axis_aligned_cases()[::3]) + list(_far_apart(40, 2))
    pairs = np.stack(pool)[rs.permutation(len(pool))]
    alone = gpu_run.narrowphase(kind, pairs, lanes=1)
    counts = np.bincount(alone[0], minlength=5)
    print('outcomes in the mix (0..4 points): %s' % counts)
    assert counts[0] > 30 and counts[1:].sum() > 100 and (counts[1:] > 0).sum() >= 2
    for lanes in (64, 37, 16):
        n, out, amb = gpu_run.narrowphase(kind, pairs, lanes=lanes)
        assert np.array_equal(n, alone[0]), (lanes, np.nonzero(n != alone[0])[0][:8])
        for t in range(len(pairs)):
            k = 10 * int(n[t])
            assert np.array_equal(out[t][:k].view(np.uint32), alone[1][t][:k].view(np.uint32)), (lanes, t)
        assert np.array_equal(amb.view(np.uint32), alone[2].view(np.uint32)), lanes


# ----------------------------------------------------------------------------------------------------------------------
def test_gpu_double_forward_kinematics_of_the_contact_links_matches_the_oracle(gpu_run):
    D.check_fk64(gpu_run.fk64)


def test_gpu_double_repeat_of_a_cylinder_pair_is_the_float64_oracle(gpu_run):
    """cyl_redo64<-1> on the gfx950 build, one case per lane, and the float pass beside it with its ambiguity flag"""
    D.check_cyl_redo64(gpu_run.cyl_redo64, gpu_run.narrowphase)


@pytest.mark.parametrize('ck', [0, 1])
def test_gpu_double_repeat_with_a_chest_in_the_scene_gives_the_same_table_contacts(gpu_run, ck):
    """cyl_redo64<0> / <1> (the chest tasks' instantiations) on the puck x table pair: the chest's boxes are not part of the
    pair, so the answer is that of cyl_redo64<-1>, bit for bit"""
    blks, kc = D.cyl_redo64_cases()
    n0, o0 = gpu_run.cyl_redo64(blks, kc)
    n1, o1 = gpu_run.cyl_redo64(blks, kc, ck=ck)
    assert np.array_equal(n0, n1) and np.array_equal(o0.view(np.uint32), o1.view(np.uint32))
    assert int((n0 > 0).sum()) > 150


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ck', [-1, 0, 1])
def test_gpu_double_repeat_matches_the_oracle_on_every_pair_it_serves(gpu_run, ck):
    """cyl_redo64<ck> on the gfx950 build on all six kinds of pair collide() hands it (the cases and bars of the emulated tier:
    the oracle's count, 1e-6 normals and points, 1e-8 depths), one case per lane, the 64 lanes of a launch carrying different
    kinds of pair in the order the generator made them.  Then the robot body's pose handed in as spec_fk / spec_pairs do: the same
    bars, and the bits of the fetch-inside mode."""
    D.check_redo_pairs(ck, gpu_run.redo_pairs, handed_bits=True)


@pytest.mark.parametrize('ck', [-1, 0, 1])
def test_gpu_double_repeat_lanes_reproduce_what_each_pair_gives_alone(gpu_run, ck):
    """200 cases of every row of one chest kind shuffled together (>= 100 in contact, >= 30 out of contact; fetched and handed-in
    poses alternating), so that neighbouring lanes enter the out-of-line cyl_redo64 with different ids: with 64, 37 and 16 lanes
    per launch every case gives, bit for bit, what it gives in a launch of its own"""
    assert D.check_redo_lanes(ck, gpu_run.redo_pairs) >= 130


def test_gpu_float_pass_matches_the_oracle_on_the_shapes_of_every_cylinder_pair(gpu_run):
    """cyl_box<float> on the gfx950 build on the gripper base, both handles and the puck against the cube, door, lid, wall and
    finger boxes (the cases, bars and the 1 % cap of the emulated tier), 64 pairs per launch"""
    D.check_float_shapes(gpu_run.narrowphase)


def test_gpu_double_sine_and_cosine_hold_their_error_on_every_joint_angle(gpu_run):
    """sincos64 as hipcc compiles it against numpy: absolute error < 1e-15 on every float32 joint angle the cases here use (limits,
    quadrant switch points, multiples of pi / 2, one float32 step to either side) and 4096 random angles in [-3.06, 3.06], the
    range the routine is written for"""
    D.check_sincos64(gpu_run.double_maths)


def test_gpu_double_square_root_and_division_hold_their_stated_error(gpu_run):
    """t_sqrt(double) / t_div(double, double) on gfx950 -- v_rsq_f64 / v_rcp_f64 and two Newton steps, code the g++ build never
    sees -- against numpy float64: relative error < 1e-15, the figure the source states, on squared lengths 1e-40 .. 1e4 (and an
    exact 0, which must give 0) and divisors of both signs 1e-20 .. 1e4, log-spaced, random, exact squares and powers of two.
    Values outside these ranges are not what the routines are for"""
    D.check_sqrt_div64(gpu_run.double_maths)
