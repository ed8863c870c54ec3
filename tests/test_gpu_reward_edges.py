"""The reward kernels (pmg_k_reward3, pmg_k_reward_flat, pmg_k_reward) at their edges, through the DEVICE entry point
pmg_compute_reward_device with caller-owned buffers (pmg_device_alloc / pmg_upload / pmg_download), against float64 numpy:
batch sizes around every kernel's hand-over, binary and dense rewards, a non-default threshold, NULL outputs, unaligned
pointers (which must take the generic kernel and give the same answers), canaries behind both outputs, every goal width
make_env can produce -- and pairs placed deliberately just inside and just outside the threshold.

The band around the threshold: the float32 distance sqrt(sum_g (a_g - d_g)^2) carries a relative error of at most
(G / 2 + 4) * 2^-24 -- one rounding per difference (two after squaring, one after the root), half a rounding for each
square, G roundings in the sum halved by the root, and the 2.5-ulp root of the build
(-fno-hip-fp32-correctly-rounded-divide-sqrt).  Only a pair whose float64 distance lies INSIDE that band of the threshold
may go either way; the pairs placed at thr * (1 +- 2 x band) may not."""
import ctypes as C

import numpy as np
import pytest

import pybullet_multigoal_gym_amd as pmg

pytestmark = pytest.mark.gpu

CANARY, CANARY_BYTES = 0xA5, 64


def band(G):
    return (G / 2.0 + 4.0) * 2.0 ** -24


def device_reward(env, ag, dg, want_r=True, want_ok=True, off_in=0, off_r=0, off_ok=0):
    """pmg_compute_reward_device on buffers of the caller; inputs / rewards shifted by off_in / off_r bytes (multiples of
    4), flags by off_ok bytes.  Both outputs sit in canary-filled buffers; the bytes in front of and behind them must come
    back untouched.  -> (rewards or None, flags or None)"""
    h = env.handle
    B, G = ag.shape
    ptrs = []

    def alloc(nbytes):
        p = h.device_alloc(nbytes)
        ptrs.append(p)
        return p
    try:
        d_ag, d_dg = alloc(ag.nbytes + 16), alloc(dg.nbytes + 16)
        h.upload(d_ag + off_in, np.ascontiguousarray(ag, np.float32))
        h.upload(d_dg + off_in, np.ascontiguousarray(dg, np.float32))
        r_bytes, ok_bytes = off_r + 4 * B + CANARY_BYTES, off_ok + B + CANARY_BYTES
        d_r, d_ok = alloc(r_bytes), alloc(ok_bytes)
        h.upload(d_r, np.full(r_bytes, CANARY, np.uint8))
        h.upload(d_ok, np.full(ok_bytes, CANARY, np.uint8))
        rc = h.L.lib.pmg_compute_reward_device(h.h, C.c_void_p(d_ag + off_in), C.c_void_p(d_dg + off_in), C.c_int64(B),
                                               C.c_void_p(d_r + off_r if want_r else None), C.c_void_p(d_ok + off_ok if want_ok else None))
        assert rc == 0, rc
        h.sync()
        rb, okb = np.empty(r_bytes, np.uint8), np.empty(ok_bytes, np.uint8)
        h.download(rb, d_r)
        h.download(okb, d_ok)
    finally:
        for p in ptrs:
            h.device_free(p)
    assert (rb[:off_r] == CANARY).all() and (rb[off_r + 4 * B:] == CANARY).all(), 'bytes around the rewards were written'
    assert (okb[:off_ok] == CANARY).all() and (okb[off_ok + B:] == CANARY).all(), 'bytes around the flags were written'
    if not want_r:
        assert (rb == CANARY).all(), 'd_r == NULL, yet the reward buffer was written'
    if not want_ok:
        assert (okb == CANARY).all(), 'd_ok == NULL, yet the flag buffer was written'
    r = rb[off_r:off_r + 4 * B].copy().view(np.float32) if want_r else None
    ok = okb[off_ok:off_ok + B].copy() if want_ok else None
    return r, ok


def make_pairs(B, G, thr, seed):
    """random pairs around the threshold, and -- from 16 pairs on -- every eighth pair PLACED at thr * (1 +- 2 x band),
    alternately outside and inside.  -> ag, dg, float64 distance, placed (+1 outside / -1 inside / 0 random)"""
    rs = np.random.RandomState(seed)
    ag = rs.uniform(-0.1, 0.1, (B, G)).astype(np.float32)
    dg = (ag + rs.uniform(-1, 1, (B, G)) * thr * 1.8 / np.sqrt(G)).astype(np.float32)
    placed = np.zeros(B, np.int64)
    if B >= 16:
        idx = np.arange(0, B, 8)
        placed[idx] = np.where(np.arange(len(idx)) % 2 == 0, 1, -1)
        target = thr * (1.0 + 2.0 * band(G) * placed[idx])
        u = rs.uniform(0.2, 1.0, (len(idx), G))
        x = np.float32(u / np.linalg.norm(u, axis=1)[:, None] * target[:, None]).astype(np.float64)
        rest = (x[:, 1:] ** 2).sum(1)
        x[:, 0] = np.sqrt(target ** 2 - rest)                     # the first component closes the gap the rounding left
        ag[idx] = 0.0
        dg[idx] = np.float32(x)
    d = np.linalg.norm(ag.astype(np.float64) - dg.astype(np.float64), axis=1)
    if B >= 16:
        # placed where intended: within a quarter of the band of thr * (1 +- 2 x band), so never inside the band itself
        assert (np.abs(d[idx] / target - 1.0) < 0.25 * band(G)).all()
    return ag, dg, d, placed


def check(env, B, G, thr, binary, seed, **kw):
    thr = float(np.float32(thr))                                    # the threshold as the library holds it
    ag, dg, d, placed = make_pairs(B, G, thr, seed)
    r, ok = device_reward(env, ag, dg, **kw)
    inside = np.abs(d / thr - 1.0) <= band(G)                      # the only pairs that may go either way
    assert not inside[placed != 0].any()
    clear = ~inside
    na = d > thr
    if ok is not None:
        assert set(np.unique(ok)) <= {0, 1}
        assert np.array_equal(ok[clear], (~na[clear]).astype(np.uint8)), np.nonzero(ok[clear] != ~na[clear])[0][:8]
    if r is not None:
        if binary:
            assert np.array_equal(r[clear], -(na[clear].astype(np.float32)))
            assert np.signbit(r).all()                              # -0.0 on success, -1.0 otherwise: never +0.0
            assert (r[placed == 1] == -1.0).all() and (r[placed == -1] == 0.0).all() and np.signbit(r[placed == -1]).all()
        else:
            assert (np.abs(r.astype(np.float64) + d) <= band(G) * d + 1e-45).all(), np.abs(r + d).max()
    if ok is not None:
        assert (ok[placed == 1] == 0).all() and (ok[placed == -1] == 1).all()
    return int((placed != 0).sum())


G3_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 3 - 1, 4 * 256 * 3 + 1, 262147]


@pytest.mark.parametrize('mode', ['binary', 'dense', 'binary_threshold_0.02'])
def test_reward_device_entry_point_goal_width_3(built, mode):
    """G = 3 (pmg_k_reward3 on quads of pairs + pmg_k_reward on the < 4 tail): every size around one pair, one quad, one
    workgroup of 256 quads, three workgroups, and 262 147 pairs; aligned buffers, then the inputs / rewards offset by 4 bytes
    and the flags by 1 byte (the generic kernel: same answers), then either output NULL."""
    thr = 0.02 if mode.endswith('0.02') else 0.05
    binary = mode != 'dense'
    env = pmg.make_env(task='reach', num_envs=4, binary_reward=binary, distance_threshold=thr)
    assert env.dims.goal_dim == 3
    placed = 0
    for k, B in enumerate(G3_SIZES):
        placed += check(env, B, 3, thr, binary, seed=k)
        check(env, B, 3, thr, binary, seed=100 + k, off_in=4)
        check(env, B, 3, thr, binary, seed=200 + k, off_r=4)
        check(env, B, 3, thr, binary, seed=300 + k, off_ok=1)
        check(env, B, 3, thr, binary, seed=400 + k, want_r=False)
        check(env, B, 3, thr, binary, seed=500 + k, want_ok=False)
    assert placed > 30000
    env.close()


# every goal width make_env can produce beyond 3: 3 nb (+ 4 with the gripper tail) for the block tasks, 1 + 3 nb (+ 3 / + 4)
# for the chest tasks
WIDTHS = [(4, 'chest_push', dict(num_block=1)), (6, 'block_stack', dict(num_block=2)), (7, 'block_stack', dict(num_block=1, grip_informed_goal=True)),
          (8, 'chest_pick_and_place', dict(num_block=1, grip_informed_goal=True)), (9, 'block_stack', dict(num_block=3)),
          (10, 'chest_push', dict(num_block=2, grip_informed_goal=True)), (11, 'chest_pick_and_place', dict(num_block=2, grip_informed_goal=True)),
          (12, 'block_stack', dict(num_block=4)), (13, 'chest_push', dict(num_block=4)), (14, 'chest_pick_and_place', dict(num_block=3, grip_informed_goal=True)),
          (15, 'block_rearrange', dict(num_block=5)), (16, 'chest_push', dict(num_block=5)), (17, 'chest_pick_and_place', dict(num_block=4, grip_informed_goal=True)),
          (19, 'block_stack', dict(num_block=5, grip_informed_goal=True)), (20, 'chest_pick_and_place', dict(num_block=5, grip_informed_goal=True))]


@pytest.mark.parametrize('G,task,kw', WIDTHS, ids=['G%d' % w[0] for w in WIDTHS])
def test_reward_device_entry_point_multi_block_goal_widths(built, G, task, kw):
    """pmg_k_reward_flat on the full workgroups of 256 pairs + pmg_k_reward on the tail, at every goal width, binary and
    dense, around one and two workgroups and at 70 001 pairs; with the inputs offset by 4 bytes the whole batch takes the
    generic kernel and must answer the same."""
    import warnings
    for binary in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            env = pmg.make_env(task=task, num_envs=1, binary_reward=binary, **kw)
        assert env.dims.goal_dim == G
        for k, B in enumerate((255, 256, 257, 511, 70001)):
            check(env, B, G, 0.05, binary, seed=10 * G + k)
            check(env, B, G, 0.05, binary, seed=10 * G + k, off_in=4)
        env.close()
