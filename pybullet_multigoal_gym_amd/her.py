"""Hindsight-experience-replay minibatches, sampled on the device from episode rows the caller keeps.

Host-side face of ``pmg_her_sample_device`` (include/pmg.h): numpy in, numpy out.  All arithmetic happens in
the HIP library; this file validates shapes and moves buffers.  The library owns no replay store.  A device-resident learner
keeps its table in device memory and uses the pointer calls instead; recording a rollout takes three lines per step
(``HerSampler.record`` is exactly that):

    rows = h.device_alloc(4 * (T + 1) * N * P)                                 # time-major [T + 1, N, P], once
    h.device_copy(rows + 4 * t * N * P, h.device_ptr(PMG_BUF_PACKED), 4 * N * P)   # after reset (t = 0) and after step t - 1
    h.her_sample_device(rows, N, T, P, N * P, batch, ...)                      # episode stride P, time stride N * P
"""
import numpy as np

from ._lib import PMG_BUF_PACKED, PMG_NORM_OBSERVATION, PMG_NORM_POLICY_STATE

KINDS = {'observation': PMG_NORM_OBSERVATION, 'policy_state': PMG_NORM_POLICY_STATE}


class HerSampler:
    """``env.her``: draws HER minibatches from complete episodes of packed rows (the layout of PMG_BUF_PACKED)."""

    def __init__(self, env):
        self._env = env
        self._h = env.handle

    def record(self, d_rows_ptr, t, d_actions_ptr=None, d_step_actions_ptr=None):
        """Copy the packed rows of the env's last step / reset into slot ``t`` of a time-major device table
        [T + 1, N, P], and (given both pointers) the actions [N, A] of step ``t`` into slot ``t`` of [T, N, A]; on the
        handle's stream, no host sync."""
        h, d = self._h, self._h.dims
        nbytes = 4 * h.N * d.packed_dim
        h.device_copy(d_rows_ptr + t * nbytes, h.device_ptr(PMG_BUF_PACKED), nbytes)
        if d_actions_ptr is not None and d_step_actions_ptr is not None:
            h.device_copy(d_actions_ptr + t * 4 * h.N * d.action_dim, d_step_actions_ptr, 4 * h.N * d.action_dim)

    def sample(self, rows, actions, batch, future_p=0.8, seed=0, counter=0, kind='policy_state', raw=False, time_major=True):
        """rows [T + 1, E, P] and actions [T, E, A] (``time_major=False``: [E, T + 1, P] and [E, T, A]) -> dict(x, x_next
        [B, Ds + Dg], action [B, A], reward [B], goal_achieved [B] bool, index [B, 3] = e, t, f).  The draws are a pure
        function of (seed, counter, sample index)."""
        h, d = self._h, self._h.dims
        if kind not in KINDS:
            raise ValueError('kind must be one of %s, not %r' % (sorted(KINDS), kind))
        rows, actions = np.asarray(rows), np.asarray(actions)
        if rows.ndim != 3 or rows.shape[2] != d.packed_dim:
            raise ValueError('rows must have shape [T + 1, E, %d], not %s' % (d.packed_dim, rows.shape))
        T1, E = (rows.shape[0], rows.shape[1]) if time_major else (rows.shape[1], rows.shape[0])
        if T1 < 2 or E < 1:
            raise ValueError('rows %s hold no complete episode (T >= 1 steps need T + 1 rows)' % (rows.shape,))
        want = (T1 - 1, E, d.action_dim) if time_major else (E, T1 - 1, d.action_dim)
        if actions.shape != want:
            raise ValueError('actions must have shape %s, not %s' % (want, actions.shape))
        batch = int(batch)
        if batch < 0:
            raise ValueError('batch %d is negative' % batch)
        if not 0.0 <= float(future_p) <= 1.0:
            raise ValueError('future_p %r is outside [0, 1]' % (future_p,))
        rows, actions = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(actions, np.float32)
        P, A, W = d.packed_dim, d.action_dim, h.norm_width(KINDS[kind]) + d.goal_dim
        out = {'x': np.empty((batch, W), np.float32), 'x_next': np.empty((batch, W), np.float32),
               'action': np.empty((batch, A), np.float32), 'reward': np.empty(batch, np.float32),
               'goal_achieved': np.empty(batch, np.uint8), 'index': np.empty((batch, 3), np.int32)}
        ptrs = []
        try:
            for a in (rows, actions) + tuple(out.values()):
                ptrs.append(h.device_alloc(a.nbytes))
            h.upload(ptrs[0], rows)
            h.upload(ptrs[1], actions)
            es, ts = (P, E * P) if time_major else (T1 * P, P)
            aes, ats = (A, E * A) if time_major else ((T1 - 1) * A, A)
            h.her_sample_device(ptrs[0], E, T1 - 1, es, ts, batch, ptrs[1], aes, ats, state_kind=KINDS[kind], raw=raw,
                                future_p=float(future_p), seed=int(seed), counter=int(counter), d_x=ptrs[2], d_x_next=ptrs[3],
                                d_action=ptrs[4], d_reward=ptrs[5], d_goal_achieved=ptrs[6], d_index=ptrs[7])
            h.sync()
            for a, p in zip(out.values(), ptrs[2:]):
                if a.nbytes:
                    h.download(a, p)
        finally:
            for p in ptrs:
                h.device_free(p)
        out['goal_achieved'] = out['goal_achieved'].astype(np.bool_)
        return out
