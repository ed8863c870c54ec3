"""Running normaliser and policy-input rows of goal-conditioned learners (HER + DDPG / SAC), on the device.

Host-side face of ``pmg_norm_*`` / ``pmg_policy_input*`` (include/pmg.h): numpy in, numpy out.  All
arithmetic happens in the HIP library; this file validates shapes and moves buffers.  A device-resident loop uses the raw
pointer calls of ``PmgHandle`` instead.
"""
import numpy as np

from ._lib import PMG_NORM_GOAL, PMG_NORM_OBSERVATION, PMG_NORM_POLICY_STATE

KINDS = {'observation': PMG_NORM_OBSERVATION, 'policy_state': PMG_NORM_POLICY_STATE, 'goal': PMG_NORM_GOAL}


class Normalizer:
    """``env.normalizer``: three independent running normalisers (observation, policy_state, goal) of one KukaVecEnv."""

    def __init__(self, env):
        self._env = env
        self._h = env.handle
        self.eps, self.clip_input, self.clip_output = 0.01, 200.0, 5.0

    def _kind(self, kind, state_only=False):
        if kind not in KINDS or (state_only and kind == 'goal'):
            raise ValueError('kind must be one of %s, not %r' % (sorted(k for k in KINDS if not (state_only and k == 'goal')), kind))
        return KINDS[kind]

    def _rows(self, a, which):
        """[B, D] float32 rows of an array shaped [..., D] ([D] alone is one row)."""
        D = self._h.norm_width(which)
        a = np.asarray(a)
        if a.ndim == 0 or a.shape[-1] != D:
            raise ValueError('expected an array ending in %d columns, got shape %s' % (D, a.shape))
        return np.ascontiguousarray(a, np.float32).reshape(-1, D)

    def configure(self, eps=0.01, clip_input=200.0, clip_output=5.0):
        """Floor of the standard deviation and the two clips; re-derives mean / std, keeps the totals."""
        self._h.norm_configure(float(eps), float(clip_input), float(clip_output))
        self.eps, self.clip_input, self.clip_output = float(eps), float(clip_input), float(clip_output)

    def update(self, observation=None, policy_state=None, goal=None, mask=None):
        """Add rows to the running statistics; ``mask`` ([B] bool) selects rows and applies to every array given."""
        given = [(KINDS[k], self._rows(v, KINDS[k])) for k, v in
                 (('observation', observation), ('policy_state', policy_state), ('goal', goal)) if v is not None]
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(-1)
        for which, rows in given:
            if m is not None and m.shape[0] != rows.shape[0]:
                raise ValueError('mask has %d entries for %d rows' % (m.shape[0], rows.shape[0]))
            self._h.norm_update(which, rows, m)

    def update_from_env(self, mask=None):
        """Add the observation, policy_state and desired_goal of the env's last step / reset, read in place on the device."""
        h = self._h
        if mask is None:
            h.norm_update_env_device(None)
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(h.N)
        d_mask = h.device_alloc(h.N)
        try:
            h.upload(d_mask, m)
            h.norm_update_env_device(d_mask)
        finally:
            h.device_free(d_mask)   # waits for the handle's stream first

    def update_ranks(self, observation=None, policy_state=None, goal=None, mask=None):
        """``update`` as a collective of a data-parallel learner: every rank passes ITS rows -- the same number on every rank,
        rank r's rows being rows r * B_local ... of the global batch -- and every rank ends with the totals of ONE ``update`` on the
        concatenated rows, bit for bit.  With more than one rank B_local must be a multiple of the chunk of the global batch,
        64 * ceil(R * B_local / 65 408).  Every rank must make the same calls; needs ``comm_init`` and no ``comm_overlap``."""
        h = self._h
        given = [(KINDS[k], self._rows(v, KINDS[k])) for k, v in
                 (('observation', observation), ('policy_state', policy_state), ('goal', goal)) if v is not None]
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(-1)
        for which, rows in given:
            if m is not None and m.shape[0] != rows.shape[0]:
                raise ValueError('mask has %d entries for %d rows' % (m.shape[0], rows.shape[0]))
            ptrs = []
            try:
                ptrs.append(h.device_alloc(max(rows.nbytes, 4)))
                h.upload(ptrs[0], rows)
                if m is not None:
                    ptrs.append(h.device_alloc(max(m.nbytes, 4)))
                    h.upload(ptrs[1], m)
                h.norm_update_ranks_device(which, ptrs[0], rows.shape[1], rows.shape[0], ptrs[1] if m is not None else None)
                h.sync()
            finally:
                for p in ptrs:
                    h.device_free(p)

    def update_from_env_ranks(self, mask=None):
        """``update_from_env`` as a collective: the rows of every rank's envs, the totals of one unsharded env of all of them on every rank.
        The ranks' envs must be the global envs in rank order (``distributed.check_data_parallel``)."""
        h = self._h
        if mask is None:
            h.norm_update_env_ranks_device(None)
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(h.N)
        d_mask = h.device_alloc(h.N)
        try:
            h.upload(d_mask, m)
            h.norm_update_env_ranks_device(d_mask)
        finally:
            h.device_free(d_mask)   # waits for the handle's stream first

    def policy_input(self, state, goal, kind='policy_state'):
        """[..., Ds + Dg] float32: clip((clip(v) - mean) * inv_std) of ``state`` (of ``kind``) and ``goal``, side by side."""
        which = self._kind(kind, state_only=True)
        s, g = np.asarray(state), np.asarray(goal)
        if s.shape[:-1] != g.shape[:-1]:
            raise ValueError('state %s and goal %s must share their leading axes' % (s.shape, g.shape))
        out = self._h.policy_input(which, self._rows(s, which), self._rows(g, PMG_NORM_GOAL))
        return out.reshape(s.shape[:-1] + (out.shape[-1],))

    def policy_input_from_env(self, kind='policy_state'):
        """The same for every env's last step / reset, from the device-resident rows: [N, Ds + Dg] ([Ds + Dg] with
        num_envs=None)."""
        which = self._kind(kind, state_only=True)
        h = self._h
        W = h.norm_width(which) + h.dims.goal_dim
        out = np.empty((h.N, W), np.float32)
        d_out = h.device_alloc(out.nbytes)
        try:
            h.policy_input_env_device(which, d_out)
            h.download(out, d_out)
        finally:
            h.device_free(d_out)
        return out if self._env.batched else out[0]

    def mean(self, kind):
        return self._h.norm_read(self._kind(kind))['mean']

    def std(self, kind):
        return self._h.norm_read(self._kind(kind))['std']

    def count(self, kind):
        return self._h.norm_read(self._kind(kind))['count']

    def state_dict(self):
        """Totals and settings, enough for load_state_dict() on a fresh env to give bit-identical policy inputs."""
        out = {'eps': self.eps, 'clip_input': self.clip_input, 'clip_output': self.clip_output}
        for name, which in KINDS.items():
            r = self._h.norm_read(which)
            out[name] = {'sum': r['sum'], 'sumsq': r['sumsq'], 'count': r['count']}
        return out

    def load_state_dict(self, sd):
        self.configure(sd['eps'], sd['clip_input'], sd['clip_output'])
        for name, which in KINDS.items():
            self._h.norm_write(which, sd[name]['sum'], sd[name]['sumsq'], float(sd[name]['count']))
