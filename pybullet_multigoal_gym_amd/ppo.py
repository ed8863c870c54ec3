"""Proximal policy optimisation (PPO) on whole rollouts, on the device: generalised advantage estimation, the advantage normaliser, the
clipped-surrogate gradient of a Gaussian actor and the statistics of a minibatch.

Host-side face of ``pmg_gae_device``, ``pmg_adv_stats_device`` / ``pmg_adv_apply_device``, ``pmg_ppo_policy_grad_device`` and
``pmg_ppo_stats_device`` (include/pmg.h).  All arithmetic happens in the HIP library; this file validates shapes and moves
buffers.  The policy is ``env.gaussian_actor`` (sac.GaussianActor: an MLP with 2 A identity outputs, means | log-stds), the value function any
``Critic``-like network with one output evaluated by ``pmg_mlp_forward_device``; Adam and the data-parallel merge are ``optim.Trainable``'s.

One PPO iteration on N envs and T steps (``pi`` the loaded actor, ``vf`` the value network, ``ppo = env.ppo``; every call is stream-ordered on
the handle's stream, nothing is computed on the host and nothing waits):

    for t in range(T):                                          # the rollout: no new acting kernel
        pi.act_device(d_act, seed=s, counter=c + t, d_noise=d_n + t * N * A * 4, d_preact=d_zo + t * N * 2 * A * 4)    # sample, keep n and z
        h.device_copy(d_rows + t * N * P * 4, h.device_ptr(), N * P * 4)       # the packed rows the action was drawn from: s_t
        h.step_device(d_act)
        h.device_copy(d_succ + t * N * P * 4, h.device_ptr(), N * P * 4)       # the rows step t led to, BEFORE the reset: reward, done, s'_t
        h.reset_done_device()
    h.policy_input_device(kind, d_rows + so, P, d_rows + dgo, P, T * N, d_x)   # x  [T, N, Dx]: normalised rows of s_t
    h.policy_input_device(kind, d_succ + so, P, d_succ + dgo, P, T * N, d_xs)  # x' [T, N, Dx]: of the successors
    h.mlp_forward_device(vf_mlp, d_x, Dx, T * N, d_v, 1); h.mlp_forward_device(vf_mlp, d_xs, Dx, T * N, d_vs, 1)       # V [T, N] and V' [T, N]
    ppo.gae_device(T, N, (d_succ + 4 * reward_col, N * P, P), (d_v, N, 1), (d_vs, N, 1), (d_adv, N, 1), gamma, lam,
                   cut=(d_succ + 4 * done_col, N * P, P), ret=(d_ret, N, 1))   # reward and done read in place from the recorded rows
    ppo.normalize_advantages_device(d_adv, T * N, d_stats)
    for epoch in range(K):
        for lo in range(0, T * N, B):                           # minibatches: contiguous slices of the flattened rollout
            ppo.policy_grad_device(pi, B, d_x + lo * Dx * 4, d_zo + lo * 2 * A * 4, d_n + lo * A * 4, d_adv + lo * 4, d_work, work, clip=0.2,
                                   ent_coef=0.0, grads=sa.g, d_ratio=d_rho, d_logratio=d_lr, d_clipped=d_cl, chunk_rows=R)
            pi.adam_step_device(sa.g, sa, lr)
            vf.grad_device(B, d_x + lo * Dx * 4, Dx, d_vwork, vwork, d_target=d_ret + lo * 4, gscale=vf_coef / B, grads=sv.g, chunk_rows=R)
            vf.adam_step_device(sv.g, sv, lr)                   # gscale * (V - ret): the gradient of vf_coef / (2 B) sum (V - ret)^2
            ppo.stats_device(B, d_rho, d_lr, d_cl, d_adv + lo * 4, d_st)      # approximate KL, clip fraction, surrogate, mean log-ratio

Why ``value_next`` is a table of its own.  Every episode of this library ends by TimeLimit, so the packed row's ``done`` is a truncation: GAE
bootstraps from the value of the finished episode's LAST observation and only restarts its chain there (``cut``).  After ``reset_done_device``
the env's current row is the new episode's first state, so a ``[T + 1, N]`` value table of the rows acted on, shifted by one step, bootstraps a
finished episode from the wrong state.  The recipe above records the successor rows before the reset and evaluates them separately.  (Only when
no env is reset inside the rollout -- T = max_episode_steps, started from a reset -- may one table of T + 1 recorded rows serve both, with
``value_next = (d_v + 4 * N, N, 1)``.)
``terminal`` (no bootstrap at all) is for learners that treat reaching the goal as an absorbing state; it is independent of ``cut``.

The loss.  ``policy_grad_device`` forms the gradient of

    pscale * sum_b min(rho_b adv_b, clip(rho_b, 1 - clip, 1 + clip) adv_b) + escale * sum_b sum_j ls_bj,   pscale = -1 / B, escale = -ent_coef / B

where rho = pi_new(u | x) / pi_old(u | x) at the recorded pre-squash sample u = zo_mu + exp(clamp(zo_ls)) n (the tanh correction cancels in
the ratio).  The entropy bonus is that of the pre-squash Gaussian (sum of the log-stds inside the clamp), not of the squashed policy.
"""
import numpy as np

from .optim import ParamBuffers
from .sac import LS_HI, LS_LO, GaussianActor, _clamp


def _table(tab, name, optional=False):
    if tab is None:
        if optional:
            return None
        raise ValueError('%s must be (device pointer, time_stride, env_stride)' % name)
    if len(tab) != 3 or tab[0] is None:
        raise ValueError('%s must be (device pointer, time_stride, env_stride), not %r' % (name, tab))
    return int(tab[0]), int(tab[1]), int(tab[2])


def _clip(clip):
    """clip (eps, or the pair (clip_lo, clip_hi)) -> clip_lo, clip_hi as the floats the device compares with"""
    if isinstance(clip, (tuple, list)):
        lo, hi = float(clip[0]), float(clip[1])
    else:
        eps = float(clip)
        lo, hi = float(np.float32(1.0) - np.float32(eps)), float(np.float32(1.0) + np.float32(eps))
    if not (0.0 <= lo <= hi):
        raise ValueError('the clip range %r / %r must be ordered and >= 0' % (lo, hi))
    return lo, hi


class Ppo:
    """``env.ppo``: the PPO calls of the env's device."""

    def __init__(self, env):
        self._env = env
        self._h = env.handle

    # -- generalised advantage estimation --
    def gae_device(self, steps, envs, reward, value, value_next, adv, gamma, lam, cut=None, terminal=None, ret=None):
        """Advantages (and returns) of ``steps`` x ``envs`` transitions in device memory.  Every table is ``(device pointer, time_stride,
        env_stride)`` with the strides in floats: a time-major [T, N] table is ``(p, N, 1)``, a column of recorded packed rows
        ``(p + 4 * column, N * packed_dim, packed_dim)``.  ``value_next``: V of the state each step led to, before any reset.  ``cut``
        (non-zero: an episode ends behind the step; the packed row's ``done``) and ``terminal`` (non-zero: no bootstrap) are optional float
        tables, ``ret`` an optional output.  On the handle's stream, no host sync."""
        steps, envs, gamma, lam = int(steps), int(envs), float(gamma), float(lam)
        if steps < 0 or envs < 0 or steps * envs >= 2 ** 31:
            raise ValueError('steps %r and envs %r must be >= 0 with steps * envs < 2^31' % (steps, envs))
        if not (0.0 <= gamma <= 1.0 and 0.0 <= lam <= 1.0):
            raise ValueError('gamma %r and lam %r must lie in [0, 1]' % (gamma, lam))
        h = self._h
        g = h.gae_struct(steps, envs, gamma, lam, _table(reward, 'reward'), _table(value, 'value'), _table(value_next, 'value_next'), _table(adv, 'adv'),
                         _table(cut, 'cut', True), _table(terminal, 'terminal', True), _table(ret, 'ret', True))
        h.gae_device(g)

    def gae(self, reward, value, value_next, gamma, lam, cut=None, terminal=None):
        """reward, value, value_next [T, N] (cut, terminal [T, N] or None; non-zero is true) -> adv, ret [T, N], numpy."""
        reward = np.ascontiguousarray(reward, np.float32)
        if reward.ndim != 2:
            raise ValueError('reward %s must be [T, N]' % (reward.shape,))
        T, N = reward.shape
        tabs = {'reward': reward}
        for name, arr in (('value', value), ('value_next', value_next), ('cut', cut), ('terminal', terminal)):
            if arr is None:
                if name in ('value', 'value_next'):
                    raise ValueError('%s is required' % name)
                continue
            arr = np.ascontiguousarray(arr, np.float32)
            if arr.shape != (T, N):
                raise ValueError('%s %s must be [%d, %d]' % (name, arr.shape, T, N))
            tabs[name] = arr
        adv, ret = np.empty((T, N), np.float32), np.empty((T, N), np.float32)
        if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(lam) <= 1.0):
            raise ValueError('gamma %r and lam %r must lie in [0, 1]' % (gamma, lam))
        if T == 0 or N == 0:
            return adv, ret
        h, ptrs = self._h, []
        try:
            d = {}
            for name, arr in tabs.items():
                ptrs.append(h.device_alloc(arr.nbytes))
                h.upload(ptrs[-1], arr)
                d[name] = (ptrs[-1], N, 1)
            for name in ('adv', 'ret'):
                ptrs.append(h.device_alloc(adv.nbytes))
                d[name] = (ptrs[-1], N, 1)
            self.gae_device(T, N, d['reward'], d['value'], d['value_next'], d['adv'], gamma, lam, d.get('cut'), d.get('terminal'), d['ret'])
            h.sync()
            h.download(adv, d['adv'][0])
            h.download(ret, d['ret'][0])
        finally:
            for p in ptrs:
                h.device_free(p)
        return adv, ret

    # -- the advantage normaliser --
    def adv_stats_device(self, d_x, count, d_stats, eps=1e-8, ddof=0):
        """d_stats [2] = mean | 1 / (std + eps) of d_x [count] (accumulated in double by one workgroup).  On the handle's stream, no host sync."""
        count, eps, ddof = int(count), float(eps), int(ddof)
        if count < 0 or ddof not in (0, 1) or (count >= 1 and count - ddof < 1) or not (np.isfinite(eps) and eps >= 0.0):
            raise ValueError('count %r >= 0, ddof %r in {0, 1} with count - ddof >= 1, eps %r finite and >= 0' % (count, ddof, eps))
        if d_x is None or d_stats is None:
            raise ValueError('d_x and d_stats must be given')
        h = self._h
        h.adv_stats_device(h.adv_stats_struct(count, d_x, d_stats, eps, ddof))

    def adv_apply_device(self, d_x, count, d_stats, d_y=None):
        """d_y [count] = (d_x - d_stats[0]) * d_stats[1]; d_y None: in place.  The statistics are read on the stream: no host sync."""
        if d_x is None or d_stats is None or int(count) < 0:
            raise ValueError('d_x and d_stats must be given, count %r >= 0' % (count,))
        self._h.adv_apply_device(d_x, int(count), d_stats, d_x if d_y is None else d_y)

    def normalize_advantages_device(self, d_adv, count, d_stats, eps=1e-8, ddof=0, d_out=None):
        """The two calls above in a row: d_out (None: d_adv itself) = (adv - mean) / (std + eps) over the whole rollout; d_stats [2] keeps the
        statistics.  On the handle's stream, no host sync."""
        self.adv_stats_device(d_adv, count, d_stats, eps, ddof)
        self.adv_apply_device(d_adv, count, d_stats, d_out)

    def normalize_advantages(self, adv, eps=1e-8, ddof=0):
        """adv (any shape) -> (normalised adv of the same shape, stats [2] = mean | 1 / (std + eps)), numpy."""
        adv = np.ascontiguousarray(adv, np.float32)
        out, stats = np.empty(adv.shape, np.float32), np.zeros(2, np.float32)
        if adv.size == 0:
            return out, stats
        h, ptrs = self._h, []
        try:
            ptrs.append(h.device_alloc(adv.nbytes))
            ptrs.append(h.device_alloc(8))
            h.upload(ptrs[0], adv)
            self.normalize_advantages_device(ptrs[0], adv.size, ptrs[1], eps, ddof)
            h.sync()
            h.download(out, ptrs[0])
            h.download(stats, ptrs[1])
        finally:
            for p in ptrs:
                h.device_free(p)
        return out, stats

    # -- the clipped-surrogate gradient --
    @staticmethod
    def _actor(actor):
        if not isinstance(actor, GaussianActor):
            raise ValueError('actor must be a GaussianActor, not %r' % (type(actor),))
        return actor._loaded()

    def policy_grad_work_floats(self, actor, batch, chunk_rows=None):
        """floats of workspace ``policy_grad_device`` needs with ``grads``: the actor's gradient figure (with ``chunk_rows``: the chunked one)"""
        mlp = self._actor(actor)
        return self._h.ppo_policy_grad_work_floats(mlp, int(batch), actor._chunk_rows(chunk_rows) or 0)

    def policy_grad_device(self, actor, batch, d_x, d_preact_old, d_noise, d_adv, d_work=None, work_floats=0, clip=0.2, ent_coef=0.0, pscale=None,
                           escale=None, grads=None, d_ratio=None, d_logratio=None, d_clipped=None, d_ghead=None, ls_lo=LS_LO, ls_hi=LS_HI, x_stride=None,
                           preact_old_stride=None, noise_stride=None, chunk_rows=None):
        """PPO's actor update in one call (pmg_ppo_policy_grad_device): the gradient of the clipped surrogate and the entropy bonus
        (module docstring) with respect to ``actor``'s parameters from d_x [batch, Dx], d_preact_old [batch, 2 A] and d_noise [batch, A] (what
        ``act_device`` / ``sample_device`` returned as d_preact and d_noise when the action was drawn, with the same ls_lo / ls_hi) and d_adv
        [batch], all in device memory.  ``clip``: eps, or the pair (clip_lo, clip_hi).  The defaults ``pscale = -1 / batch``,
        ``escale = -ent_coef / batch`` are PPO's loss.  ``grads``: a ParamBuffers that receives dW / db (d_work then holds
        ``policy_grad_work_floats`` floats), or None (the outputs alone); d_ratio, d_logratio [batch] floats, d_clipped [batch] bytes and d_ghead
        [batch, 2 A] are optional.  ``chunk_rows``: as in ``grad_device``.  On the handle's stream, no host sync."""
        mlp, A = self._actor(actor), actor.widths[-1] // 2
        chunk_rows = actor._chunk_rows(chunk_rows)
        ls_lo, ls_hi = _clamp(ls_lo, ls_hi)
        clip_lo, clip_hi = _clip(clip)
        batch = int(batch)
        pscale = -1.0 / max(batch, 1) if pscale is None else float(pscale)
        escale = -float(ent_coef) / max(batch, 1) if escale is None else float(escale)
        if not (np.isfinite(pscale) and np.isfinite(escale)):
            raise ValueError('pscale %r and escale %r must be finite' % (pscale, escale))
        if grads is not None and (not isinstance(grads, ParamBuffers) or grads.widths != list(actor.widths)):
            raise ValueError('grads must be a ParamBuffers of the actor')
        h = self._h
        g = h.ppo_policy_grad_struct(batch, d_x, actor.widths[0] if x_stride is None else x_stride, d_preact_old,
                                     2 * A if preact_old_stride is None else preact_old_stride, d_noise, A if noise_stride is None else noise_stride, d_adv,
                                     pscale, escale, clip_lo, clip_hi, ls_lo, ls_hi, None if grads is None else grads.struct, d_ratio, d_logratio, d_clipped,
                                     d_ghead, 2 * A, d_work, int(work_floats))
        h.ppo_policy_grad_device(mlp, g, chunk_rows or 0)

    def policy_grad(self, actor, x, preact_old, noise, adv, clip=0.2, ent_coef=0.0, pscale=None, escale=None, grads=True, ls_lo=LS_LO, ls_hi=LS_HI,
                    chunk_rows=None):
        """x [B, Dx], preact_old [B, 2 A], noise [B, A], adv [B] -> dict(dW, db: lists per layer, or None with ``grads=False``; ratio [B];
        logratio [B]; clipped [B] bool; ghead [B, 2 A]), numpy.  The arguments are those of ``policy_grad_device``."""
        self._actor(actor)
        chunk_rows = actor._chunk_rows(chunk_rows)
        h, Dx, A = self._h, actor.widths[0], actor.widths[-1] // 2
        x, preact_old, noise, adv = (np.ascontiguousarray(v, np.float32) for v in (x, preact_old, noise, adv))
        if x.ndim != 2 or x.shape[1] != Dx:
            raise ValueError('x %s must be [B, %d]' % (x.shape, Dx))
        B = x.shape[0]
        if preact_old.shape != (B, 2 * A) or noise.shape != (B, A) or adv.shape != (B,):
            raise ValueError('preact_old %s, noise %s, adv %s must be [%d, %d], [%d, %d], [%d]' % (preact_old.shape, noise.shape, adv.shape, B, 2 * A, B, A, B))
        _clip(clip)
        _clamp(ls_lo, ls_hi)
        res = {'dW': None, 'db': None, 'ratio': np.empty(B, np.float32), 'logratio': np.empty(B, np.float32), 'clipped': np.empty(B, np.uint8),
               'ghead': np.empty((B, 2 * A), np.float32)}
        has_bias = [bool(actor._mlp.d_bias[l]) for l in range(len(actor.widths) - 1)]
        if B == 0:
            if grads:
                res['dW'] = [np.zeros((actor.widths[l + 1], actor.widths[l]), np.float32) for l in range(len(has_bias))]
                res['db'] = [np.zeros(actor.widths[l + 1], np.float32) if keep else None for l, keep in enumerate(has_bias)]
            res['clipped'] = res['clipped'].astype(bool)
            return res
        ptrs, bufs = [], None
        try:
            def put(arr):
                ptrs.append(h.device_alloc(arr.nbytes))
                h.upload(ptrs[-1], arr)
                return ptrs[-1]

            def room(arr):
                ptrs.append(h.device_alloc(arr.nbytes))
                return ptrs[-1]
            d_x, d_zo, d_n, d_adv = put(x), put(preact_old), put(noise), put(adv)
            keys = ('ratio', 'logratio', 'clipped', 'ghead')
            d = {k: room(res[k]) for k in keys}
            work, d_work = 0, None
            if grads:
                work = self.policy_grad_work_floats(actor, B, chunk_rows)
                d_work = h.device_alloc(4 * max(work, 1))
                ptrs.append(d_work)
                bufs = ParamBuffers(h, actor.widths, has_bias)
            self.policy_grad_device(actor, B, d_x, d_zo, d_n, d_adv, d_work, work, clip, ent_coef, pscale, escale, bufs, d['ratio'], d['logratio'],
                                    d['clipped'], d['ghead'], ls_lo, ls_hi, chunk_rows=chunk_rows)
            h.sync()
            for k in keys:
                h.download(res[k], d[k])
            if grads:
                res['dW'], res['db'] = bufs.download()
        finally:
            for p in ptrs:
                h.device_free(p)
            if bufs is not None:
                bufs.close()
        res['clipped'] = res['clipped'].astype(bool)
        return res

    # -- the statistics of a minibatch --
    def stats_device(self, batch, d_ratio, d_logratio, d_clipped, d_adv, d_stats, clip=0.2):
        """d_stats [4] = approximate KL (mean of rho - 1 - log rho) | clip fraction | mean clipped surrogate | mean log-ratio, from the per-row
        outputs of ``policy_grad_device`` and the advantages of the same ``batch`` rows.  On the handle's stream, no host sync."""
        clip_lo, clip_hi = _clip(clip)
        if int(batch) < 1 or any(p is None for p in (d_ratio, d_logratio, d_clipped, d_adv, d_stats)):
            raise ValueError('batch %r must be >= 1 and every pointer given' % (batch,))
        h = self._h
        h.ppo_stats_device(h.ppo_stats_struct(int(batch), d_ratio, d_logratio, d_clipped, d_adv, d_stats, clip_lo, clip_hi))

    def stats(self, ratio, logratio, clipped, adv, clip=0.2):
        """ratio, logratio, adv [B] float, clipped [B] bool -> dict(approx_kl, clip_fraction, surrogate, mean_logratio), numpy float32."""
        ratio, logratio, adv = (np.ascontiguousarray(v, np.float32) for v in (ratio, logratio, adv))
        clipped = np.ascontiguousarray(clipped).astype(np.uint8)
        B = ratio.shape[0] if ratio.ndim == 1 else -1
        if B < 1 or logratio.shape != (B,) or adv.shape != (B,) or clipped.shape != (B,):
            raise ValueError('ratio, logratio, clipped and adv must be [B] with B >= 1')
        h, ptrs = self._h, []
        out = np.empty(4, np.float32)
        try:
            for arr in (ratio, logratio, clipped, adv):
                ptrs.append(h.device_alloc(arr.nbytes))
                h.upload(ptrs[-1], arr)
            ptrs.append(h.device_alloc(16))
            self.stats_device(B, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], clip)
            h.sync()
            h.download(out, ptrs[4])
        finally:
            for p in ptrs:
                h.device_free(p)
        return dict(zip(('approx_kl', 'clip_fraction', 'surrogate', 'mean_logratio'), out))
