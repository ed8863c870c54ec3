"""The stochastic actor of soft actor-critic (SAC) on the device: a tanh-squashed Gaussian policy -- action, log-probability and the noise
used -- on minibatch rows and on the env's current rows.

Host-side face of ``pmg_sac_sample_device`` and ``pmg_sac_act_env_device`` (include/pmg.h); the soft target is
``Critic.sac_target_device`` (critic.py), the update side -- gradients, Adam, Polyak -- comes from ``optim.Trainable``.  All arithmetic happens
in the HIP library; this file uploads the network, validates shapes and moves buffers.  The network is an MLP with 2 A identity outputs:
units [0, A) are the mean m, units [A, 2 A) the log standard deviation, clamped to [ls_lo, ls_hi]:

    u = m + exp(ls) n,  a = tanh(u),  log pi = sum_j [ -n^2 / 2 - ls - log(2 pi) / 2 - log(1 - tanh(u)^2) ],  n ~ N(0, 1) (sample) or 0

A device-resident rollout is two stream-ordered calls per step, as with ``Actor``:

    pi = env.gaussian_actor; pi.load(weights, biases)      # the last layer has 2 A outputs
    pi.act_device(d_actions, seed=s, counter=t)            # sample=False: the mode tanh(m)
    h.step_device(d_actions)

One SAC update (``critic, critic2`` online, ``critic_t, critic2_t`` their Polyak targets, all loaded ``Critic`` objects; ``u`` counts the
updates; ``alpha`` the temperature, or ``d_alpha`` one float in device memory).  Everything but the four-line fix-up of the actor's half runs
on the device:

    critic_t.sac_target_device(pi, critic2_t, d_xn, d_r, d_y, 0.98, -1 / (1 - 0.98), 0.0, alpha, seed=s, counter=2 * u,
                               d_terminal=d_ok, d_next_action=d_na, batch=B)                                # y; the ONLINE actor
    for c, st in ((critic, sc), (critic2, s2)):
        c.grad_device(B, d_x, Dx, d_work, work, d_a=d_a, a_dim=A, d_target=d_y, gscale=2.0 / B, grads=st.g, chunk_rows=R)
        c.adam_step_device(st.g, st, lr)
    pi.sample_device(B, d_x, d_action=d_pa, d_logp=d_lp, d_noise=d_n, d_preact=d_z, seed=s, counter=2 * u + 1)   # a, log pi, n, z
    critic.q_device(d_x, Dx, d_pa, A, B, d_q1); critic2.q_device(d_x, Dx, d_pa, A, B, d_q2)
    # per row, the critic with the smaller Q supplies ga = d(-Q / B) / da:
    critic.grad_device(B, d_x, Dx, d_work, work, d_a=d_pa, a_dim=A, gscale=-1.0 / B, d_ga=d_ga1)            # likewise critic2 -> d_ga2
    # the host fix-up (``actor_head_grad`` below), the one piece the fused SAC policy gradient will take over:
    gout = actor_head_grad(a, n, z, np.where((q1 <= q2)[:, None], ga1, ga2), alpha, ls_lo, ls_hi)          # [B, 2 A]
    pi.grad_device(B, d_x, Dx, d_work, work, d_gout=d_gout, grads=sa.g, chunk_rows=R); pi.adam_step_device(sa.g, sa, lr)
    critic_t.soft_update_from(critic, tau); critic2_t.soft_update_from(critic2, tau)

The head gradient of ``mean_b(alpha log pi - min(Q1, Q2))`` with respect to (m, ls), with ga = d(-Q / B) / da from the critic:

    gout_mu = 2 alpha a / B + ga (1 - a^2)
    gout_ls = alpha (2 a sd n - 1) / B + ga (1 - a^2) sd n        where ls_lo <= z_ls <= ls_hi, else 0 (the clamp's derivative)

(d log pi / du = 2 tanh(u) = 2 a; d log pi / d ls = -1 + 2 a sd n; the -n^2 / 2 term does not depend on the parameters.)
"""
import numpy as np

from .actor import KINDS, upload_network
from .optim import Trainable

LS_LO, LS_HI = -20.0, 2.0


def actor_head_grad(a, n, z, ga, alpha, ls_lo=LS_LO, ls_hi=LS_HI):
    """The host fix-up of the SAC actor step: a, n, ga [B, A], z [B, 2 A] (what ``sample`` and the critic's ``grad`` return, ga already scaled
    by -1 / B) -> gout [B, 2 A] float32, the gradient of mean_b(alpha log pi - Q) with respect to the actor's outputs."""
    a, n, z, ga = (np.asarray(v, np.float32) for v in (a, n, z, ga))
    B, A = a.shape
    f = np.float32
    ls_raw = z[:, A:]
    inrange = (ls_raw >= f(ls_lo)) & (ls_raw <= f(ls_hi))
    sdn = np.exp(np.clip(ls_raw, f(ls_lo), f(ls_hi))) * n
    d = ga * (f(1) - a * a)
    out = np.empty((B, 2 * A), np.float32)
    out[:, :A] = f(2) * f(alpha) * a / f(B) + d
    out[:, A:] = np.where(inrange, f(alpha) * (f(2) * a * sdn - f(1)) / f(B) + d * sdn, f(0))
    return out


def _clamp(ls_lo, ls_hi):
    ls_lo, ls_hi = float(ls_lo), float(ls_hi)
    if not (np.isfinite(ls_lo) and np.isfinite(ls_hi) and ls_lo <= ls_hi):
        raise ValueError('ls_lo %r / ls_hi %r must be finite and ordered' % (ls_lo, ls_hi))
    return ls_lo, ls_hi


class GaussianActor(Trainable):
    """``env.gaussian_actor``: an MLP with ReLU hidden layers and 2 A identity outputs (means | log-stds) on the env's device."""

    def __init__(self, env):
        self._env = env
        self._h = env.handle
        self._ptrs = []
        self._mlp = None
        self.widths = None

    @property
    def action_dim(self):
        self._loaded()
        return self.widths[-1] // 2

    def load(self, weights, biases=None):
        """Upload a network as ``Actor.load`` does; the last layer must have an even number of outputs (means | log-stds).  Replaces a network
        loaded earlier."""
        weights = list(weights)
        if len(weights) and np.ndim(weights[-1]) == 2 and np.shape(weights[-1])[0] % 2:
            raise ValueError('the last layer must have 2 A outputs (means | log-stds), not %d' % np.shape(weights[-1])[0])
        loaded = upload_network(self._h, weights, biases)
        self.close()
        self._ptrs, self.widths, d_w, d_b = loaded
        self._mlp = self._h.mlp_struct(self.widths, d_w, d_b, 0)

    def _loaded(self):
        if self._mlp is None:
            raise ValueError('no network: call load() first')
        return self._mlp

    def sample_device(self, batch, d_x, d_action=None, d_logp=None, d_noise=None, d_preact=None, sample=True, seed=0, counter=0, row_offset=0,
                      ls_lo=LS_LO, ls_hi=LS_HI, x_stride=None):
        """a [batch, A], log pi [batch], n [batch, A] and z [batch, 2 A] of the rows d_x [batch, Dx] in device memory (each output optional,
        d_action or d_logp given; contiguous).  The draws are a function of (seed, counter, row_offset + row, column); sample=False: n = 0,
        the mode.  On the handle's stream, no host sync."""
        mlp, A = self._loaded(), self.widths[-1] // 2
        ls_lo, ls_hi = _clamp(ls_lo, ls_hi)
        if int(row_offset) < 0:
            raise ValueError('row_offset %r must be >= 0' % (row_offset,))
        if d_action is None and d_logp is None:
            raise ValueError('give d_action or d_logp')
        h = self._h
        s = h.sac_sample_struct(int(batch), d_x, self.widths[0] if x_stride is None else x_stride, d_action, A, d_logp, d_noise, A, d_preact, 2 * A,
                                ls_lo, ls_hi, bool(sample), int(seed), int(counter), int(row_offset))
        h.sac_sample_device(mlp, s)

    def sample(self, x, sample=True, seed=0, counter=0, row_offset=0, ls_lo=LS_LO, ls_hi=LS_HI, preact=False):
        """x [B, Dx] -> a [B, A], logp [B], n [B, A] (and z [B, 2 A] with ``preact=True``), numpy."""
        self._loaded()
        h, Dx, A = self._h, self.widths[0], self.widths[-1] // 2
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[1] != Dx:
            raise ValueError('x %s must be [B, %d]' % (x.shape, Dx))
        _clamp(ls_lo, ls_hi)
        if int(row_offset) < 0:
            raise ValueError('row_offset %r must be >= 0' % (row_offset,))
        B = x.shape[0]
        outs = [np.empty((B, A), np.float32), np.empty(B, np.float32), np.empty((B, A), np.float32), np.empty((B, 2 * A), np.float32)]
        if B:
            ptrs = []
            try:
                for arr in [x] + outs:
                    ptrs.append(h.device_alloc(arr.nbytes))
                h.upload(ptrs[0], x)
                self.sample_device(B, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], sample, seed, counter, row_offset, ls_lo, ls_hi)
                h.sync()
                for arr, p in zip(outs, ptrs[1:]):
                    h.download(arr, p)
            finally:
                for p in ptrs:
                    h.device_free(p)
        return tuple(outs) if preact else tuple(outs[:3])

    def act_device(self, d_actions_ptr, kind='policy_state', sample=True, seed=0, counter=0, d_logp=None, d_noise=None, d_preact=None,
                   ls_lo=LS_LO, ls_hi=LS_HI):
        """Actions [N, A] of the env's current rows into device memory (then ``handle.step_device(d_actions_ptr)``); d_logp [N], d_noise
        [N, A] and d_preact [N, 2 A] are optional.  The draws are a pure function of (seed, counter, global env index, column).  On the
        handle's stream, no host sync."""
        if kind not in KINDS:
            raise ValueError('kind must be one of %s, not %r' % (sorted(KINDS), kind))
        mlp, A = self._loaded(), self.widths[-1] // 2
        ls_lo, ls_hi = _clamp(ls_lo, ls_hi)
        if d_actions_ptr is None and d_logp is None:
            raise ValueError('give d_actions_ptr or d_logp')
        h = self._h
        s = h.sac_sample_struct(0, None, 0, d_actions_ptr, A, d_logp, d_noise, A, d_preact, 2 * A, ls_lo, ls_hi, bool(sample), int(seed), int(counter), 0)
        h.sac_act_env_device(mlp, KINDS[kind], s)

    def act(self, kind='policy_state', sample=True, seed=0, counter=0, ls_lo=LS_LO, ls_hi=LS_HI):
        """-> actions [N, A], logp [N] of the env's current rows (numpy)."""
        h = self._h
        self._loaded()
        a, lp = np.empty((h.N, h.dims.action_dim), np.float32), np.empty(h.N, np.float32)
        ptrs = []
        try:
            for arr in (a, lp):
                ptrs.append(h.device_alloc(arr.nbytes))
            self.act_device(ptrs[0], kind, sample, seed, counter, d_logp=ptrs[1], ls_lo=ls_lo, ls_hi=ls_hi)
            h.sync()
            h.download(a, ptrs[0])
            h.download(lp, ptrs[1])
        finally:
            for p in ptrs:
                h.device_free(p)
        return a, lp

    def close(self):
        """Free the uploaded network and the Adam states made for it."""
        self._close_states()
        if getattr(self._h, 'h', None):
            for p in self._ptrs:
                self._h.device_free(p)
        self._ptrs, self._mlp, self.widths = [], None, None
