"""The stochastic actor of soft actor-critic (SAC) on the device: a tanh-squashed Gaussian policy -- action, log-probability and the noise
used -- on minibatch rows and on the env's current rows.

Host-side face of ``pmg_sac_sample_device`` and ``pmg_sac_act_env_device`` (include/pmg.h) and of ``pmg_sac_policy_grad_device``
and ``pmg_sac_alpha_device`` (3.16: the actor's half of an update in one call, and the temperature step); the soft target is
``Critic.sac_target_device`` (critic.py), the update side -- gradients, Adam, Polyak -- comes from ``optim.Trainable``.  All arithmetic happens
in the HIP library; this file uploads the network, validates shapes and moves buffers.  The network is an MLP with 2 A identity outputs:
units [0, A) are the mean m, units [A, 2 A) the log standard deviation, clamped to [ls_lo, ls_hi]:

    u = m + exp(ls) n,  a = tanh(u),  log pi = sum_j [ -n^2 / 2 - ls - log(2 pi) / 2 - log(1 - tanh(u)^2) ],  n ~ N(0, 1) (sample) or 0

A device-resident rollout is two stream-ordered calls per step, as with ``Actor``:

    pi = env.gaussian_actor; pi.load(weights, biases)      # the last layer has 2 A outputs
    pi.act_device(d_actions, seed=s, counter=t)            # sample=False: the mode tanh(m)
    h.step_device(d_actions)

One SAC update (``critic, critic2`` online, ``critic_t, critic2_t`` their Polyak targets, all loaded ``Critic`` objects; ``u`` counts the
updates; ``temp`` a ``Temperature`` after ``temp.init(alpha0)``, whose ``d_alpha`` is one float in device memory -- a fixed temperature is the
number ``alpha`` in its place).  Every call is stream-ordered on the handle's stream; nothing is computed on the host and nothing waits:

    critic_t.sac_target_device(pi, critic2_t, d_xn, d_r, d_y, 0.98, -1 / (1 - 0.98), 0.0, 0.0, d_alpha=temp.d_alpha, seed=s, counter=2 * u,
                               d_terminal=d_ok, d_next_action=d_na, batch=B)                                # y; the ONLINE actor, alpha from d_alpha
    for c, st in ((critic, sc), (critic2, s2)):
        c.grad_device(B, d_x, Dx, d_work, work, d_a=d_a, a_dim=A, d_target=d_y, gscale=2.0 / B, grads=st.g, chunk_rows=R)
        c.adam_step_device(st.g, st, lr)
    # the actor's half: sample, both critics, the smaller Q's ga, the head gradient and the actor's backward in ONE call
    pi.policy_grad_device(B, d_x, critic, critic2, d_pwork, pwork, d_alpha=temp.d_alpha, grads=sa.g, d_logp=d_lp, seed=s, counter=2 * u + 1,
                          chunk_rows=R)                     # pwork = pi.policy_grad_work_floats(B, critic2, chunk_rows=R)
    pi.adam_step_device(sa.g, sa, lr)
    temp.update_device(d_lp, B, -float(A), lr, u + 1)       # log_alpha's Adam step from mean(log pi); alpha = exp(log_alpha) for the next update
    critic_t.soft_update_from(critic, tau); critic2_t.soft_update_from(critic2, tau)

Before 3.16 the actor's half was ``sample_device``, two ``q_device``, two input-only ``grad_device`` calls on the critics, a download, the numpy
fix-up ``actor_head_grad`` below, an upload and the actor's ``grad_device``.  ``actor_head_grad`` stays as the reference of that recipe: the
tests hold the fused call to it.

The head gradient of ``mean_b(alpha log pi - min(Q1, Q2))`` with respect to (m, ls), with ga = d(-Q / B) / da from the critic:

    gout_mu = 2 alpha a / B + ga (1 - a^2)
    gout_ls = alpha (2 a sd n - 1) / B + ga (1 - a^2) sd n        where ls_lo <= z_ls <= ls_hi, else 0 (the clamp's derivative)

(d log pi / du = 2 tanh(u) = 2 a; d log pi / d ls = -1 + 2 a sd n; the -n^2 / 2 term does not depend on the parameters.)
"""
import numpy as np

from .actor import KINDS, upload_network
from .optim import ParamBuffers, Trainable

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

    def _online_critic(self, critic, what='critic'):
        from .critic import Critic
        if not isinstance(critic, Critic):
            raise ValueError('%s must be a Critic (whose loaded network is the online critic), not %r' % (what, type(critic)))
        mlp = critic._loaded()
        if self.widths[0] + self.widths[-1] // 2 != critic.widths[0]:
            raise ValueError('the actor maps %d -> 2 * %d, %s takes %d inputs' % (self.widths[0], self.widths[-1] // 2, what, critic.widths[0]))
        return mlp

    def policy_grad_work_floats(self, batch, critic2=None, action=False, chunk_rows=None):
        """floats of workspace ``policy_grad_device`` needs for ``batch`` rows: the actor's gradient figure (with ``chunk_rows``: the chunked one),
        + batch * A unless d_action is given (``action=True``), + batch * A with a second critic"""
        mlp = self._loaded()
        chunk_rows = self._chunk_rows(chunk_rows)
        return self._h.sac_policy_grad_work_floats(mlp, bool(action), critic2 is not None, int(batch), chunk_rows or 0)

    def policy_grad_device(self, batch, d_x, critic, critic2, d_work, work_floats, alpha=0.0, d_alpha=None, gscale=None, lscale=None, grads=None,
                           d_action=None, d_logp=None, d_q1=None, d_q2=None, d_gaction=None, d_ghead=None, sample=True, seed=0, counter=0, row_offset=0,
                           ls_lo=LS_LO, ls_hi=LS_HI, x_stride=None, chunk_rows=None):
        """SAC's actor half in one call (pmg_sac_policy_grad_device): the gradient of
        ``lscale * alpha * sum log pi(a | x) + gscale * sum min(Q1, Q2)(x, a)`` with respect to this network's parameters, a reparameterised,
        through ``critic`` and ``critic2`` (None: one critic), from d_x [batch, Dx] in device memory.  The defaults ``lscale = 1 / batch``,
        ``gscale = -1 / batch`` are SAC's ``mean(alpha log pi - min Q)``.  ``alpha``: a number, or ``d_alpha``: one float in device memory
        (``Temperature.d_alpha``).  ``grads``: a ParamBuffers that receives dW / db, or None (the outputs alone); d_action [batch, A], d_logp,
        d_q1, d_q2 [batch], d_gaction [batch, A] and d_ghead [batch, 2 A] are optional, contiguous.  The draws are those of ``sample_device``
        for the same (seed, counter, row_offset).  ``chunk_rows``: as in ``grad_device``.  On the handle's stream, no host sync."""
        mlp, A = self._loaded(), self.widths[-1] // 2
        c1 = self._online_critic(critic)
        c2 = None if critic2 is None else self._online_critic(critic2, 'critic2')
        chunk_rows = self._chunk_rows(chunk_rows)
        ls_lo, ls_hi = _clamp(ls_lo, ls_hi)
        if int(row_offset) < 0:
            raise ValueError('row_offset %r must be >= 0' % (row_offset,))
        gscale = -1.0 / max(int(batch), 1) if gscale is None else float(gscale)
        lscale = 1.0 / max(int(batch), 1) if lscale is None else float(lscale)
        alpha = float(alpha)
        if not (np.isfinite(gscale) and np.isfinite(lscale) and np.isfinite(alpha) and alpha >= 0.0):
            raise ValueError('gscale %r and lscale %r must be finite, alpha %r finite and >= 0' % (gscale, lscale, alpha))
        h = self._h
        g = h.sac_policy_grad_struct(int(batch), d_x, self.widths[0] if x_stride is None else x_stride, d_work, int(work_floats), gscale, lscale, alpha,
                                     ls_lo, ls_hi, bool(sample), int(seed), int(counter), int(row_offset), d_alpha, None if grads is None else grads.struct,
                                     d_action, A, d_logp, d_q1, d_q2, d_gaction, A, d_ghead, 2 * A)
        h.sac_policy_grad_device(mlp, c1, c2, g, chunk_rows or 0)

    def policy_grad(self, x, critic, critic2, alpha, gscale=None, lscale=None, grads=True, sample=True, seed=0, counter=0, row_offset=0, ls_lo=LS_LO,
                    ls_hi=LS_HI, chunk_rows=None):
        """x [B, Dx] -> dict(dW, db: lists per layer, or None with ``grads=False``; action [B, A]; logp [B]; q1 [B]; q2 [B] or None; gaction
        [B, A]; ghead [B, 2 A]), numpy.  The arguments are those of ``policy_grad_device``."""
        self._loaded()
        self._online_critic(critic)
        if critic2 is not None:
            self._online_critic(critic2, 'critic2')
        chunk_rows = self._chunk_rows(chunk_rows)
        h, Dx, A = self._h, self.widths[0], self.widths[-1] // 2
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[1] != Dx:
            raise ValueError('x %s must be [B, %d]' % (x.shape, Dx))
        B = x.shape[0]
        res = {'dW': None, 'db': None, 'action': np.empty((B, A), np.float32), 'logp': np.empty(B, np.float32), 'q1': np.empty(B, np.float32),
               'q2': None if critic2 is None else np.empty(B, np.float32), 'gaction': np.empty((B, A), np.float32), 'ghead': np.empty((B, 2 * A), np.float32)}
        has_bias = [bool(self._mlp.d_bias[l]) for l in range(len(self.widths) - 1)]
        if B == 0:
            if grads:
                res['dW'] = [np.zeros((self.widths[l + 1], self.widths[l]), np.float32) for l in range(len(has_bias))]
                res['db'] = [np.zeros(self.widths[l + 1], np.float32) if keep else None for l, keep in enumerate(has_bias)]
            return res
        ptrs, bufs = [], None
        try:
            def room(arr):
                if arr is None:
                    return None
                ptrs.append(h.device_alloc(arr.nbytes))
                return ptrs[-1]
            d_x = room(x)
            h.upload(d_x, x)
            keys = ('action', 'logp', 'q1', 'q2', 'gaction', 'ghead')
            d = {k: room(res[k]) for k in keys}
            work = self.policy_grad_work_floats(B, critic2, True, chunk_rows if grads else None)
            d_work = h.device_alloc(4 * max(work, 1))
            ptrs.append(d_work)
            if grads:
                bufs = ParamBuffers(h, self.widths, has_bias)
            self.policy_grad_device(B, d_x, critic, critic2, d_work, work, alpha, None, gscale, lscale, bufs, d['action'], d['logp'], d['q1'], d['q2'],
                                    d['gaction'], d['ghead'], sample, seed, counter, row_offset, ls_lo, ls_hi, chunk_rows=chunk_rows)
            h.sync()
            for k in keys:
                if res[k] is not None:
                    h.download(res[k], d[k])
            if grads:
                res['dW'], res['db'] = bufs.download()
        finally:
            for p in ptrs:
                h.device_free(p)
            if bufs is not None:
                bufs.close()
        return res

    def close(self):
        """Free the uploaded network and the Adam states made for it."""
        self._close_states()
        if getattr(self._h, 'h', None):
            for p in self._ptrs:
                self._h.device_free(p)
        self._ptrs, self._mlp, self.widths = [], None, None


class Temperature:
    """SAC's learned temperature on the device (pmg_sac_alpha_device): four floats in device memory, log_alpha | m | v | alpha.
    ``d_alpha`` is the address of the last one: pass it to ``Critic.sac_target_device`` and ``GaussianActor.policy_grad_device``, which read
    it on the stream -- a learned temperature needs no host sync."""

    def __init__(self, env):
        self._h = env.handle
        self._d_state = None

    def init(self, alpha0):
        """(Re)start from alpha0 > 0 with Adam's moments at zero."""
        alpha0 = float(alpha0)
        if not (np.isfinite(alpha0) and alpha0 > 0.0):
            raise ValueError('alpha0 %r must be finite and > 0' % (alpha0,))
        if self._d_state is None:
            self._d_state = self._h.device_alloc(16)
        self._h.upload(self._d_state, np.array([np.log(alpha0), 0.0, 0.0, alpha0], np.float32))

    def _state(self):
        if self._d_state is None:
            raise ValueError('no temperature: call init() first')
        return self._d_state

    @property
    def d_alpha(self):
        return self._state() + 12

    def update_device(self, d_logp, batch, target_entropy, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
        """One Adam step (step >= 1 counts them) on log_alpha with g = -(mean(logp) + target_entropy) from d_logp [batch] in device memory, then
        alpha = exp(log_alpha).  On the handle's stream, no host sync."""
        state = self._state()
        batch, step, target_entropy = int(batch), int(step), float(target_entropy)
        lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
        if d_logp is None or batch < 1 or step < 1 or not np.isfinite(target_entropy):
            raise ValueError('d_logp must be given, batch %r and step %r >= 1, target_entropy %r finite' % (batch, step, target_entropy))
        if not (np.isfinite(lr) and np.isfinite(eps) and eps >= 0.0 and 0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError('lr %r must be finite, eps %r finite and >= 0, the betas %r / %r in [0, 1)' % (lr, eps, beta1, beta2))
        h = self._h
        h.sac_alpha_device(h.sac_alpha_struct(batch, d_logp, state, target_entropy, lr, step, beta1, beta2, eps))

    def value(self):
        """-> alpha as it is on the device now (waits for the stream)"""
        out = np.empty(4, np.float32)
        self._h.sync()
        self._h.download(out, self._state())
        return out[3]

    def close(self):
        if self._d_state is not None and getattr(self._h, 'h', None):
            self._h.device_free(self._d_state)
        self._d_state = None
