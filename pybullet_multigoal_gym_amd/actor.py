"""The actor of a goal-conditioned learner on the device: a small MLP and DDPG / HER's exploration on its output.

Host-side face of ``pmg_mlp_forward_device``, ``pmg_act_env_device`` (include/pmg.h) and ``pmg_policy_grad_device``, the
actor's half of an update through the critic in one call, and of ``pmg_policy_grad_bc_device``, the same with a
behaviour-cloning term and its Q-filter on the demonstration rows of the minibatch.  All arithmetic happens
in the HIP library; this file uploads the network, validates shapes and moves buffers.  The library keeps no learner state: the
weights live in buffers this object owns until ``close()`` (or the next ``load``).  A device-resident rollout is two
stream-ordered calls per step and nothing leaves the GPU:

    env.actor.load(weights, biases)                         # torch layout: weights[l] is [out, in]
    d_actions = h.device_alloc(4 * N * A)                   # once
    env.actor.act_device(d_actions, noise_eps=0.2, random_eps=0.3, seed=s, counter=t)
    h.step_device(d_actions)
"""
import numpy as np

from ._lib import PMG_NORM_OBSERVATION, PMG_NORM_POLICY_STATE
from .optim import ParamBuffers, Trainable

KINDS = {'observation': PMG_NORM_OBSERVATION, 'policy_state': PMG_NORM_POLICY_STATE}
ACTIVATIONS = {'identity': 0, 'tanh': 1}
MAX_LAYERS, MAX_WIDTH = 4, 256


def upload_network(h, weights, biases=None, outputs=None):
    """Check a network (weights[l] is [out_l, in_l], biases[l] is [out_l] or None; 1..MAX_LAYERS layers of 1..MAX_WIDTH units, each layer's
    inputs the outputs of the one before; ``outputs``: the width the last layer must have) and upload it -> every device pointer (to free),
    widths, weight pointers, bias pointers.  Nothing is allocated when a check fails.  Shared by ``Actor.load`` and ``Critic.load``."""
    weights = [np.ascontiguousarray(w, np.float32) for w in weights]
    L = len(weights)
    if not 1 <= L <= MAX_LAYERS:
        raise ValueError('a network has 1..%d layers, not %d' % (MAX_LAYERS, L))
    biases = [None] * L if biases is None else [None if b is None else np.ascontiguousarray(b, np.float32) for b in biases]
    if len(biases) != L:
        raise ValueError('%d biases for %d layers' % (len(biases), L))
    for l, (w, b) in enumerate(zip(weights, biases)):
        if w.ndim != 2 or not (1 <= w.shape[0] <= MAX_WIDTH and 1 <= w.shape[1] <= MAX_WIDTH):
            raise ValueError('weights[%d] must be [out, in] with both in 1..%d, not %s' % (l, MAX_WIDTH, w.shape))
        if l and w.shape[1] != weights[l - 1].shape[0]:
            raise ValueError('weights[%d] takes %d inputs, layer %d has %d outputs' % (l, w.shape[1], l - 1, weights[l - 1].shape[0]))
        if b is not None and b.shape != (w.shape[0],):
            raise ValueError('biases[%d] must have shape (%d,), not %s' % (l, w.shape[0], b.shape))
    if outputs is not None and weights[-1].shape[0] != outputs:
        raise ValueError('the last layer must have %d output(s), not %d' % (outputs, weights[-1].shape[0]))
    ptrs, d_w, d_b = [], [], []
    for w, b in zip(weights, biases):
        for a, out in ((w, d_w), (b, d_b)):
            if a is None:
                out.append(None)
                continue
            p = h.device_alloc(a.nbytes)
            ptrs.append(p)
            h.upload(p, a)
            out.append(p)
    return ptrs, [weights[0].shape[1]] + [w.shape[0] for w in weights], d_w, d_b


class Actor(Trainable):
    """``env.actor``: an MLP with ReLU hidden layers on the env's device, and the actions of the env's current rows."""

    def __init__(self, env):
        self._env = env
        self._h = env.handle
        self._ptrs = []
        self._mlp = None
        self.widths = None

    def load(self, weights, biases=None, out_activation='tanh'):
        """Upload a network: weights[l] is [out_l, in_l] (torch ``nn.Linear.weight``), biases[l] is [out_l] or None; 1..4 layers
        of 1..256 units, each layer's inputs the outputs of the one before.  Replaces a network loaded earlier."""
        if out_activation not in ACTIVATIONS:
            raise ValueError('out_activation must be one of %s, not %r' % (sorted(ACTIVATIONS), out_activation))
        loaded = upload_network(self._h, weights, biases)
        self.close()
        self._ptrs, self.widths, d_w, d_b = loaded
        self._mlp = self._h.mlp_struct(self.widths, d_w, d_b, ACTIVATIONS[out_activation])

    def _loaded(self):
        if self._mlp is None:
            raise ValueError('no network: call load() first')
        return self._mlp

    def forward(self, x):
        """x [..., width[0]] -> out_activation(z) [..., width[L]]."""
        mlp, h = self._loaded(), self._h
        x = np.ascontiguousarray(x, np.float32)
        K, A = self.widths[0], self.widths[-1]
        if x.ndim == 0 or x.shape[-1] != K:
            raise ValueError('x %s must have a shape ending in %d' % (x.shape, K))
        B = x.size // K
        out = np.empty(x.shape[:-1] + (A,), np.float32)
        if B == 0:
            return out
        d_in, d_out = h.device_alloc(x.nbytes), None
        try:
            d_out = h.device_alloc(out.nbytes)
            h.upload(d_in, x)
            h.mlp_forward_device(mlp, d_in, K, B, d_out, A)
            h.sync()
            h.download(out, d_out)
        finally:
            h.device_free(d_in)
            if d_out is not None:
                h.device_free(d_out)
        return out

    def act_device(self, d_actions_ptr, kind='policy_state', noise_eps=0.0, random_eps=0.0, seed=0, counter=0, d_preact_ptr=None):
        """Actions [N, A] of the env's current rows into device memory (then ``handle.step_device(d_actions_ptr)``); on the
        handle's stream, no host sync.  The draws are a pure function of (seed, counter, global env index, column)."""
        if kind not in KINDS:
            raise ValueError('kind must be one of %s, not %r' % (sorted(KINDS), kind))
        if not float(noise_eps) >= 0.0 or not np.isfinite(noise_eps):
            raise ValueError('noise_eps %r must be finite and >= 0' % (noise_eps,))
        if not 0.0 <= float(random_eps) <= 1.0:
            raise ValueError('random_eps %r is outside [0, 1]' % (random_eps,))
        ex = self._h.explore_struct(float(noise_eps), float(random_eps), int(seed), int(counter))
        self._h.act_env_device(self._loaded(), KINDS[kind], d_actions_ptr, d_preact_ptr, ex)

    def act(self, kind='policy_state', noise_eps=0.0, random_eps=0.0, seed=0, counter=0):
        """-> actions [N, A] of the env's current rows (numpy)."""
        h = self._h
        out = np.empty((h.N, h.dims.action_dim), np.float32)
        d_out = h.device_alloc(out.nbytes)
        try:
            self.act_device(d_out, kind, noise_eps, random_eps, seed, counter)
            h.sync()
            h.download(out, d_out)
        finally:
            h.device_free(d_out)
        return out

    def _online_critic(self, critic):
        from .critic import Critic
        if not isinstance(critic, Critic):
            raise ValueError('critic must be a Critic (whose loaded network is the online critic), not %r' % (type(critic),))
        mlp = critic._loaded()
        if self.widths[0] + self.widths[-1] != critic.widths[0]:
            raise ValueError('the actor maps %d -> %d, the critic takes %d inputs' % (self.widths[0], self.widths[-1], critic.widths[0]))
        return mlp

    def policy_grad_work_floats(self, critic, batch, chunk_rows=None):
        """floats of workspace ``policy_grad_device`` needs for ``batch`` rows (with ``chunk_rows``: for the chunked reduction)"""
        mlp = self._loaded()
        chunk_rows = self._chunk_rows(chunk_rows)
        return self._h.policy_grad_work_floats(mlp, self._online_critic(critic), int(batch), chunk_rows or 0)

    def policy_grad_device(self, critic, batch, d_x, d_work, work_floats, gscale, l2scale=0.0, grads=None, d_action=None, d_out=None, d_q=None,
                           d_gaction=None, x_stride=None, chunk_rows=None):
        """The actor's half of an update in one call (pmg_policy_grad_device): the gradient of
        ``gscale * sum Q(x, clip(pi(x))) + l2scale / 2 * sum pi(x)^2`` with respect to this network's parameters, through ``critic``, from
        d_x [batch, Dx] in device memory.  HER's ``-mean Q + action_l2 * mean(pi^2)`` is ``gscale = -1 / B``, ``l2scale = 2 * action_l2 / (B * A)``.
        ``grads``: a ParamBuffers that receives dW / db, or None (the outputs alone); d_action = clip(pi(x)) [batch, A], d_out = pi(x)
        unclipped, d_q = Q [batch] and d_gaction = dLoss / da [batch, A] are optional, contiguous.  ``chunk_rows``: as in ``grad_device``.
        On the handle's stream, no host sync."""
        mlp, A = self._loaded(), self.widths[-1]
        cmlp = self._online_critic(critic)
        chunk_rows = self._chunk_rows(chunk_rows)
        g = self._h.policy_grad_struct(int(batch), d_x, self.widths[0] if x_stride is None else x_stride, d_work, int(work_floats), float(gscale),
                                       float(l2scale), None if grads is None else grads.struct, d_action, A, d_out, A, d_q, d_gaction, A)
        self._h.policy_grad_device(mlp, cmlp, g, chunk_rows or 0)

    def policy_grad(self, critic, x, gscale, l2scale=0.0, grads=True, chunk_rows=None):
        """x [B, Dx] -> dict(dW, db: lists per layer, or None with ``grads=False``; action [B, A] = clip(pi(x)); out [B, A] = pi(x); q [B];
        gaction [B, A] = dLoss / da).  gscale, l2scale, chunk_rows: as in ``policy_grad_device``."""
        self._loaded()
        self._online_critic(critic)
        chunk_rows = self._chunk_rows(chunk_rows)
        h, Dx, A = self._h, self.widths[0], self.widths[-1]
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[1] != Dx:
            raise ValueError('x %s must be [B, %d]' % (x.shape, Dx))
        if not np.isfinite(gscale) or not np.isfinite(l2scale):
            raise ValueError('gscale %r and l2scale %r must be finite' % (gscale, l2scale))
        B = x.shape[0]
        res = {'dW': None, 'db': None, 'action': np.empty((B, A), np.float32), 'out': np.empty((B, A), np.float32), 'q': np.empty(B, np.float32),
               'gaction': np.empty((B, A), np.float32)}
        has_bias = [bool(self._mlp.d_bias[l]) for l in range(len(self.widths) - 1)]
        if B == 0:
            if grads:
                res['dW'] = [np.zeros((self.widths[l + 1], self.widths[l]), np.float32) for l in range(len(has_bias))]
                res['db'] = [np.zeros(self.widths[l + 1], np.float32) if keep else None for l, keep in enumerate(has_bias)]
            return res
        ptrs, bufs = [], None
        try:
            def room(arr):
                ptrs.append(h.device_alloc(arr.nbytes))
                return ptrs[-1]
            d_x = room(x)
            h.upload(d_x, x)
            outs = [(res[k], room(res[k])) for k in ('action', 'out', 'q', 'gaction')]
            work = self.policy_grad_work_floats(critic, B, chunk_rows if grads else None)
            d_work = h.device_alloc(4 * max(work, 1))
            ptrs.append(d_work)
            if grads:
                bufs = ParamBuffers(h, self.widths, has_bias)
            self.policy_grad_device(critic, B, d_x, d_work, work, gscale, l2scale, bufs, outs[0][1], outs[1][1], outs[2][1], outs[3][1],
                                    chunk_rows=chunk_rows)
            h.sync()
            for arr, p in outs:
                h.download(arr, p)
            if grads:
                res['dW'], res['db'] = bufs.download()
        finally:
            for p in ptrs:
                h.device_free(p)
            if bufs is not None:
                bufs.close()
        return res

    def policy_grad_bc_device(self, critic, batch, d_x, d_demo_action, demo_begin, d_work, work_floats, gscale, bcscale, l2scale=0.0, q_filter=True,
                              grads=None, d_action=None, d_out=None, d_q=None, d_gaction=None, d_q_demo=None, d_filter=None, x_stride=None,
                              demo_action_stride=None, chunk_rows=None):
        """``policy_grad_device`` with a behaviour-cloning term on the demonstration rows (pmg_policy_grad_bc_device): rows from
        ``demo_begin`` on are demonstrations with the actions d_demo_action [batch, A] (indexed by the batch row; rows below ``demo_begin`` are not
        read, None is allowed with ``demo_begin == batch``).  The term ``bcscale / 2 * sum (pi(x) - a_demo)^2`` runs over the demonstration rows
        -- with ``q_filter`` only over those where the critic rates the demonstrated action above the policy's own.  baselines'
        ``prm_loss_weight * -mean Q + aux_loss_weight * sum of squares`` is ``gscale = -prm_loss_weight / B``, ``bcscale = 2 * aux_loss_weight``.
        d_q_demo [batch] floats (written from ``demo_begin`` on) and d_filter [batch] bytes are optional; the workspace is
        ``policy_grad_work_floats``.  On the handle's stream, no host sync."""
        mlp, A = self._loaded(), self.widths[-1]
        cmlp = self._online_critic(critic)
        chunk_rows = self._chunk_rows(chunk_rows)
        g = self._h.policy_grad_struct(int(batch), d_x, self.widths[0] if x_stride is None else x_stride, d_work, int(work_floats), float(gscale),
                                       float(l2scale), None if grads is None else grads.struct, d_action, A, d_out, A, d_q, d_gaction, A)
        bc = self._h.policy_bc_struct(int(demo_begin), d_demo_action, A if demo_action_stride is None else demo_action_stride, float(bcscale),
                                      1 if q_filter else 0, d_q_demo, d_filter)
        self._h.policy_grad_bc_device(mlp, cmlp, g, bc, chunk_rows or 0)

    def policy_grad_bc(self, critic, x, demo_action, demo_begin, gscale, bcscale, l2scale=0.0, q_filter=True, grads=True, chunk_rows=None):
        """x [B, Dx], demo_action [B, A] (rows below ``demo_begin`` are not read) -> ``policy_grad``'s dict plus q_demo [B] (NaN below
        ``demo_begin``, where nothing is computed) and filter [B] bool.  The arguments are those of ``policy_grad_bc_device``."""
        self._loaded()
        self._online_critic(critic)
        chunk_rows = self._chunk_rows(chunk_rows)
        h, Dx, A = self._h, self.widths[0], self.widths[-1]
        x = np.ascontiguousarray(x, np.float32)
        demo_action = np.ascontiguousarray(demo_action, np.float32)
        if x.ndim != 2 or x.shape[1] != Dx:
            raise ValueError('x %s must be [B, %d]' % (x.shape, Dx))
        B = x.shape[0]
        if demo_action.shape != (B, A):
            raise ValueError('demo_action %s must be [%d, %d]' % (demo_action.shape, B, A))
        if not np.isfinite(gscale) or not np.isfinite(l2scale) or not np.isfinite(bcscale):
            raise ValueError('gscale %r, l2scale %r and bcscale %r must be finite' % (gscale, l2scale, bcscale))
        if int(demo_begin) != demo_begin or not 0 <= demo_begin <= B:
            raise ValueError('demo_begin %r must be an integer in [0, %d]' % (demo_begin, B))
        res = {'dW': None, 'db': None, 'action': np.empty((B, A), np.float32), 'out': np.empty((B, A), np.float32), 'q': np.empty(B, np.float32),
               'gaction': np.empty((B, A), np.float32), 'q_demo': np.full(B, np.nan, np.float32), 'filter': np.zeros(B, np.uint8)}
        has_bias = [bool(self._mlp.d_bias[l]) for l in range(len(self.widths) - 1)]
        if B == 0:
            if grads:
                res['dW'] = [np.zeros((self.widths[l + 1], self.widths[l]), np.float32) for l in range(len(has_bias))]
                res['db'] = [np.zeros(self.widths[l + 1], np.float32) if keep else None for l, keep in enumerate(has_bias)]
            res['filter'] = res['filter'].astype(bool)
            return res
        ptrs, bufs = [], None
        try:
            def room(arr, fill=False):
                ptrs.append(h.device_alloc(arr.nbytes))
                if fill:
                    h.upload(ptrs[-1], arr)
                return ptrs[-1]
            d_x, d_ad = room(x, True), room(demo_action, True)
            outs = [(res[k], room(res[k], k == 'q_demo')) for k in ('action', 'out', 'q', 'gaction', 'q_demo', 'filter')]
            work = self.policy_grad_work_floats(critic, B, chunk_rows if grads else None)
            d_work = h.device_alloc(4 * max(work, 1))
            ptrs.append(d_work)
            if grads:
                bufs = ParamBuffers(h, self.widths, has_bias)
            self.policy_grad_bc_device(critic, B, d_x, d_ad, int(demo_begin), d_work, work, gscale, bcscale, l2scale, q_filter, bufs, outs[0][1], outs[1][1],
                                       outs[2][1], outs[3][1], outs[4][1], outs[5][1], chunk_rows=chunk_rows)
            h.sync()
            for arr, p in outs:
                h.download(arr, p)
            if grads:
                res['dW'], res['db'] = bufs.download()
        finally:
            for p in ptrs:
                h.device_free(p)
            if bufs is not None:
                bufs.close()
        res['filter'] = res['filter'].astype(bool)
        return res

    def close(self):
        """Free the uploaded network and the Adam states made for it."""
        self._close_states()
        if getattr(self._h, 'h', None):
            for p in self._ptrs:
                self._h.device_free(p)
        self._ptrs, self._mlp, self.widths = [], None, None
