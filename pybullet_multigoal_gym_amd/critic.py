"""The critic of a goal-conditioned DDPG / HER learner on the device: Q(x, a) on two row tables read in place, and the TD target
y = clip(r + gamma Q'(x', pi'(x'))) of a minibatch in one fused call.

Host-side face of ``pmg_q_device`` and ``pmg_td_target_device`` (include/pmg.h); the update side -- gradients, Adam, Polyak
 -- comes from ``optim.Trainable``, which ``Actor`` shares.  All arithmetic happens in the HIP library; this file uploads
the network, validates shapes and moves buffers.  The weights live in buffers this object owns until ``close()`` (or the next ``load``).
There is no learner class: one DDPG / HER update is this sequence of stream-ordered calls, with the online and the target networks in
four objects (``actor, critic = env.actor, env.critic; actor_t, critic_t = Actor(env), Critic(env)``, all loaded) and nothing leaving the
GPU:

    sa, sc = actor.adam_state(), critic.adam_state()                        # once: moments, a gradient buffer .g, t
    R = 256                    # chunk_rows of the two full gradients: 256 at B = 4096, 1024 at 65 536, None for B = 256
    work = max(actor.policy_grad_work_floats(critic, B, R), critic.grad_work_floats(B, R)); d_work = h.device_alloc(4 * work)
    h.her_sample_device(rows, E, T, es, ts, B, ..., d_x=d_x, d_x_next=d_xn, d_action=d_a, d_reward=d_r, d_goal_achieved=d_ok)
    critic_t.td_target_device(actor_t, d_xn, d_r, d_y, 0.98, -1 / (1 - 0.98), 0.0, d_terminal=d_ok, batch=B)          # y
    critic.grad_device(B, d_x, Dx, d_work, work, d_a=d_a, a_dim=A, d_target=d_y, gscale=2.0 / B, grads=sc.g, chunk_rows=R)   # d mean (Q - y)^2
    critic.adam_step_device(sc.g, sc, lr)
    actor.policy_grad_device(critic, B, d_x, d_work, work, gscale=-1.0 / B, l2scale=2.0 * action_l2 / (B * A), grads=sa.g, chunk_rows=R)
    actor.adam_step_device(sa.g, sa, lr)
    actor_t.soft_update_from(actor, tau); critic_t.soft_update_from(critic, tau)

The actor's line is the whole actor loss of HER, ``-mean Q(x, clip(pi(x))) + action_l2 * mean(pi(x)^2)``, in one call: the
call differentiates ``gscale * sum Q + l2scale / 2 * sum pi^2``, so ``gscale = -1 / B`` carries the mean over the batch and
``l2scale = 2 * action_l2 / (B * A)`` the mean over the B * A outputs and the 2 of the square's derivative; ``l2scale = 0`` is plain DDPG.
The gradient is zero where the clip is active, and the L2 term acts on the unclipped output.

TD3 is the same sequence with two critics and ``td3_target_device`` in place of ``td_target_device``: one target call with
target-policy smoothing and the smaller of the two target critics, the two critics' gradients on the SAME ``d_y``, and the actor and the
three Polyak updates on every ``policy_delay``-th update only -- a host-side ``if`` (``critic2, critic2_t = Critic(env), Critic(env)``, loaded;
``u`` counts the updates):

    s2 = critic2.adam_state()
    critic_t.td3_target_device(actor_t, critic2_t, d_xn, d_r, d_y, 0.98, -1 / (1 - 0.98), 0.0, 0.2, 0.5, seed, u,      # sigma 0.2, noise_clip 0.5
                               d_terminal=d_ok, d_next_action=d_na, batch=B)                                            # y; counter = u: fresh noise
    for c, s in ((critic, sc), (critic2, s2)):
        c.grad_device(B, d_x, Dx, d_work, work, d_a=d_a, a_dim=A, d_target=d_y, gscale=2.0 / B, grads=s.g, chunk_rows=R)
        c.adam_step_device(s.g, s, lr)
    if u % policy_delay == 0:
        actor.policy_grad_device(critic, B, d_x, d_work, work, gscale=-1.0 / B, l2scale=2.0 * action_l2 / (B * A), grads=sa.g, chunk_rows=R)
        actor.adam_step_device(sa.g, sa, lr)
        actor_t.soft_update_from(actor, tau); critic_t.soft_update_from(critic, tau); critic2_t.soft_update_from(critic2, tau)

The smoothed action both target critics saw goes to ``d_next_action`` [B, A]; without it the call keeps it in ``d_work``
(``td3_target_work_floats`` floats).  The noise of row b is a function of ``(seed, counter, row_offset + b)``, so a batch cut into pieces
(``row_offset`` = the piece's first row) gives the rows of the whole.  ``critic2 = None, sigma = 0`` is ``td_target_device``, bit for bit.

SAC takes ``sac_target_device`` with a ``sac.GaussianActor`` (the online one) in the actor's place: the sampled action, its
log-probability and ``y = clip(r + gamma (min(Q1', Q2')(x', a') - alpha log pi(a' | x')))`` in one call; the update recipe is in ``sac.py``.
"""
import numpy as np

from .actor import ACTIVATIONS, Actor, upload_network
from .optim import Trainable


class Critic(Trainable):
    """``env.critic``: an MLP with ReLU hidden layers and one output on the env's device."""

    def __init__(self, env):
        self._env = env
        self._h = env.handle
        self._ptrs = []
        self._mlp = None
        self.widths = None

    def load(self, weights, biases=None, out_activation='identity'):
        """Upload a network as ``Actor.load`` does; the last layer must have one output.  Replaces a network loaded earlier."""
        if out_activation not in ACTIVATIONS:
            raise ValueError('out_activation must be one of %s, not %r' % (sorted(ACTIVATIONS), out_activation))
        loaded = upload_network(self._h, weights, biases, outputs=1)
        self.close()
        self._ptrs, self.widths, d_w, d_b = loaded
        self._mlp = self._h.mlp_struct(self.widths, d_w, d_b, ACTIVATIONS[out_activation])

    def _loaded(self):
        if self._mlp is None:
            raise ValueError('no network: call load() first')
        return self._mlp

    def _target_actor(self, actor):
        if not isinstance(actor, Actor):
            raise ValueError('actor must be an Actor (whose loaded network is the target actor), not %r' % (type(actor),))
        mlp = actor._loaded()
        if actor.widths[0] + actor.widths[-1] != self.widths[0]:
            raise ValueError('the actor maps %d -> %d, the critic takes %d inputs' % (actor.widths[0], actor.widths[-1], self.widths[0]))
        return mlp

    def q_device(self, d_x_ptr, x_dim, d_a_ptr, a_dim, batch, d_q_ptr, x_stride=None, a_stride=None, q_stride=1):
        """d_q [batch] = Q(x, a) of the rows d_x [batch, x_dim] and d_a [batch, a_dim] in device memory (strides in floats, default:
        contiguous); on the handle's stream, no host sync."""
        self._h.q_device(self._loaded(), d_x_ptr, x_dim if x_stride is None else x_stride, x_dim, d_a_ptr, a_dim if a_stride is None else a_stride,
                         a_dim, batch, d_q_ptr, q_stride)

    def q(self, x, a):
        """x [..., x_dim], a [..., a_dim] -> Q(x, a) [...] (numpy)."""
        self._loaded()
        h = self._h
        x, a = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(a, np.float32)
        if x.ndim == 0 or a.ndim == 0 or x.shape[:-1] != a.shape[:-1] or x.shape[-1] < 1 or a.shape[-1] < 1 or x.shape[-1] + a.shape[-1] != self.widths[0]:
            raise ValueError('x %s / a %s must share their leading axes and their last axes sum to %d' % (x.shape, a.shape, self.widths[0]))
        out = np.empty(x.shape[:-1], np.float32)
        if out.size == 0:
            return out
        ptrs = []
        try:
            for arr in (x, a, out):
                ptrs.append(h.device_alloc(arr.nbytes))
            h.upload(ptrs[0], x)
            h.upload(ptrs[1], a)
            self.q_device(ptrs[0], x.shape[-1], ptrs[1], a.shape[-1], out.size, ptrs[2])
            h.sync()
            h.download(out, ptrs[2])
        finally:
            for p in ptrs:
                h.device_free(p)
        return out

    def td_target_device(self, actor, d_x_next, d_reward, d_y, gamma, clip_lo, clip_hi, d_terminal=None, d_q_next=None, d_next_action=None,
                         x_stride=None, *, batch):
        """d_y [batch] = clip(r + gamma Q'(x', pi'(x'))) with this network as Q' and ``actor``'s as pi', from d_x_next [batch, Dx] (x_stride
        floats from row to row, default Dx) and d_reward [batch]; d_terminal [batch] uint8 (non-zero: y = clip(r)), d_q_next [batch] and
        d_next_action [batch, A] are optional; clip_lo = -inf / clip_hi = inf: no clip.  On the handle's stream, no host sync."""
        mlp = self._loaded()
        amlp = self._target_actor(actor)
        gamma, clip_lo, clip_hi = float(gamma), float(clip_lo), float(clip_hi)
        if not gamma >= 0.0 or not np.isfinite(gamma):
            raise ValueError('gamma %r must be finite and >= 0' % (gamma,))
        if not clip_lo <= clip_hi:
            raise ValueError('clips %r / %r must be ordered and not NaN' % (clip_lo, clip_hi))
        h = self._h
        td = h.td_struct(int(batch), d_x_next, actor.widths[0] if x_stride is None else x_stride, d_reward, d_y, gamma,
                         clip_lo, clip_hi, d_terminal, d_q_next, d_next_action)
        h.td_target_device(amlp, mlp, td)

    def td_target(self, actor, x_next, reward, gamma, clip_lo=-float('inf'), clip_hi=float('inf'), terminal=None):
        """x_next [B, Dx], reward [B], terminal [B] or None -> y [B], q_next [B], next_action [B, A] (numpy)."""
        self._loaded()
        self._target_actor(actor)
        h = self._h
        Dx, A = actor.widths[0], actor.widths[-1]
        x_next, reward = np.ascontiguousarray(x_next, np.float32), np.ascontiguousarray(reward, np.float32)
        if x_next.ndim != 2 or x_next.shape[1] != Dx or reward.shape != (x_next.shape[0],):
            raise ValueError('x_next %s must be [B, %d] and reward %s [B]' % (x_next.shape, Dx, reward.shape))
        B = x_next.shape[0]
        if terminal is not None:
            terminal = np.ascontiguousarray(np.asarray(terminal) != 0, np.uint8)
            if terminal.shape != (B,):
                raise ValueError('terminal %s must be [B]' % (terminal.shape,))
        y, qn, na = np.empty(B, np.float32), np.empty(B, np.float32), np.empty((B, A), np.float32)
        if B == 0:
            return y, qn, na
        ins = [x_next, reward] + ([terminal] if terminal is not None else [])
        ptrs = []
        try:
            for arr in ins + [y, qn, na]:
                ptrs.append(h.device_alloc(arr.nbytes))
            for p, arr in zip(ptrs, ins):
                h.upload(p, arr)
            d_y, d_qn, d_na = ptrs[len(ins):]
            self.td_target_device(actor, ptrs[0], ptrs[1], d_y, gamma, clip_lo, clip_hi, ptrs[2] if terminal is not None else None, d_qn, d_na, batch=B)
            h.sync()
            for arr, p in ((y, d_y), (qn, d_qn), (na, d_na)):
                h.download(arr, p)
        finally:
            for p in ptrs:
                h.device_free(p)
        return y, qn, na

    def _twin(self, critic2):
        if critic2 is None:
            return None
        if not isinstance(critic2, Critic):
            raise ValueError('critic2 must be a Critic (whose loaded network is the second target critic) or None, not %r' % (type(critic2),))
        mlp2 = critic2._loaded()
        if critic2.widths[0] != self.widths[0]:
            raise ValueError('critic2 takes %d inputs, this critic %d' % (critic2.widths[0], self.widths[0]))
        return mlp2

    def td3_target_work_floats(self, actor, critic2, batch, next_action=False):
        """floats of workspace ``td3_target_device`` needs: batch * A with a second critic and no d_next_action, else 0."""
        self._loaded()
        return self._h.td3_target_work_floats(self._target_actor(actor), critic2 is not None, next_action, int(batch))

    def td3_target_device(self, actor, critic2, d_x_next, d_reward, d_y, gamma, clip_lo, clip_hi, sigma, noise_clip, seed, counter, row_offset=0,
                          d_terminal=None, d_q_min=None, d_q1=None, d_q2=None, d_next_action=None, d_work=None, work_floats=0, x_stride=None, *, batch):
        """TD3's target in one call: d_y [batch] = clip(r + gamma min(Q1', Q2')(x', a~)), a~ = clip(clip(pi'(x')) + clip(sigma n, -noise_clip,
        noise_clip), -1, 1), with this network as Q1', ``critic2``'s as Q2' (None: one critic, min = Q1') and ``actor``'s as pi'.  The draws n
        are a function of (seed, counter, row_offset + row, column); sigma = 0: no noise, no draw.  d_terminal, d_q_min, d_q1, d_q2 [batch] and
        d_next_action [batch, A] (a~) are optional.  With a second critic and without d_next_action, d_work holds at least
        ``td3_target_work_floats`` floats.  Allocates nothing; on the handle's stream, no host sync."""
        mlp = self._loaded()
        amlp = self._target_actor(actor)
        mlp2 = self._twin(critic2)
        gamma, clip_lo, clip_hi, sigma, noise_clip = float(gamma), float(clip_lo), float(clip_hi), float(sigma), float(noise_clip)
        if not gamma >= 0.0 or not np.isfinite(gamma):
            raise ValueError('gamma %r must be finite and >= 0' % (gamma,))
        if not clip_lo <= clip_hi:
            raise ValueError('clips %r / %r must be ordered and not NaN' % (clip_lo, clip_hi))
        if not sigma >= 0.0 or not np.isfinite(sigma):
            raise ValueError('sigma %r must be finite and >= 0' % (sigma,))
        if not noise_clip >= 0.0:
            raise ValueError('noise_clip %r must be >= 0 and not NaN' % (noise_clip,))
        if int(row_offset) < 0:
            raise ValueError('row_offset %r must be >= 0' % (row_offset,))
        h = self._h
        td = h.td3_struct(int(batch), d_x_next, actor.widths[0] if x_stride is None else x_stride, d_reward, d_y, gamma, clip_lo, clip_hi, sigma,
                          noise_clip, int(seed), int(counter), int(row_offset), d_terminal, d_q_min, d_q1, d_q2, d_next_action, d_work, int(work_floats))
        h.td3_target_device(amlp, mlp, mlp2, td)

    def td3_target(self, actor, critic2, x_next, reward, gamma, clip_lo=-float('inf'), clip_hi=float('inf'), sigma=0.0, noise_clip=float('inf'),
                   seed=0, counter=0, row_offset=0, terminal=None):
        """x_next [B, Dx], reward [B], terminal [B] or None -> y [B], q_min [B], q1 [B], q2 [B] (None without critic2), next_action [B, A]
        (numpy)."""
        self._loaded()
        self._target_actor(actor)
        self._twin(critic2)
        h = self._h
        Dx, A = actor.widths[0], actor.widths[-1]
        x_next, reward = np.ascontiguousarray(x_next, np.float32), np.ascontiguousarray(reward, np.float32)
        if x_next.ndim != 2 or x_next.shape[1] != Dx or reward.shape != (x_next.shape[0],):
            raise ValueError('x_next %s must be [B, %d] and reward %s [B]' % (x_next.shape, Dx, reward.shape))
        B = x_next.shape[0]
        if terminal is not None:
            terminal = np.ascontiguousarray(np.asarray(terminal) != 0, np.uint8)
            if terminal.shape != (B,):
                raise ValueError('terminal %s must be [B]' % (terminal.shape,))
        y, qm, q1, na = np.empty(B, np.float32), np.empty(B, np.float32), np.empty(B, np.float32), np.empty((B, A), np.float32)
        q2 = np.empty(B, np.float32) if critic2 is not None else None
        if B == 0:
            return y, qm, q1, q2, na
        ins = [x_next, reward] + ([terminal] if terminal is not None else [])
        outs = [y, qm, q1, na] + ([q2] if q2 is not None else [])
        ptrs = []
        try:
            for arr in ins + outs:
                ptrs.append(h.device_alloc(arr.nbytes))
            for p, arr in zip(ptrs, ins):
                h.upload(p, arr)
            d_out = ptrs[len(ins):]
            self.td3_target_device(actor, critic2, ptrs[0], ptrs[1], d_out[0], gamma, clip_lo, clip_hi, sigma, noise_clip, seed, counter, row_offset,
                                   d_terminal=ptrs[2] if terminal is not None else None, d_q_min=d_out[1], d_q1=d_out[2],
                                   d_q2=d_out[4] if q2 is not None else None, d_next_action=d_out[3], batch=B)
            h.sync()
            for arr, p in zip(outs, d_out):
                h.download(arr, p)
        finally:
            for p in ptrs:
                h.device_free(p)
        return y, qm, q1, q2, na

    def _gaussian_actor(self, actor):
        from .sac import GaussianActor
        if not isinstance(actor, GaussianActor):
            raise ValueError('actor must be a GaussianActor (SAC: the online one), not %r' % (type(actor),))
        mlp = actor._loaded()
        if actor.widths[0] + actor.widths[-1] // 2 != self.widths[0]:
            raise ValueError('the actor maps %d -> 2 * %d, the critic takes %d inputs' % (actor.widths[0], actor.widths[-1] // 2, self.widths[0]))
        return mlp

    def sac_target_work_floats(self, actor, batch, next_action=False):
        """floats of workspace ``sac_target_device`` needs: batch * A without d_next_action, else 0."""
        self._loaded()
        return self._h.sac_target_work_floats(self._gaussian_actor(actor), next_action, int(batch))

    def sac_target_device(self, actor, critic2, d_x_next, d_reward, d_y, gamma, clip_lo, clip_hi, alpha, sample=True, seed=0, counter=0, row_offset=0,
                          ls_lo=-20.0, ls_hi=2.0, d_alpha=None, d_terminal=None, d_q_min=None, d_q1=None, d_q2=None, d_next_action=None, d_logp=None,
                          d_work=None, work_floats=0, x_stride=None, *, batch):
        """SAC's soft target in one call: d_y [batch] = clip(r + gamma (min(Q1', Q2')(x', a') - alpha log pi(a' | x'))), a' and
        log pi sampled from the GaussianActor ``actor`` (SAC: the online one), with this network as Q1' and ``critic2``'s as Q2' (None: one
        critic).  ``d_alpha``: one float in device memory that replaces ``alpha`` (a learned temperature without a host sync).  The draws are a
        function of (seed, counter, row_offset + row, column); sample=False: the mode.  d_terminal, d_q_min, d_q1, d_q2, d_logp [batch] and
        d_next_action [batch, A] (a') are optional.  Without d_next_action, d_work holds at least ``sac_target_work_floats`` floats.
        Allocates nothing; on the handle's stream, no host sync."""
        mlp = self._loaded()
        amlp = self._gaussian_actor(actor)
        mlp2 = self._twin(critic2)
        gamma, clip_lo, clip_hi, alpha, ls_lo, ls_hi = float(gamma), float(clip_lo), float(clip_hi), float(alpha), float(ls_lo), float(ls_hi)
        if not gamma >= 0.0 or not np.isfinite(gamma):
            raise ValueError('gamma %r must be finite and >= 0' % (gamma,))
        if not clip_lo <= clip_hi:
            raise ValueError('clips %r / %r must be ordered and not NaN' % (clip_lo, clip_hi))
        if not alpha >= 0.0 or not np.isfinite(alpha):
            raise ValueError('alpha %r must be finite and >= 0' % (alpha,))
        if not (np.isfinite(ls_lo) and np.isfinite(ls_hi) and ls_lo <= ls_hi):
            raise ValueError('ls_lo %r / ls_hi %r must be finite and ordered' % (ls_lo, ls_hi))
        if int(row_offset) < 0:
            raise ValueError('row_offset %r must be >= 0' % (row_offset,))
        h = self._h
        td = h.sac_target_struct(int(batch), d_x_next, actor.widths[0] if x_stride is None else x_stride, d_reward, d_y, gamma, clip_lo, clip_hi, alpha, ls_lo,
                                 ls_hi, bool(sample), int(seed), int(counter), int(row_offset), d_alpha, d_terminal, d_q_min, d_q1, d_q2, d_next_action, d_logp,
                                 d_work, int(work_floats))
        h.sac_target_device(amlp, mlp, mlp2, td)

    def sac_target(self, actor, critic2, x_next, reward, gamma, alpha, clip_lo=-float('inf'), clip_hi=float('inf'), sample=True, seed=0, counter=0,
                   row_offset=0, ls_lo=-20.0, ls_hi=2.0, terminal=None):
        """x_next [B, Dx], reward [B], terminal [B] or None -> y [B], q_min [B], q1 [B], q2 [B] (None without critic2), next_action [B, A],
        logp [B] (numpy)."""
        self._loaded()
        self._gaussian_actor(actor)
        self._twin(critic2)
        h = self._h
        Dx, A = actor.widths[0], actor.widths[-1] // 2
        x_next, reward = np.ascontiguousarray(x_next, np.float32), np.ascontiguousarray(reward, np.float32)
        if x_next.ndim != 2 or x_next.shape[1] != Dx or reward.shape != (x_next.shape[0],):
            raise ValueError('x_next %s must be [B, %d] and reward %s [B]' % (x_next.shape, Dx, reward.shape))
        B = x_next.shape[0]
        if terminal is not None:
            terminal = np.ascontiguousarray(np.asarray(terminal) != 0, np.uint8)
            if terminal.shape != (B,):
                raise ValueError('terminal %s must be [B]' % (terminal.shape,))
        y, qm, q1, na, lp = np.empty(B, np.float32), np.empty(B, np.float32), np.empty(B, np.float32), np.empty((B, A), np.float32), np.empty(B, np.float32)
        q2 = np.empty(B, np.float32) if critic2 is not None else None
        if B == 0:
            return y, qm, q1, q2, na, lp
        ins = [x_next, reward] + ([terminal] if terminal is not None else [])
        outs = [y, qm, q1, na, lp] + ([q2] if q2 is not None else [])
        ptrs = []
        try:
            for arr in ins + outs:
                ptrs.append(h.device_alloc(arr.nbytes))
            for p, arr in zip(ptrs, ins):
                h.upload(p, arr)
            d_out = ptrs[len(ins):]
            self.sac_target_device(actor, critic2, ptrs[0], ptrs[1], d_out[0], gamma, clip_lo, clip_hi, alpha, sample, seed, counter, row_offset, ls_lo, ls_hi,
                                   d_terminal=ptrs[2] if terminal is not None else None, d_q_min=d_out[1], d_q1=d_out[2],
                                   d_q2=d_out[5] if q2 is not None else None, d_next_action=d_out[3], d_logp=d_out[4], batch=B)
            h.sync()
            for arr, p in zip(outs, d_out):
                h.download(arr, p)
        finally:
            for p in ptrs:
                h.device_free(p)
        return y, qm, q1, q2, na, lp

    def close(self):
        """Free the uploaded network and the Adam states made for it."""
        self._close_states()
        if getattr(self._h, 'h', None):
            for p in self._ptrs:
                self._h.device_free(p)
        self._ptrs, self._mlp, self.widths = [], None, None
