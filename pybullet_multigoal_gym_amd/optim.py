"""The update side of a device-resident learner: gradients of a loaded network, Adam on its weights, Polyak onto a target.

Host-side face of ``pmg_mlp_grad_device``, ``pmg_mlp_grad_chunked_device``, ``pmg_mlp_adam_device`` and ``pmg_mlp_polyak_device``
(include/pmg.h).  All
arithmetic happens in the HIP library.  ``Trainable`` is what ``Actor`` and ``Critic`` share: both are networks whose uploaded weights
the object owns, so both get ``grad_device`` / ``grad`` / ``adam_step_device`` / ``soft_update_from`` from here.  ``ParamBuffers`` is a
set of device tensors shaped like a network (gradients, Adam's moments); ``AdamState`` owns the two moments, a gradient buffer and t.
For a data-parallel learner ``Trainable`` also carries the rank-ordered merge of the ranks' gradients:
``allreduce_grads_device``, ``adam_step_allreduce_device``, ``allreduce_work_floats`` and the numpy faces ``pack_params`` / ``merge_params``.
"""
import numpy as np


class ParamBuffers:
    """Device tensors with the shapes of a network's weights and biases, zero at first; freed by ``close()``."""

    def __init__(self, h, widths, has_bias):
        self._h = h
        self.widths, self.has_bias = list(widths), list(has_bias)
        self.d_w, self.d_b, self._ptrs = [], [], []
        try:
            for l in range(len(self.widths) - 1):
                for n, keep, out in ((self.widths[l + 1] * self.widths[l], True, self.d_w), (self.widths[l + 1], self.has_bias[l], self.d_b)):
                    if not keep:
                        out.append(None)
                        continue
                    p = h.device_alloc(4 * n)
                    self._ptrs.append(p)
                    h.upload(p, np.zeros(n, np.float32))
                    out.append(p)
        except Exception:
            self.close()
            raise
        self.struct = h.params_struct(self.d_w, self.d_b)

    def _shapes(self):
        L = len(self.widths) - 1
        return [(self.widths[l + 1], self.widths[l]) for l in range(L)], [(self.widths[l + 1],) for l in range(L)]

    def upload(self, weights, biases=None):
        ws, bs = self._shapes()
        for l, shape in enumerate(ws):
            w = np.ascontiguousarray(weights[l], np.float32)
            b = None if not self.has_bias[l] else np.ascontiguousarray(biases[l], np.float32)
            if w.shape != shape or (b is not None and b.shape != bs[l]):
                raise ValueError('tensor %d has shape %s, the network needs %s' % (l, w.shape, shape))
            self._h.upload(self.d_w[l], w)
            if b is not None:
                self._h.upload(self.d_b[l], b)

    def download(self):
        """-> weights [L], biases [L] (None where the network has no bias); waits for the stream"""
        self._h.sync()
        ws, bs = self._shapes()
        W, b = [np.empty(s, np.float32) for s in ws], [np.empty(s, np.float32) if keep else None for s, keep in zip(bs, self.has_bias)]
        for l in range(len(ws)):
            self._h.download(W[l], self.d_w[l])
            if b[l] is not None:
                self._h.download(b[l], self.d_b[l])
        return W, b

    def close(self):
        if getattr(self._h, 'h', None):
            for p in self._ptrs:
                self._h.device_free(p)
        self._ptrs, self.d_w, self.d_b = [], [], []


class AdamState:
    """Adam's state for one network: the moments ``m`` and ``v``, a gradient buffer ``g`` to hand to ``grad_device``, and the step
    count ``t`` (0 before the first step)."""

    def __init__(self, net):
        net._loaded()
        has_bias = [bool(net._mlp.d_bias[l]) for l in range(len(net.widths) - 1)]
        self.m = self.v = self.g = None
        try:
            self.m = ParamBuffers(net._h, net.widths, has_bias)
            self.v = ParamBuffers(net._h, net.widths, has_bias)
            self.g = ParamBuffers(net._h, net.widths, has_bias)
        except Exception:
            self.close()
            raise
        self.t = 0

    def close(self):
        for b in (self.m, self.v, self.g):
            if b is not None:
                b.close()
        self.m = self.v = self.g = None


class Trainable:
    """What ``Actor`` and ``Critic`` share on the update side.  The object has ``_h``, ``_mlp``, ``widths`` and ``_loaded()``."""

    def adam_state(self):
        """A new AdamState of the loaded network; ``close()`` (and the next ``load``) frees it with the weights."""
        state = AdamState(self)
        self.__dict__.setdefault('_states', []).append(state)
        return state

    def _close_states(self):
        for state in self.__dict__.pop('_states', []):
            state.close()

    def _own_params(self):
        mlp = self._loaded()
        L = len(self.widths) - 1
        return self._h.params_struct([mlp.d_weight[l] for l in range(L)], [mlp.d_bias[l] for l in range(L)])

    def parameters(self):
        """-> weights [L], biases [L] as they are on the device now (numpy; waits for the stream)"""
        mlp, h = self._loaded(), self._h
        h.sync()
        L = len(self.widths) - 1
        W = [np.empty((self.widths[l + 1], self.widths[l]), np.float32) for l in range(L)]
        b = [np.empty(self.widths[l + 1], np.float32) if mlp.d_bias[l] else None for l in range(L)]
        for l in range(L):
            h.download(W[l], mlp.d_weight[l])
            if b[l] is not None:
                h.download(b[l], mlp.d_bias[l])
        return W, b

    @staticmethod
    def _chunk_rows(chunk_rows):
        """None, or the even integer >= 2 that pmg_mlp_grad_chunked_device takes"""
        if chunk_rows is None:
            return None
        if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, (int, np.integer)) or chunk_rows < 2 or chunk_rows % 2:
            raise ValueError('chunk_rows %r must be an even integer >= 2 (or None: one chain over the batch)' % (chunk_rows,))
        return int(chunk_rows)

    def grad_work_floats(self, batch, chunk_rows=None):
        """floats of workspace ``grad_device`` needs for ``batch`` rows (with ``chunk_rows``: for the chunked reduction)"""
        chunk_rows = self._chunk_rows(chunk_rows)
        if chunk_rows is None:
            return self._h.mlp_grad_work_floats(self._loaded(), int(batch))
        return self._h.mlp_grad_chunked_work_floats(self._loaded(), int(batch), chunk_rows)

    def grad_device(self, batch, d_x, x_dim, d_work, work_floats, d_a=None, a_dim=0, d_gout=None, d_target=None, gscale=1.0, grads=None, d_gx=None,
                    d_ga=None, d_out=None, x_stride=None, a_stride=None, chunk_rows=None):
        """Forward and backward of ``batch`` rows in device memory: d_x [batch, x_dim] (and d_a [batch, a_dim]: the rows x | a); the head is
        d_gout, gscale * (out - d_target) or the constant gscale; ``grads``: a ParamBuffers that receives dW / db, or None; d_gx, d_ga, d_out
        optional; contiguous rows unless a stride is given.  On the handle's stream, no host sync.

        ``chunk_rows`` (an even integer >= 2; None: one chain over the batch): dW / db are summed per chunk of that many rows and the
        chunks' sums added in ascending order (pmg_mlp_grad_chunked_device): other bits than the single chain's, the same
        bits for the same rows, order and chunk_rows; d_work then holds ``grad_work_floats(batch, chunk_rows)`` floats.  Measured on
        3 x 256 networks (3.12): about half the single chain's time at B = 4096 (best: chunk_rows = 256) and 0.27 x at B = 65 536 (best of
        those tried: 1024); at B = 256 it gains 2 % at most, leave it None there."""
        mlp, A = self._loaded(), self.widths[-1]
        chunk_rows = self._chunk_rows(chunk_rows)
        g = self._h.grad_struct(int(batch), d_x, x_dim if x_stride is None else x_stride, x_dim, d_work, int(work_floats), d_a,
                                a_dim if a_stride is None else a_stride, a_dim, d_gout, A, d_target, A, float(gscale),
                                None if grads is None else grads.struct, d_gx, x_dim, d_ga, a_dim, d_out, A)
        if chunk_rows is None:
            self._h.mlp_grad_device(mlp, g)
        else:
            self._h.mlp_grad_chunked_device(mlp, g, chunk_rows)

    def grad(self, x, a=None, gout=None, target=None, gscale=1.0, grads=True, chunk_rows=None):
        """x [B, x_dim] (and a [B, a_dim]) -> dict(dW, db: lists per layer, or None with ``grads=False``; gx [B, x_dim]; ga [B, a_dim] or
        None; out [B, width[L]]).  gout / target [B, width[L]]: the head (at most one).  chunk_rows: as in ``grad_device``."""
        self._loaded()
        chunk_rows = self._chunk_rows(chunk_rows)
        h, A = self._h, self.widths[-1]
        x = np.ascontiguousarray(x, np.float32)
        a = None if a is None else np.ascontiguousarray(a, np.float32)
        if x.ndim != 2 or (a is not None and (a.ndim != 2 or a.shape[0] != x.shape[0])) or x.shape[1] + (0 if a is None else a.shape[1]) != self.widths[0] \
                or x.shape[1] < 1 or (a is not None and a.shape[1] < 1):
            raise ValueError('x %s%s must be [B, .] rows whose widths sum to %d' % (x.shape, '' if a is None else ' / a %s' % (a.shape,), self.widths[0]))
        B = x.shape[0]
        if gout is not None and target is not None:
            raise ValueError('give gout or target, not both')
        head = gout if gout is not None else target
        if head is not None:
            head = np.ascontiguousarray(head, np.float32)
            if head.shape != (B, A):
                raise ValueError('gout / target %s must be [%d, %d]' % (head.shape, B, A))
        if not np.isfinite(gscale):
            raise ValueError('gscale %r must be finite' % (gscale,))
        res = {'dW': None, 'db': None, 'gx': np.empty(x.shape, np.float32), 'ga': None if a is None else np.empty(a.shape, np.float32),
               'out': np.empty((B, A), np.float32)}
        mlp = self._mlp
        has_bias = [bool(mlp.d_bias[l]) for l in range(len(self.widths) - 1)]
        if B == 0:
            if grads:
                res['dW'] = [np.zeros((self.widths[l + 1], self.widths[l]), np.float32) for l in range(len(has_bias))]
                res['db'] = [np.zeros(self.widths[l + 1], np.float32) if keep else None for l, keep in enumerate(has_bias)]
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
            d_x, d_a, d_head = put(x), None if a is None else put(a), None if head is None else put(head)
            d_gx, d_ga, d_out = room(res['gx']), None if a is None else room(res['ga']), room(res['out'])
            work = self.grad_work_floats(B, chunk_rows if grads else None)
            d_work = h.device_alloc(4 * max(work, 1))
            ptrs.append(d_work)
            if grads:
                bufs = ParamBuffers(h, self.widths, has_bias)
            self.grad_device(B, d_x, x.shape[1], d_work, work, d_a, 0 if a is None else a.shape[1], d_head if gout is not None else None,
                             d_head if target is not None else None, gscale, bufs, d_gx, d_ga, d_out, chunk_rows=chunk_rows)
            h.sync()
            h.download(res['gx'], d_gx)
            h.download(res['out'], d_out)
            if a is not None:
                h.download(res['ga'], d_ga)
            if grads:
                res['dW'], res['db'] = bufs.download()
        finally:
            for p in ptrs:
                h.device_free(p)
            if bufs is not None:
                bufs.close()
        return res

    def adam_step_device(self, grads, state, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        """One Adam step on this object's own uploaded weights.  ``grads``: a ParamBuffers (e.g. ``state.g`` after ``grad_device``) or the
        dict ``grad()`` returned (uploaded into ``state.g``).  Advances ``state.t``.  On the handle's stream, no host sync."""
        mlp = self._loaded()
        adam = self._adam_args(state, lr, beta1, beta2, eps)
        if isinstance(grads, dict):
            state.g.upload(grads['dW'], grads['db'])
            grads = state.g
        if not isinstance(grads, ParamBuffers) or grads.widths != list(self.widths):
            raise ValueError('grads must be a ParamBuffers of this network or the dict grad() returns')
        self._h.mlp_adam_device(mlp, self._own_params(), grads.struct, state.m.struct, state.v.struct, adam)
        state.t += 1

    # -- data-parallel learner: the rank-ordered merge of gradients (include/pmg.h) --
    def _grads_of(self, grads):
        if not isinstance(grads, ParamBuffers) or grads.widths != list(self.widths):
            raise ValueError('grads must be a ParamBuffers of this network')
        return grads

    def _adam_args(self, state, lr, beta1, beta2, eps):
        if not isinstance(state, AdamState) or state.m is None or state.m.widths != list(self.widths):
            raise ValueError('state must be an open AdamState of this network')
        lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
        if not (np.isfinite(lr) and np.isfinite(eps) and eps >= 0.0 and 0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError('lr %r must be finite, eps %r finite and >= 0, the betas %r / %r in [0, 1)' % (lr, eps, beta1, beta2))
        return self._h.adam_struct(lr, state.t + 1, beta1, beta2, eps)

    def param_floats(self):
        """P: the floats of this network's tensors in their flat order (weight 0, bias 0, weight 1, ...)"""
        return self._h.mlp_param_floats(self._loaded())

    def allreduce_work_floats(self):
        """floats of workspace ``allreduce_grads_device`` / ``adam_step_allreduce_device`` need: (nranks + 1) * P"""
        return self._h.mlp_allreduce_work_floats(self._loaded())

    def allreduce_grads_device(self, grads, d_work, work_floats):
        """``grads`` (a ParamBuffers each rank filled with ``grad_device`` on ITS rows, gscale = ... / B_global) becomes the ranks' gradients
        added in rank order, in place: the bits of ``grad_device(chunk_rows=B_local)`` on the concatenated batch on one GPU, the same on every
        rank.  A collective on the handle's stream (every rank calls it), no host sync; not while ``comm_overlap`` is on."""
        self._h.mlp_grad_allreduce_device(self._loaded(), self._grads_of(grads).struct, d_work, int(work_floats))

    def adam_step_allreduce_device(self, grads, state, lr, d_work, work_floats, beta1=0.9, beta2=0.999, eps=1e-8):
        """``allreduce_grads_device`` and ``adam_step_device`` in one sweep: the summed gradient is never stored; ``grads`` keeps this rank's own.
        Advances ``state.t``.  A collective on the handle's stream, no host sync."""
        mlp = self._loaded()
        adam = self._adam_args(state, lr, beta1, beta2, eps)
        self._h.mlp_adam_allreduce_device(mlp, self._own_params(), self._grads_of(grads).struct, state.m.struct, state.v.struct, adam, d_work, int(work_floats))
        state.t += 1

    def _flat(self, flat, rows=None):
        P = self.param_floats()
        a = np.ascontiguousarray(flat, np.float32)
        if (a.ndim != 1 and rows is None) or (rows is not None and a.ndim != 2) or a.shape[-1] != P or a.shape[0] < 1:
            raise ValueError('expected %s of %d floats, got shape %s' % ('a flat gradient' if rows is None else 'slots [R, P]', P, a.shape))
        return a

    def pack_params(self, weights, biases=None):
        """numpy face of pmg_mlp_params_pack_device: the tensors (lists per layer, as ``grad()`` returns dW / db) -> one flat array [P]"""
        mlp, h = self._loaded(), self._h
        has_bias = [bool(mlp.d_bias[l]) for l in range(len(self.widths) - 1)]
        out = np.empty(self.param_floats(), np.float32)
        bufs, d_flat = ParamBuffers(h, self.widths, has_bias), None
        try:
            bufs.upload(weights, biases)
            d_flat = h.device_alloc(out.nbytes)
            h.mlp_params_pack_device(mlp, bufs.struct, d_flat)
            h.sync()
            h.download(out, d_flat)
        finally:
            bufs.close()
            if d_flat is not None:
                h.device_free(d_flat)
        return out

    def merge_params(self, slots):
        """numpy face of pmg_mlp_params_merge_device: slots [R, P] (row r: rank r's flat gradient) -> (dW, db), lists per layer, the slots
        added in ascending r in float32"""
        mlp, h = self._loaded(), self._h
        slots = self._flat(slots, rows=True)
        has_bias = [bool(mlp.d_bias[l]) for l in range(len(self.widths) - 1)]
        bufs, d_slots = ParamBuffers(h, self.widths, has_bias), None
        try:
            d_slots = h.device_alloc(slots.nbytes)
            h.upload(d_slots, slots)
            h.mlp_params_merge_device(mlp, d_slots, slots.shape[1], slots.shape[0], bufs.struct)
            return bufs.download()
        finally:
            bufs.close()
            if d_slots is not None:
                h.device_free(d_slots)

    def soft_update_from(self, other, tau):
        """Polyak onto this object's weights: w = fmaf(tau, other's w - w, w).  On the handle's stream, no host sync."""
        self._loaded()
        if not isinstance(other, Trainable) or other._mlp is None or list(other.widths) != list(self.widths) or \
                any(bool(other._mlp.d_bias[l]) != bool(self._mlp.d_bias[l]) for l in range(len(self.widths) - 1)):
            raise ValueError('other must be a loaded network of the same shape')
        tau = float(tau)
        if not 0.0 <= tau <= 1.0:
            raise ValueError('tau %r is outside [0, 1]' % (tau,))
        self._h.mlp_polyak_device(other._mlp, self._own_params(), tau)
