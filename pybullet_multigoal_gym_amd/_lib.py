"""ctypes binding of the C ABI in include/pmg.h (libpmg_hip.so, built by hipcc for gfx950).

There is no Python/NumPy fallback: if the shared library is missing this
module raises at load time with the build command.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, 'csrc', 'libpmg_hip.so')

TASK_IDS = {'reach': 0, 'push': 1, 'pick_and_place': 2, 'slide': 3, 'block_stack': 4, 'block_rearrange': 5,
            'chest_push': 6, 'chest_pick_and_place': 7}
PMG_BUF_PACKED = 7
PMG_BUF_STATE = 8
PMG_BUF_SCHED = 9
PMG_BUF_ENV_CYCLES = 10
PMG_BUF_WAVE_TRACE = 11
# one record of PMG_BUF_WAVE_TRACE (include/pmg.h; pmgx::WaveRec of csrc/pmg_kernels.h), 64 bytes
WAVE_REC = np.dtype([('t0', '<i8'), ('t1', '<i8'), ('c0', '<i8'), ('c1', '<i8'), ('hw', '<u4'), ('xcc', '<u4'), ('role', '<i4'),
                     ('env', '<i4'), ('nc', '<i4'), ('kernel', '<i4'), ('pad', '<i4', (2,))])
WAVE_ROLES = ('wave0', 'helper', 'packed', 'redo')
PMG_NORM_OBSERVATION = 0
PMG_NORM_POLICY_STATE = 1
PMG_NORM_GOAL = 2


class PmgConfig(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('task', C.c_int32), ('num_envs', C.c_int32), ('num_block', C.c_int32),
                ('binary_reward', C.c_int32), ('joint_control', C.c_int32), ('max_episode_steps', C.c_int32),
                ('device', C.c_int32), ('distance_threshold', C.c_float), ('random_order', C.c_int32),
                ('seed_base', C.c_uint64), ('seed_stride', C.c_uint64), ('env_index_offset', C.c_int32),
                ('task_decomposition', C.c_int32), ('use_curriculum', C.c_int32), ('num_goals_to_generate', C.c_int32),
                ('grip_informed_goal', C.c_int32), ('reserved', C.c_int32 * 3)]


class PmgDims(C.Structure):
    _fields_ = [('num_envs', C.c_int32), ('action_dim', C.c_int32), ('observation_dim', C.c_int32),
                ('policy_state_dim', C.c_int32), ('goal_dim', C.c_int32), ('state_dim', C.c_int32),
                ('packed_dim', C.c_int32), ('reserved', C.c_int32)]


class PmgHerSource(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('num_episodes', C.c_int32), ('episode_steps', C.c_int32), ('reserved', C.c_int32),
                ('d_rows', C.c_void_p), ('row_episode_stride', C.c_int64), ('row_time_stride', C.c_int64),
                ('d_actions', C.c_void_p), ('action_episode_stride', C.c_int64), ('action_time_stride', C.c_int64)]


class PmgHerBatch(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('state_kind', C.c_int32), ('raw', C.c_int32), ('future_p', C.c_float),
                ('seed', C.c_uint64), ('counter', C.c_uint64), ('batch', C.c_int64),
                ('d_x', C.c_void_p), ('d_x_next', C.c_void_p), ('d_action', C.c_void_p), ('d_reward', C.c_void_p),
                ('d_goal_achieved', C.c_void_p), ('d_index', C.c_void_p)]


class PmgMlp(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('num_layers', C.c_int32), ('width', C.c_int32 * 5), ('out_activation', C.c_int32),
                ('d_weight', C.c_void_p * 4), ('d_bias', C.c_void_p * 4)]


class PmgExplore(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('noise_eps', C.c_float), ('random_eps', C.c_float),
                ('seed', C.c_uint64), ('counter', C.c_uint64)]


class PmgTdTarget(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('gamma', C.c_float), ('clip_lo', C.c_float), ('clip_hi', C.c_float),
                ('batch', C.c_int64), ('d_x_next', C.c_void_p), ('x_stride', C.c_int64), ('d_reward', C.c_void_p), ('d_terminal', C.c_void_p),
                ('d_y', C.c_void_p), ('d_q_next', C.c_void_p), ('d_next_action', C.c_void_p)]


class PmgTd3Target(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('gamma', C.c_float), ('clip_lo', C.c_float), ('clip_hi', C.c_float),
                ('sigma', C.c_float), ('noise_clip', C.c_float), ('seed', C.c_uint64), ('counter', C.c_uint64), ('row_offset', C.c_int64),
                ('batch', C.c_int64), ('d_x_next', C.c_void_p), ('x_stride', C.c_int64), ('d_reward', C.c_void_p), ('d_terminal', C.c_void_p),
                ('d_y', C.c_void_p), ('d_q_min', C.c_void_p), ('d_q1', C.c_void_p), ('d_q2', C.c_void_p), ('d_next_action', C.c_void_p),
                ('d_work', C.c_void_p), ('work_floats', C.c_int64)]


class PmgSacSample(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('ls_lo', C.c_float), ('ls_hi', C.c_float), ('sample', C.c_int32), ('reserved2', C.c_int32),
                ('seed', C.c_uint64), ('counter', C.c_uint64), ('row_offset', C.c_int64), ('batch', C.c_int64), ('d_x', C.c_void_p), ('x_stride', C.c_int64),
                ('d_action', C.c_void_p), ('action_stride', C.c_int64), ('d_logp', C.c_void_p), ('d_noise', C.c_void_p), ('noise_stride', C.c_int64),
                ('d_preact', C.c_void_p), ('preact_stride', C.c_int64)]


class PmgSacTarget(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('gamma', C.c_float), ('clip_lo', C.c_float), ('clip_hi', C.c_float), ('alpha', C.c_float),
                ('ls_lo', C.c_float), ('ls_hi', C.c_float), ('sample', C.c_int32), ('reserved2', C.c_int32), ('seed', C.c_uint64), ('counter', C.c_uint64),
                ('row_offset', C.c_int64), ('batch', C.c_int64), ('d_alpha', C.c_void_p), ('d_x_next', C.c_void_p), ('x_stride', C.c_int64),
                ('d_reward', C.c_void_p), ('d_terminal', C.c_void_p), ('d_y', C.c_void_p), ('d_q_min', C.c_void_p), ('d_q1', C.c_void_p), ('d_q2', C.c_void_p),
                ('d_next_action', C.c_void_p), ('d_logp', C.c_void_p), ('d_work', C.c_void_p), ('work_floats', C.c_int64)]


class PmgMlpParams(C.Structure):
    _fields_ = [('d_weight', C.c_void_p * 4), ('d_bias', C.c_void_p * 4)]


class PmgMlpGrad(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('gscale', C.c_float), ('x_dim', C.c_int32), ('a_dim', C.c_int32),
                ('reserved2', C.c_int32), ('batch', C.c_int64), ('d_x', C.c_void_p), ('x_stride', C.c_int64), ('d_a', C.c_void_p), ('a_stride', C.c_int64),
                ('d_gout', C.c_void_p), ('gout_stride', C.c_int64), ('d_target', C.c_void_p), ('target_stride', C.c_int64),
                ('grads', C.POINTER(PmgMlpParams)), ('d_gx', C.c_void_p), ('gx_stride', C.c_int64), ('d_ga', C.c_void_p), ('ga_stride', C.c_int64),
                ('d_out', C.c_void_p), ('out_stride', C.c_int64), ('d_work', C.c_void_p), ('work_floats', C.c_int64)]


class PmgPolicyGrad(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('gscale', C.c_float), ('l2scale', C.c_float), ('batch', C.c_int64),
                ('d_x', C.c_void_p), ('x_stride', C.c_int64), ('grads', C.POINTER(PmgMlpParams)), ('d_action', C.c_void_p), ('action_stride', C.c_int64),
                ('d_out', C.c_void_p), ('out_stride', C.c_int64), ('d_q', C.c_void_p), ('d_gaction', C.c_void_p), ('gaction_stride', C.c_int64),
                ('d_work', C.c_void_p), ('work_floats', C.c_int64)]


class PmgPolicyBc(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('q_filter', C.c_int32), ('bcscale', C.c_float), ('reserved', C.c_int32), ('demo_begin', C.c_int64),
                ('d_demo_action', C.c_void_p), ('demo_action_stride', C.c_int64), ('d_q_demo', C.c_void_p), ('d_filter', C.c_void_p)]


class PmgSacPolicyGrad(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('gscale', C.c_float), ('lscale', C.c_float), ('alpha', C.c_float), ('ls_lo', C.c_float),
                ('ls_hi', C.c_float), ('sample', C.c_int32), ('reserved2', C.c_int32), ('seed', C.c_uint64), ('counter', C.c_uint64), ('row_offset', C.c_int64),
                ('batch', C.c_int64), ('d_alpha', C.c_void_p), ('d_x', C.c_void_p), ('x_stride', C.c_int64), ('grads', C.POINTER(PmgMlpParams)),
                ('d_action', C.c_void_p), ('action_stride', C.c_int64), ('d_logp', C.c_void_p), ('d_q1', C.c_void_p), ('d_q2', C.c_void_p),
                ('d_gaction', C.c_void_p), ('gaction_stride', C.c_int64), ('d_ghead', C.c_void_p), ('ghead_stride', C.c_int64), ('d_work', C.c_void_p),
                ('work_floats', C.c_int64)]


class PmgSacAlpha(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('target_entropy', C.c_float), ('lr', C.c_float), ('beta1', C.c_float), ('beta2', C.c_float),
                ('eps', C.c_float), ('reserved2', C.c_int32), ('step', C.c_int64), ('batch', C.c_int64), ('d_logp', C.c_void_p), ('d_state', C.c_void_p)]


class PmgGae(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('gamma', C.c_float), ('lam', C.c_float), ('steps', C.c_int64), ('envs', C.c_int64)] + \
               [f for name in ('reward', 'value', 'value_next', 'cut', 'terminal', 'adv', 'ret')
                for f in (('d_' + name, C.c_void_p), (name + '_time_stride', C.c_int64), (name + '_env_stride', C.c_int64))]


class PmgAdvStats(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('ddof', C.c_int32), ('eps', C.c_float), ('reserved', C.c_int32), ('count', C.c_int64), ('d_x', C.c_void_p),
                ('d_stats', C.c_void_p)]


class PmgPpoPolicyGrad(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('pscale', C.c_float), ('escale', C.c_float), ('clip_lo', C.c_float), ('clip_hi', C.c_float),
                ('ls_lo', C.c_float), ('ls_hi', C.c_float), ('batch', C.c_int64), ('d_x', C.c_void_p), ('x_stride', C.c_int64), ('d_preact_old', C.c_void_p),
                ('preact_old_stride', C.c_int64), ('d_noise', C.c_void_p), ('noise_stride', C.c_int64), ('d_adv', C.c_void_p), ('grads', C.POINTER(PmgMlpParams)),
                ('d_ratio', C.c_void_p), ('d_logratio', C.c_void_p), ('d_clipped', C.c_void_p), ('d_ghead', C.c_void_p), ('ghead_stride', C.c_int64),
                ('d_work', C.c_void_p), ('work_floats', C.c_int64)]


class PmgPpoStats(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('clip_lo', C.c_float), ('clip_hi', C.c_float), ('batch', C.c_int64), ('d_ratio', C.c_void_p),
                ('d_logratio', C.c_void_p), ('d_clipped', C.c_void_p), ('d_adv', C.c_void_p), ('d_stats', C.c_void_p)]


class PmgAdam(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('lr', C.c_float), ('beta1', C.c_float), ('beta2', C.c_float), ('eps', C.c_float),
                ('step', C.c_int64)]


class PmgError(RuntimeError):
    pass


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class PmgLibrary:
    """A loaded libpmg_hip.so with typed entry points."""

    SYMBOLS = ['pmg_create', 'pmg_destroy', 'pmg_device_count', 'pmg_get_dims', 'pmg_last_error', 'pmg_seed', 'pmg_reset', 'pmg_step',
               'pmg_reset_device', 'pmg_reset_done_device', 'pmg_step_device', 'pmg_device_ptr', 'pmg_stream', 'pmg_sync', 'pmg_read_outputs',
               'pmg_compute_reward', 'pmg_compute_reward_device', 'pmg_get_state', 'pmg_set_state', 'pmg_set_goal',
               'pmg_comm_unique_id', 'pmg_comm_init', 'pmg_allgather_packed', 'pmg_comm_overlap', 'pmg_allgather_packed_async', 'pmg_allgather_wait', 'pmg_timing_reset', 'pmg_timing_every', 'pmg_timing_read',
               'pmg_device_alloc', 'pmg_device_free', 'pmg_upload', 'pmg_download',
               'pmg_set_sub_goal', 'pmg_curriculum_update', 'pmg_curriculum_read', 'pmg_timing_stats', 'pmg_get_rng', 'pmg_set_rng', 'pmg_comm_timing',
               'pmg_norm_configure', 'pmg_norm_update_device', 'pmg_norm_update', 'pmg_norm_update_env_device', 'pmg_norm_read',
               'pmg_norm_write', 'pmg_policy_input_device', 'pmg_policy_input', 'pmg_policy_input_env_device',
               'pmg_her_sample_device', 'pmg_device_copy', 'pmg_mlp_forward_device', 'pmg_act_env_device', 'pmg_q_device', 'pmg_td_target_device',
               'pmg_mlp_grad_work_floats', 'pmg_mlp_grad_device', 'pmg_mlp_adam_device', 'pmg_mlp_polyak_device',
               'pmg_mlp_grad_chunked_work_floats', 'pmg_mlp_grad_chunked_device', 'pmg_policy_grad_work_floats', 'pmg_policy_grad_device',
               'pmg_policy_grad_bc_device',
               'pmg_td3_target_work_floats', 'pmg_td3_target_device',
               'pmg_sac_sample_device', 'pmg_sac_act_env_device', 'pmg_sac_target_work_floats', 'pmg_sac_target_device',
               'pmg_sac_policy_grad_work_floats', 'pmg_sac_policy_grad_device', 'pmg_sac_alpha_device',
               'pmg_gae_device', 'pmg_adv_stats_device', 'pmg_adv_apply_device', 'pmg_ppo_policy_grad_work_floats', 'pmg_ppo_policy_grad_device',
               'pmg_ppo_stats_device',
               'pmg_comm_info', 'pmg_allgather_device', 'pmg_mlp_param_floats', 'pmg_mlp_params_pack_device', 'pmg_mlp_params_merge_device',
               'pmg_mlp_adam_merge_device', 'pmg_mlp_allreduce_work_floats', 'pmg_mlp_grad_allreduce_device', 'pmg_mlp_adam_allreduce_device',
               'pmg_norm_update_ranks_device', 'pmg_norm_update_env_ranks_device']

    def device_count(self):
        return int(self.lib.pmg_device_count())

    def __init__(self, path=None):
        self.path = path or DEFAULT_LIBRARY
        if not os.path.exists(self.path):
            raise PmgError('%s not found: the HIP extension is not built (run `python -c "import __graft_entry__ as g; '
                           'g.build()"` or `make -C pybullet_multigoal_gym_amd/csrc`). There is no CPU fallback.' % self.path)
        self.lib = C.CDLL(self.path)
        L = self.lib
        for s in self.SYMBOLS:
            getattr(L, s)  # raises AttributeError if the ABI is incomplete
        L.pmg_last_error.restype = C.c_char_p
        L.pmg_last_error.argtypes = [C.c_void_p]
        L.pmg_destroy.restype = None
        L.pmg_destroy.argtypes = [C.c_void_p]
        for name in self.SYMBOLS:
            if name not in ('pmg_last_error', 'pmg_destroy'):
                getattr(L, name).restype = C.c_int
        L.pmg_mlp_grad_work_floats.restype = C.c_int64
        L.pmg_mlp_grad_chunked_work_floats.restype = C.c_int64
        L.pmg_policy_grad_work_floats.restype = C.c_int64
        L.pmg_td3_target_work_floats.restype = C.c_int64
        L.pmg_sac_target_work_floats.restype = C.c_int64
        L.pmg_sac_policy_grad_work_floats.restype = C.c_int64
        L.pmg_ppo_policy_grad_work_floats.restype = C.c_int64
        L.pmg_mlp_param_floats.restype = C.c_int64
        L.pmg_mlp_allreduce_work_floats.restype = C.c_int64

    def error(self, handle=None):
        msg = self.lib.pmg_last_error(handle)
        return msg.decode() if msg else ''


_default = None


def default_library():
    global _default
    if _default is None:
        _default = PmgLibrary()
    return _default


class PmgHandle:
    """One pmg_env handle (N envs on one GPU)."""

    def __init__(self, library, **cfg_kw):
        self.L = library
        cfg = PmgConfig()
        cfg.struct_size = C.sizeof(PmgConfig)
        for k, v in cfg_kw.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = library.lib.pmg_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise PmgError('pmg_create failed (%d): %s' % (rc, library.error(None)))
        self.dims = PmgDims()
        self._check(library.lib.pmg_get_dims(self.h, C.byref(self.dims)))
        self.N = self.dims.num_envs

    def _check(self, rc):
        if rc != 0:
            raise PmgError('pmg call failed (%d): %s' % (rc, self.L.error(self.h)))

    def close(self):
        if getattr(self, 'h', None):
            self.L.lib.pmg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-buffer calls -------------------------------------------------
    def _obs_bufs(self):
        d, N = self.dims, self.N
        return (np.empty((N, d.observation_dim), np.float32), np.empty((N, d.policy_state_dim), np.float32),
                np.empty((N, d.goal_dim), np.float32), np.empty((N, d.goal_dim), np.float32))

    def seed(self, base, stride):
        self._check(self.L.lib.pmg_seed(self.h, C.c_uint64(base), C.c_uint64(stride)))

    def reset(self, mask=None):
        o, p, a, g = self._obs_bufs()
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.N)
        self._check(self.L.lib.pmg_reset(self.h, _p(m), _p(o), _p(p), _p(a), _p(g)))
        return o, p, a, g

    def step(self, actions):
        o, p, a, g = self._obs_bufs()
        r = np.empty(self.N, np.float32)
        ok = np.empty(self.N, np.uint8)
        dn = np.empty(self.N, np.uint8)
        self._check(self.L.lib.pmg_step(self.h, _p(actions), _p(o), _p(p), _p(a), _p(g), _p(r), _p(ok), _p(dn)))
        return o, p, a, g, r, ok.astype(np.bool_), dn.astype(np.bool_)

    def read_outputs(self):
        o, p, a, g = self._obs_bufs()
        r = np.empty(self.N, np.float32)
        ok = np.empty(self.N, np.uint8)
        dn = np.empty(self.N, np.uint8)
        self._check(self.L.lib.pmg_read_outputs(self.h, _p(o), _p(p), _p(a), _p(g), _p(r), _p(ok), _p(dn)))
        return o, p, a, g, r, ok.astype(np.bool_), dn.astype(np.bool_)

    def compute_reward(self, ag, dg):
        G = self.dims.goal_dim
        ag = np.ascontiguousarray(ag, np.float32)
        dg = np.ascontiguousarray(dg, np.float32)
        if ag.shape != dg.shape or ag.shape[-1] != G:
            raise ValueError('achieved_goal %s / desired_goal %s must share a shape ending in %d' % (ag.shape, dg.shape, G))
        B = ag.size // G
        r = np.empty(B, np.float32)
        ok = np.empty(B, np.uint8)
        self._check(self.L.lib.pmg_compute_reward(self.h, _p(ag), _p(dg), C.c_int64(B), _p(r), _p(ok)))
        return r.reshape(ag.shape[:-1]), ok.astype(np.bool_).reshape(ag.shape[:-1])

    def get_state(self):
        s = np.empty((self.N, self.dims.state_dim), np.float32)
        self._check(self.L.lib.pmg_get_state(self.h, _p(s)))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, np.float32)
        if s.shape != (self.N, self.dims.state_dim):
            raise ValueError('state must have shape %s' % ((self.N, self.dims.state_dim),))
        self._check(self.L.lib.pmg_set_state(self.h, _p(s)))

    def set_goal(self, goals, mask=None):
        goals = np.ascontiguousarray(goals, np.float32).reshape(self.N, self.dims.goal_dim)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.N)
        self._check(self.L.lib.pmg_set_goal(self.h, _p(m), _p(goals)))

    # -- multi-step task bookkeeping ----------------------------------------
    def set_sub_goal(self, sub_goal_ind, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.N)
        self._check(self.L.lib.pmg_set_sub_goal(self.h, _p(m), C.c_int32(int(sub_goal_ind))))

    def curriculum_update(self, enabled):
        self._check(self.L.lib.pmg_curriculum_update(self.h, C.c_int32(int(bool(enabled)))))

    def curriculum_read(self):
        nb = self.cfg.num_block + (1 if self.cfg.task in (TASK_IDS['chest_push'], TASK_IDS['chest_pick_and_place']) else 0)
        level, goal_step = np.empty(self.N, np.int32), np.empty(self.N, np.int32)
        prob, generated = np.empty((self.N, nb), np.float32), np.empty((self.N, nb), np.float32)
        self._check(self.L.lib.pmg_curriculum_read(self.h, _p(level), _p(goal_step), _p(prob), _p(generated)))
        return level, goal_step, prob, generated

    # -- device-resident calls --------------------------------------------
    def step_device(self, d_actions_ptr):
        self._check(self.L.lib.pmg_step_device(self.h, C.c_void_p(d_actions_ptr)))

    def reset_device(self, d_mask_ptr=None):
        self._check(self.L.lib.pmg_reset_device(self.h, C.c_void_p(d_mask_ptr) if d_mask_ptr else None))

    def reset_done_device(self):
        """Reset, on the device, the envs whose episode has ended (TimeLimit); no host mask (include/pmg.h)."""
        self._check(self.L.lib.pmg_reset_done_device(self.h))

    def device_ptr(self, which=PMG_BUF_PACKED):
        p = C.c_void_p()
        self._check(self.L.lib.pmg_device_ptr(self.h, C.c_int(which), C.byref(p)))
        return p.value

    def schedule(self):
        """Launch schedule of the last step (diagnostics): dict(prone=[...], free=[...], redo=[...]) of env indices."""
        n = self.N   # the one Python mirror of the layout that csrc/pmg_sched.h (pmgx::Sched) defines: counts, list 0, list 1, redo count, redo list
        buf = np.empty(3 + 3 * n, np.int32)
        self.sync()
        self.download(buf, self.device_ptr(PMG_BUF_SCHED))
        return {'prone': buf[2:2 + buf[0]].copy(), 'free': buf[2 + n:2 + n + buf[1]].copy(),
                'redo': buf[3 + 2 * n:3 + 2 * n + buf[2 + 2 * n]].copy()}

    def env_cycles(self):
        """Per-env cost of the last step (diagnostics; the handle must have been created with PMG_ENV_CYCLES=1 in the
        environment): [N, 2] int32 = shader cycles / 64 of the env's wavefront, largest contact count of a substep."""
        buf = np.empty((self.N, 2), np.int32)
        self.sync()
        self.download(buf, self.device_ptr(PMG_BUF_ENV_CYCLES))
        return buf

    def wave_trace(self):
        """Per-wavefront records of the last reach step (diagnostics; the handle must have been created with PMG_WAVE_TRACE=1 in the
        environment): [2 N] WAVE_REC; a record no wavefront wrote is all 0xFF bytes (role == -1)."""
        buf = np.empty(2 * self.N, WAVE_REC)
        self.sync()
        self.download(buf, self.device_ptr(PMG_BUF_WAVE_TRACE))
        return buf

    def stream(self):
        p = C.c_void_p()
        self._check(self.L.lib.pmg_stream(self.h, C.byref(p)))
        return p.value

    def sync(self):
        self._check(self.L.lib.pmg_sync(self.h))

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._check(self.L.lib.pmg_device_alloc(self.h, C.c_uint64(nbytes), C.byref(p)))
        return p.value

    def device_free(self, ptr):
        self._check(self.L.lib.pmg_device_free(self.h, C.c_void_p(ptr)))

    def upload(self, d_ptr, array):
        a = np.ascontiguousarray(array)
        self._check(self.L.lib.pmg_upload(self.h, C.c_void_p(d_ptr), _p(a), C.c_uint64(a.nbytes)))

    def download(self, array, d_ptr):
        assert array.flags['C_CONTIGUOUS']
        self._check(self.L.lib.pmg_download(self.h, _p(array), C.c_void_p(d_ptr), C.c_uint64(array.nbytes)))

    def device_copy(self, d_dst_ptr, d_src_ptr, nbytes):
        """Device to device on the handle's stream, no host sync (how a rollout records PMG_BUF_PACKED rows for her_sample_device)."""
        self._check(self.L.lib.pmg_device_copy(self.h, C.c_void_p(d_dst_ptr), C.c_void_p(d_src_ptr), C.c_uint64(nbytes)))

    # -- HER minibatches from caller-owned episode rows (include/pmg.h) --
    def her_structs(self, d_rows, num_episodes, episode_steps, row_episode_stride, row_time_stride, batch, d_actions=None,
                    action_episode_stride=0, action_time_stride=0, state_kind=PMG_NORM_POLICY_STATE, raw=False, future_p=0.8,
                    seed=0, counter=0, d_x=None, d_x_next=None, d_action=None, d_reward=None, d_goal_achieved=None, d_index=None):
        """The two argument structs of pmg_her_sample_device (pointers as integers or None)."""
        src = PmgHerSource(C.sizeof(PmgHerSource), num_episodes, episode_steps, 0, d_rows, row_episode_stride, row_time_stride,
                           d_actions, action_episode_stride, action_time_stride)
        out = PmgHerBatch(C.sizeof(PmgHerBatch), state_kind, int(bool(raw)), future_p, seed & (2 ** 64 - 1), counter & (2 ** 64 - 1), batch,
                          d_x, d_x_next, d_action, d_reward, d_goal_achieved, d_index)
        return src, out

    def her_sample_device(self, *args, **kw):
        """pmg_her_sample_device with the arguments of her_structs(); stream-ordered, no host sync."""
        src, out = self.her_structs(*args, **kw)
        self._check(self.L.lib.pmg_her_sample_device(self.h, C.byref(src), C.byref(out)))

    # -- actor forward + exploration (include/pmg.h) --
    @staticmethod
    def mlp_struct(widths, d_weights, d_biases=None, out_activation=1):
        """pmg_mlp of a network widths[0] -> ... -> widths[L] from device pointers (integers; a bias may be None)."""
        L = len(widths) - 1
        if not 1 <= L <= 4 or len(d_weights) != L or (d_biases is not None and len(d_biases) != L):
            raise ValueError('a network has 1..4 layers, one weight (and one bias or None) per layer')
        m = PmgMlp()
        m.struct_size, m.num_layers, m.out_activation = C.sizeof(PmgMlp), L, int(out_activation)
        for l, w in enumerate(widths):
            m.width[l] = int(w)
        for l in range(L):
            m.d_weight[l] = d_weights[l]
            m.d_bias[l] = None if d_biases is None else d_biases[l]
        return m

    @staticmethod
    def explore_struct(noise_eps=0.0, random_eps=0.0, seed=0, counter=0):
        return PmgExplore(C.sizeof(PmgExplore), 0, noise_eps, random_eps, seed & (2 ** 64 - 1), counter & (2 ** 64 - 1))

    def mlp_forward_device(self, mlp, d_in_ptr, in_stride, batch, d_out_ptr, out_stride):
        """d_out [batch, width[L]] = the network on the rows d_in [batch, width[0]]; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_forward_device(self.h, C.byref(mlp), C.c_void_p(d_in_ptr), C.c_int64(in_stride), C.c_int64(batch),
                                                      C.c_void_p(d_out_ptr), C.c_int64(out_stride)))

    def act_env_device(self, mlp, state_kind, d_actions_ptr, d_preact_ptr=None, explore=None):
        """Actions [N, action_dim] of the rows of the last step / reset (what step_device takes); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_act_env_device(self.h, C.byref(mlp), C.c_int(state_kind), C.byref(explore) if explore is not None else None,
                                                  C.c_void_p(d_actions_ptr), C.c_void_p(d_preact_ptr) if d_preact_ptr else None))

    # -- critic and TD target (include/pmg.h) --
    @staticmethod
    def td_struct(batch, d_x_next, x_stride, d_reward, d_y, gamma, clip_lo=-float('inf'), clip_hi=float('inf'), d_terminal=None, d_q_next=None,
                  d_next_action=None):
        """pmg_td_target from device pointers (integers or None)."""
        return PmgTdTarget(C.sizeof(PmgTdTarget), 0, gamma, clip_lo, clip_hi, batch, d_x_next, x_stride, d_reward, d_terminal, d_y, d_q_next,
                           d_next_action)

    def q_device(self, critic, d_x_ptr, x_stride, x_dim, d_a_ptr, a_stride, a_dim, batch, d_q_ptr, q_stride=1):
        """d_q [batch] = the critic on the rows x[b] | a[b] of two tables read in place; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_q_device(self.h, C.byref(critic), C.c_void_p(d_x_ptr), C.c_int64(x_stride), C.c_int32(x_dim), C.c_void_p(d_a_ptr),
                                            C.c_int64(a_stride), C.c_int32(a_dim), C.c_int64(batch), C.c_void_p(d_q_ptr), C.c_int64(q_stride)))

    def td_target_device(self, actor_target, critic_target, td):
        """y = clip(r + gamma Q'(x', pi'(x'))) of a td_struct(); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_td_target_device(self.h, C.byref(actor_target), C.byref(critic_target), C.byref(td)))

    # -- TD3's target: twin critics and target-policy smoothing (include/pmg.h) --
    @staticmethod
    def td3_struct(batch, d_x_next, x_stride, d_reward, d_y, gamma, clip_lo=-float('inf'), clip_hi=float('inf'), sigma=0.0, noise_clip=float('inf'),
                   seed=0, counter=0, row_offset=0, d_terminal=None, d_q_min=None, d_q1=None, d_q2=None, d_next_action=None, d_work=None, work_floats=0):
        """pmg_td3_target from device pointers (integers or None)."""
        return PmgTd3Target(C.sizeof(PmgTd3Target), 0, gamma, clip_lo, clip_hi, sigma, noise_clip, seed & (2 ** 64 - 1), counter & (2 ** 64 - 1),
                            row_offset, batch, d_x_next, x_stride, d_reward, d_terminal, d_y, d_q_min, d_q1, d_q2, d_next_action, d_work, work_floats)

    def td3_target_work_floats(self, actor_target, has_critic2, has_next_action, batch):
        """floats of workspace pmg_td3_target_device needs: batch * A with a second critic and no d_next_action, else 0 (< 0: invalid)"""
        return int(self.L.lib.pmg_td3_target_work_floats(C.byref(actor_target), C.c_int(bool(has_critic2)), C.c_int(bool(has_next_action)), C.c_int64(batch)))

    def td3_target_device(self, actor_target, critic1_target, critic2_target, td):
        """y = clip(r + gamma min(Q1', Q2')(x', smoothed pi'(x'))) of a td3_struct(); critic2_target may be None; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_td3_target_device(self.h, C.byref(actor_target), C.byref(critic1_target),
                                                     C.byref(critic2_target) if critic2_target is not None else None, C.byref(td)))

    # -- SAC: the Gaussian head and the soft target (include/pmg.h) --
    @staticmethod
    def sac_sample_struct(batch, d_x, x_stride, d_action=None, action_stride=0, d_logp=None, d_noise=None, noise_stride=0, d_preact=None, preact_stride=0,
                          ls_lo=-20.0, ls_hi=2.0, sample=1, seed=0, counter=0, row_offset=0):
        """pmg_sac_sample from device pointers (integers or None); pmg_sac_act_env_device does not read batch, d_x, x_stride and row_offset."""
        return PmgSacSample(C.sizeof(PmgSacSample), 0, ls_lo, ls_hi, int(bool(sample)), 0, seed & (2 ** 64 - 1), counter & (2 ** 64 - 1), row_offset, batch,
                            d_x, x_stride, d_action, action_stride, d_logp, d_noise, noise_stride, d_preact, preact_stride)

    def sac_sample_device(self, actor, s):
        """action, log-probability, noise and pre-activations of a Gaussian actor on the rows of a sac_sample_struct(); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_sac_sample_device(self.h, C.byref(actor), C.byref(s)))

    def sac_act_env_device(self, actor, state_kind, s):
        """the same on the rows of the last step / reset (the outputs and the head's settings of a sac_sample_struct()); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_sac_act_env_device(self.h, C.byref(actor), C.c_int(state_kind), C.byref(s)))

    @staticmethod
    def sac_target_struct(batch, d_x_next, x_stride, d_reward, d_y, gamma, clip_lo=-float('inf'), clip_hi=float('inf'), alpha=0.0, ls_lo=-20.0, ls_hi=2.0,
                          sample=1, seed=0, counter=0, row_offset=0, d_alpha=None, d_terminal=None, d_q_min=None, d_q1=None, d_q2=None, d_next_action=None,
                          d_logp=None, d_work=None, work_floats=0):
        """pmg_sac_target from device pointers (integers or None)."""
        return PmgSacTarget(C.sizeof(PmgSacTarget), 0, gamma, clip_lo, clip_hi, alpha, ls_lo, ls_hi, int(bool(sample)), 0, seed & (2 ** 64 - 1),
                            counter & (2 ** 64 - 1), row_offset, batch, d_alpha, d_x_next, x_stride, d_reward, d_terminal, d_y, d_q_min, d_q1, d_q2,
                            d_next_action, d_logp, d_work, work_floats)

    def sac_target_work_floats(self, actor, has_next_action, batch):
        """floats of workspace pmg_sac_target_device needs: batch * A without d_next_action, else 0 (< 0: invalid)"""
        return int(self.L.lib.pmg_sac_target_work_floats(C.byref(actor), C.c_int(bool(has_next_action)), C.c_int64(batch)))

    def sac_target_device(self, actor, critic1_target, critic2_target, td):
        """y = clip(r + gamma (min(Q1', Q2')(x', a') - alpha log pi(a' | x'))) of a sac_target_struct(); critic2_target may be None; stream-ordered, no
        host sync."""
        self._check(self.L.lib.pmg_sac_target_device(self.h, C.byref(actor), C.byref(critic1_target),
                                                     C.byref(critic2_target) if critic2_target is not None else None, C.byref(td)))

    # -- SAC: the actor's half in one call and the temperature step (include/pmg.h) --
    @staticmethod
    def sac_policy_grad_struct(batch, d_x, x_stride, d_work, work_floats, gscale, lscale, alpha=0.0, ls_lo=-20.0, ls_hi=2.0, sample=1, seed=0, counter=0,
                               row_offset=0, d_alpha=None, grads=None, d_action=None, action_stride=0, d_logp=None, d_q1=None, d_q2=None, d_gaction=None,
                               gaction_stride=0, d_ghead=None, ghead_stride=0):
        """pmg_sac_policy_grad from device pointers (integers or None); grads: a params_struct() or None (it must outlive the call)."""
        return PmgSacPolicyGrad(C.sizeof(PmgSacPolicyGrad), 0, gscale, lscale, alpha, ls_lo, ls_hi, int(bool(sample)), 0, seed & (2 ** 64 - 1),
                                counter & (2 ** 64 - 1), row_offset, batch, d_alpha, d_x, x_stride, C.pointer(grads) if grads is not None else None,
                                d_action, action_stride, d_logp, d_q1, d_q2, d_gaction, gaction_stride, d_ghead, ghead_stride, d_work, work_floats)

    def sac_policy_grad_work_floats(self, actor, has_action, has_critic2, batch, chunk_rows=0):
        """floats of workspace pmg_sac_policy_grad_device needs: the actor's gradient figure, + batch * A without d_action, + batch * A with a second
        critic (< 0: invalid)"""
        return int(self.L.lib.pmg_sac_policy_grad_work_floats(C.byref(actor), C.c_int(bool(has_action)), C.c_int(bool(has_critic2)), C.c_int64(batch),
                                                              C.c_int64(chunk_rows)))

    def sac_policy_grad_device(self, actor, critic1, critic2, grad, chunk_rows=0):
        """the Gaussian actor's gradient of lscale alpha sum log pi + gscale sum min(Q1, Q2) of a sac_policy_grad_struct(); critic2 may be None;
        stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_sac_policy_grad_device(self.h, C.byref(actor), C.byref(critic1), C.byref(critic2) if critic2 is not None else None,
                                                          C.byref(grad), C.c_int64(chunk_rows)))

    @staticmethod
    def sac_alpha_struct(batch, d_logp, d_state, target_entropy, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
        """pmg_sac_alpha from device pointers; d_state: four floats, log_alpha | m | v | alpha."""
        return PmgSacAlpha(C.sizeof(PmgSacAlpha), 0, target_entropy, lr, beta1, beta2, eps, 0, step, batch, d_logp, d_state)

    def sac_alpha_device(self, a):
        """one Adam step on the log-temperature of a sac_alpha_struct(), then alpha = exp(log_alpha); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_sac_alpha_device(self.h, C.byref(a)))

    # -- PPO on whole rollouts: GAE, the advantage normaliser, the clipped-surrogate gradient, the statistics (include/pmg.h) --
    @staticmethod
    def gae_struct(steps, envs, gamma, lam, reward, value, value_next, adv, cut=None, terminal=None, ret=None):
        """pmg_gae; every table is (device pointer, time_stride, env_stride) in floats, or None where the call allows it."""
        g = PmgGae()
        g.struct_size, g.gamma, g.lam, g.steps, g.envs = C.sizeof(PmgGae), gamma, lam, steps, envs
        for name, tab in (('reward', reward), ('value', value), ('value_next', value_next), ('cut', cut), ('terminal', terminal), ('adv', adv), ('ret', ret)):
            if tab is not None:
                setattr(g, 'd_' + name, tab[0])
                setattr(g, name + '_time_stride', tab[1])
                setattr(g, name + '_env_stride', tab[2])
        return g

    def gae_device(self, g):
        """advantages (and returns) of a gae_struct(): one reverse chain per env; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_gae_device(self.h, C.byref(g)))

    @staticmethod
    def adv_stats_struct(count, d_x, d_stats, eps=1e-8, ddof=0):
        """pmg_adv_stats from device pointers; d_stats: two floats, mean | 1 / (std + eps)."""
        return PmgAdvStats(C.sizeof(PmgAdvStats), int(ddof), eps, 0, count, d_x, d_stats)

    def adv_stats_device(self, s):
        """mean and 1 / (std + eps) of the floats of an adv_stats_struct() into device memory; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_adv_stats_device(self.h, C.byref(s)))

    def adv_apply_device(self, d_x_ptr, count, d_stats_ptr, d_y_ptr):
        """y = (x - stats[0]) * stats[1] with the statistics read on the stream; d_y may be d_x; no host sync."""
        self._check(self.L.lib.pmg_adv_apply_device(self.h, C.c_void_p(d_x_ptr), C.c_int64(count), C.c_void_p(d_stats_ptr), C.c_void_p(d_y_ptr)))

    @staticmethod
    def ppo_policy_grad_struct(batch, d_x, x_stride, d_preact_old, preact_old_stride, d_noise, noise_stride, d_adv, pscale, escale, clip_lo, clip_hi,
                               ls_lo=-20.0, ls_hi=2.0, grads=None, d_ratio=None, d_logratio=None, d_clipped=None, d_ghead=None, ghead_stride=0, d_work=None,
                               work_floats=0):
        """pmg_ppo_policy_grad from device pointers (integers or None); grads: a params_struct() or None (it must outlive the call)."""
        return PmgPpoPolicyGrad(C.sizeof(PmgPpoPolicyGrad), 0, pscale, escale, clip_lo, clip_hi, ls_lo, ls_hi, batch, d_x, x_stride, d_preact_old,
                                preact_old_stride, d_noise, noise_stride, d_adv, C.pointer(grads) if grads is not None else None, d_ratio, d_logratio,
                                d_clipped, d_ghead, ghead_stride, d_work, work_floats)

    def ppo_policy_grad_work_floats(self, actor, batch, chunk_rows=0):
        """floats of workspace pmg_ppo_policy_grad_device needs with grads: the actor's gradient figure (< 0: invalid)"""
        return int(self.L.lib.pmg_ppo_policy_grad_work_floats(C.byref(actor), C.c_int64(batch), C.c_int64(chunk_rows)))

    def ppo_policy_grad_device(self, actor, grad, chunk_rows=0):
        """the Gaussian actor's gradient of PPO's clipped surrogate and entropy bonus of a ppo_policy_grad_struct(); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_ppo_policy_grad_device(self.h, C.byref(actor), C.byref(grad), C.c_int64(chunk_rows)))

    @staticmethod
    def ppo_stats_struct(batch, d_ratio, d_logratio, d_clipped, d_adv, d_stats, clip_lo, clip_hi):
        """pmg_ppo_stats from device pointers; d_stats: four floats, approximate KL | clip fraction | clipped surrogate | mean log-ratio."""
        return PmgPpoStats(C.sizeof(PmgPpoStats), 0, clip_lo, clip_hi, batch, d_ratio, d_logratio, d_clipped, d_adv, d_stats)

    def ppo_stats_device(self, s):
        """the four means of a ppo_stats_struct() into device memory; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_ppo_stats_device(self.h, C.byref(s)))

    # -- back-propagation, Adam, Polyak (include/pmg.h) --
    @staticmethod
    def params_struct(d_weights, d_biases=None):
        """pmg_mlp_params from device pointers (integers; a bias may be None)."""
        p = PmgMlpParams()
        for l, w in enumerate(d_weights):
            p.d_weight[l] = w
            p.d_bias[l] = None if d_biases is None else d_biases[l]
        return p

    @staticmethod
    def grad_struct(batch, d_x, x_stride, x_dim, d_work, work_floats, d_a=None, a_stride=0, a_dim=0, d_gout=None, gout_stride=0, d_target=None,
                    target_stride=0, gscale=1.0, grads=None, d_gx=None, gx_stride=0, d_ga=None, ga_stride=0, d_out=None, out_stride=0):
        """pmg_mlp_grad from device pointers (integers or None); grads: a params_struct() or None (it must outlive the call)."""
        return PmgMlpGrad(C.sizeof(PmgMlpGrad), 0, gscale, x_dim, a_dim, 0, batch, d_x, x_stride, d_a, a_stride, d_gout, gout_stride, d_target,
                          target_stride, C.pointer(grads) if grads is not None else None, d_gx, gx_stride, d_ga, ga_stride, d_out, out_stride,
                          d_work, work_floats)

    @staticmethod
    def adam_struct(lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
        return PmgAdam(C.sizeof(PmgAdam), 0, lr, beta1, beta2, eps, step)

    def mlp_grad_work_floats(self, mlp, batch):
        """floats of workspace pmg_mlp_grad_device needs for `batch` rows (< 0: invalid network / batch)"""
        return int(self.L.lib.pmg_mlp_grad_work_floats(C.byref(mlp), C.c_int64(batch)))

    def mlp_grad_device(self, mlp, grad):
        """forward with saved activations, then backward, of a grad_struct(); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_grad_device(self.h, C.byref(mlp), C.byref(grad)))

    def mlp_grad_chunked_work_floats(self, mlp, batch, chunk_rows):
        """floats of workspace pmg_mlp_grad_chunked_device needs for `batch` rows in chunks of `chunk_rows` (< 0: invalid)"""
        return int(self.L.lib.pmg_mlp_grad_chunked_work_floats(C.byref(mlp), C.c_int64(batch), C.c_int64(chunk_rows)))

    def mlp_grad_chunked_device(self, mlp, grad, chunk_rows):
        """mlp_grad_device with dW / db reduced over chunks of `chunk_rows` rows (even, >= 2); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_grad_chunked_device(self.h, C.byref(mlp), C.byref(grad), C.c_int64(chunk_rows)))

    @staticmethod
    def policy_grad_struct(batch, d_x, x_stride, d_work, work_floats, gscale, l2scale=0.0, grads=None, d_action=None, action_stride=0, d_out=None,
                           out_stride=0, d_q=None, d_gaction=None, gaction_stride=0):
        """pmg_policy_grad from device pointers (integers or None); grads: a params_struct() or None (it must outlive the call)."""
        return PmgPolicyGrad(C.sizeof(PmgPolicyGrad), 0, gscale, l2scale, batch, d_x, x_stride, C.pointer(grads) if grads is not None else None,
                             d_action, action_stride, d_out, out_stride, d_q, d_gaction, gaction_stride, d_work, work_floats)

    def policy_grad_work_floats(self, actor, critic, batch, chunk_rows=0):
        """floats of workspace pmg_policy_grad_device needs (chunk_rows 0: one chain over the batch; < 0: invalid)"""
        return int(self.L.lib.pmg_policy_grad_work_floats(C.byref(actor), C.byref(critic), C.c_int64(batch), C.c_int64(chunk_rows)))

    def policy_grad_device(self, actor, critic, grad, chunk_rows=0):
        """the actor's gradient through the critic, L2 and clip terms included, of a policy_grad_struct(); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_policy_grad_device(self.h, C.byref(actor), C.byref(critic), C.byref(grad), C.c_int64(chunk_rows)))

    @staticmethod
    def policy_bc_struct(demo_begin, d_demo_action, demo_action_stride, bcscale, q_filter=1, d_q_demo=None, d_filter=None):
        """pmg_policy_bc from device pointers (integers or None): rows from demo_begin on are demonstrations with the actions d_demo_action [B, A]."""
        return PmgPolicyBc(C.sizeof(PmgPolicyBc), int(q_filter), bcscale, 0, demo_begin, d_demo_action, demo_action_stride, d_q_demo, d_filter)

    def policy_grad_bc_device(self, actor, critic, grad, bc, chunk_rows=0):
        """policy_grad_device with the behaviour-cloning term of a policy_bc_struct() on the demonstration rows; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_policy_grad_bc_device(self.h, C.byref(actor), C.byref(critic), C.byref(grad), C.byref(bc), C.c_int64(chunk_rows)))

    def mlp_adam_device(self, shape, param, grad, m, v, adam):
        """one Adam step on the tensors of `param` (params_struct()s, adam_struct()); stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_adam_device(self.h, C.byref(shape), C.byref(param), C.byref(grad), C.byref(m), C.byref(v), C.byref(adam)))

    def mlp_polyak_device(self, source, target, tau):
        """target = fmaf(tau, source - target, target) per parameter; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_polyak_device(self.h, C.byref(source), C.byref(target), C.c_float(tau)))

    # -- data-parallel learner: rank-ordered gradient and normaliser merge (include/pmg.h) --
    def comm_info(self):
        """(rank, nranks) of comm_init(); PmgError before it"""
        rank, nranks = C.c_int32(), C.c_int32()
        self._check(self.L.lib.pmg_comm_info(self.h, C.byref(rank), C.byref(nranks)))
        return rank.value, nranks.value

    def allgather_device(self, d_src_ptr, count, d_gathered_ptr):
        """count floats of every rank into d_gathered [nranks * count], rank order; a collective, stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_allgather_device(self.h, C.c_void_p(d_src_ptr), C.c_int64(count), C.c_void_p(d_gathered_ptr)))

    def mlp_param_floats(self, shape):
        """P: the floats of a network's tensors in their flat order, weight 0, bias 0, weight 1, ... (< 0: invalid network)"""
        return int(self.L.lib.pmg_mlp_param_floats(C.byref(shape)))

    def mlp_params_pack_device(self, shape, src, d_flat_ptr):
        """the tensors of `src` (a params_struct()) into one flat run of P floats; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_params_pack_device(self.h, C.byref(shape), C.byref(src), C.c_void_p(d_flat_ptr)))

    def mlp_params_merge_device(self, shape, d_slots_ptr, slot_stride, nslots, out):
        """out = the flat slots at d_slots + r * slot_stride added in ascending r, in float32; stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_params_merge_device(self.h, C.byref(shape), C.c_void_p(d_slots_ptr), C.c_int64(slot_stride), C.c_int64(nslots),
                                                           C.byref(out)))

    def mlp_adam_merge_device(self, shape, param, d_slots_ptr, slot_stride, nslots, grad_out, m, v, adam):
        """the same sum handed to mlp_adam_device's step in one sweep; grad_out: a params_struct() that receives the sum, or None."""
        self._check(self.L.lib.pmg_mlp_adam_merge_device(self.h, C.byref(shape), C.byref(param), C.c_void_p(d_slots_ptr), C.c_int64(slot_stride),
                                                         C.c_int64(nslots), C.byref(grad_out) if grad_out is not None else None, C.byref(m), C.byref(v),
                                                         C.byref(adam)))

    def mlp_allreduce_work_floats(self, shape):
        """floats of workspace the two all-reduce calls need: (nranks + 1) * P (< 0: invalid network)"""
        return int(self.L.lib.pmg_mlp_allreduce_work_floats(self.h, C.byref(shape)))

    def mlp_grad_allreduce_device(self, shape, grads, d_work_ptr, work_floats):
        """grads = the ranks' grads added in rank order, in place; a collective, stream-ordered, no host sync."""
        self._check(self.L.lib.pmg_mlp_grad_allreduce_device(self.h, C.byref(shape), C.byref(grads), C.c_void_p(d_work_ptr), C.c_int64(work_floats)))

    def mlp_adam_allreduce_device(self, shape, param, grads, m, v, adam, d_work_ptr, work_floats):
        """one Adam step on `param` with the ranks' grads added in rank order; grads keeps this rank's own; a collective, no host sync."""
        self._check(self.L.lib.pmg_mlp_adam_allreduce_device(self.h, C.byref(shape), C.byref(param), C.byref(grads), C.byref(m), C.byref(v), C.byref(adam),
                                                             C.c_void_p(d_work_ptr), C.c_int64(work_floats)))

    def norm_update_ranks_device(self, which, d_rows_ptr, row_stride, batch_local, d_mask_ptr=None):
        """norm_update_device of the ranks' rows concatenated in rank order, the same totals on every rank; a collective, no host sync."""
        self._check(self.L.lib.pmg_norm_update_ranks_device(self.h, C.c_int(which), C.c_void_p(d_rows_ptr), C.c_int64(row_stride), C.c_int64(batch_local),
                                                            C.c_void_p(d_mask_ptr) if d_mask_ptr else None))

    def norm_update_env_ranks_device(self, d_mask_ptr=None):
        self._check(self.L.lib.pmg_norm_update_env_ranks_device(self.h, C.c_void_p(d_mask_ptr) if d_mask_ptr else None))

    def timing_reset(self):
        self._check(self.L.lib.pmg_timing_reset(self.h))

    def timing_every(self, n):
        """Events around every n-th batched step only (an event costs ~6 us of idle queue on either side of the step)."""
        self._check(self.L.lib.pmg_timing_every(self.h, C.c_int(n)))

    def timing_read(self):
        ms = C.c_double()
        n = C.c_int64()
        self._check(self.L.lib.pmg_timing_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_stats(self):
        """(min, avg, max) ms of the step-kernel launches since timing_reset(), and their count."""
        lo, avg, hi = C.c_double(), C.c_double(), C.c_double()
        n = C.c_int64()
        self._check(self.L.lib.pmg_timing_stats(self.h, C.byref(lo), C.byref(avg), C.byref(hi), C.byref(n)))
        return lo.value, avg.value, hi.value, n.value

    # -- running normaliser + policy-input rows (include/pmg.h) --
    def norm_width(self, which):
        d = self.dims
        return (d.observation_dim, d.policy_state_dim, d.goal_dim)[which]

    def norm_configure(self, eps=0.01, clip_input=200.0, clip_output=5.0):
        self._check(self.L.lib.pmg_norm_configure(self.h, C.c_float(eps), C.c_float(clip_input), C.c_float(clip_output)))

    def norm_update(self, which, rows, mask=None):
        D = self.norm_width(which)
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim == 0 or rows.shape[-1] != D:
            raise ValueError('rows %s must have a shape ending in %d' % (rows.shape, D))
        B = rows.size // D
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(B)
        self._check(self.L.lib.pmg_norm_update(self.h, C.c_int(which), _p(rows), C.c_int64(B), _p(m)))

    def norm_update_device(self, which, d_rows_ptr, row_stride, batch, d_mask_ptr=None):
        self._check(self.L.lib.pmg_norm_update_device(self.h, C.c_int(which), C.c_void_p(d_rows_ptr), C.c_int64(row_stride),
                                                      C.c_int64(batch), C.c_void_p(d_mask_ptr) if d_mask_ptr else None))

    def norm_update_env_device(self, d_mask_ptr=None):
        self._check(self.L.lib.pmg_norm_update_env_device(self.h, C.c_void_p(d_mask_ptr) if d_mask_ptr else None))

    def norm_read(self, which):
        """dict(sum, sumsq [D] float64, count float, mean, std, inv_std [D] float32) of one normaliser."""
        D = self.norm_width(which)
        s, q, n = np.empty(D, np.float64), np.empty(D, np.float64), C.c_double()
        mean, std, inv = np.empty(D, np.float32), np.empty(D, np.float32), np.empty(D, np.float32)
        self._check(self.L.lib.pmg_norm_read(self.h, C.c_int(which), _p(s), _p(q), C.byref(n), _p(mean), _p(std), _p(inv)))
        return {'sum': s, 'sumsq': q, 'count': n.value, 'mean': mean, 'std': std, 'inv_std': inv}

    def norm_write(self, which, sum, sumsq, count):
        D = self.norm_width(which)
        s = np.ascontiguousarray(sum, np.float64).reshape(D)
        q = np.ascontiguousarray(sumsq, np.float64).reshape(D)
        self._check(self.L.lib.pmg_norm_write(self.h, C.c_int(which), _p(s), _p(q), C.c_double(count)))

    def policy_input(self, state_kind, state, goal):
        Ds, Dg = self.norm_width(state_kind), self.dims.goal_dim
        state = np.ascontiguousarray(state, np.float32)
        goal = np.ascontiguousarray(goal, np.float32)
        if state.ndim == 0 or goal.ndim == 0 or state.shape[-1] != Ds or goal.shape[-1] != Dg or state.shape[:-1] != goal.shape[:-1]:
            raise ValueError('state %s / goal %s must share their leading axes and end in %d / %d' % (state.shape, goal.shape, Ds, Dg))
        B = state.size // Ds
        out = np.empty(state.shape[:-1] + (Ds + Dg,), np.float32)
        self._check(self.L.lib.pmg_policy_input(self.h, C.c_int(state_kind), _p(state), _p(goal), C.c_int64(B), _p(out)))
        return out

    def policy_input_device(self, state_kind, d_state_ptr, state_stride, d_goal_ptr, goal_stride, batch, d_out_ptr):
        self._check(self.L.lib.pmg_policy_input_device(self.h, C.c_int(state_kind), C.c_void_p(d_state_ptr), C.c_int64(state_stride),
                                                       C.c_void_p(d_goal_ptr), C.c_int64(goal_stride), C.c_int64(batch), C.c_void_p(d_out_ptr)))

    def policy_input_env_device(self, state_kind, d_out_ptr):
        self._check(self.L.lib.pmg_policy_input_env_device(self.h, C.c_int(state_kind), C.c_void_p(d_out_ptr)))

    def get_rng(self):
        w = np.empty((self.N, 625), np.uint32)
        self._check(self.L.lib.pmg_get_rng(self.h, _p(w)))
        return w

    def set_rng(self, words):
        w = np.ascontiguousarray(words, np.uint32)
        if w.shape != (self.N, 625):
            raise ValueError('rng words must have shape (%d, 625)' % self.N)
        self._check(self.L.lib.pmg_set_rng(self.h, _p(w)))

    def comm_unique_id(self):
        buf = (C.c_uint8 * 128)()
        rc = self.L.lib.pmg_comm_unique_id(buf)
        if rc != 0:
            raise PmgError('pmg_comm_unique_id failed (%d)' % rc)
        return bytes(buf)

    def comm_init(self, rank, nranks, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.L.lib.pmg_comm_init(self.h, C.c_int(rank), C.c_int(nranks), buf))

    def comm_timing(self):
        """(avg, max) ms of the all-gathers since timing_reset() on this rank's stream, and their count."""
        avg, hi, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.L.lib.pmg_comm_timing(self.h, C.byref(avg), C.byref(hi), C.byref(n)))
        return avg.value, hi.value, n.value

    def allgather_packed(self, d_out_ptr):
        self._check(self.L.lib.pmg_allgather_packed(self.h, C.c_void_p(d_out_ptr)))

    def comm_overlap(self, enabled=True):
        """Double-buffer the packed rows so that allgather_packed_async() of step t runs beside step t + 1 (include/pmg.h)."""
        self._check(self.L.lib.pmg_comm_overlap(self.h, C.c_int32(1 if enabled else 0)))

    def allgather_packed_async(self, d_out_ptr):
        self._check(self.L.lib.pmg_allgather_packed_async(self.h, C.c_void_p(d_out_ptr)))

    def allgather_wait(self, host=True):
        self._check(self.L.lib.pmg_allgather_wait(self.h, C.c_int32(1 if host else 0)))
