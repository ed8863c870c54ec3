"""CPU tier: every call the data-parallel entries refuse (include/pmg.h) -- PMG_E_STATE without a communicator and under
pmg_comm_overlap, the PMG_E_INVALID lists, a batch_local that is no multiple of the global chunk, a workspace one float short, an
env_index_offset that is not rank * N -- with guard bytes around the workspace, the slots and every tensor that must stay untouched; and the
host faces' own errors."""
import numpy as np
import pytest

import dp_cases as DP
from pybullet_multigoal_gym_amd import distributed as D


def test_invalid_calls(emu_library):
    DP.case_invalid_calls(emu_library)


def test_faces_refuse_what_is_not_theirs(emu_library):
    env = DP.AC.stepped(emu_library, 'reach', 8)
    try:
        critic = env.critic
        Ws, bs = DP.GC.net(802, (9, 33, 1))
        critic.load(Ws, bs)
        P = 9 * 33 + 33 + 33 + 1
        assert critic.param_floats() == P and critic.allreduce_work_floats() == 2 * P
        other = DP.AC.stepped(emu_library, 'reach', 8)
        try:
            other.critic.load(*DP.GC.net(803, (9, 17, 1)))
            wrong = other.critic.adam_state()
            for call in (lambda: critic.allreduce_grads_device(wrong.g, 16, 2 * P), lambda: critic.allreduce_grads_device(None, 16, 2 * P),
                         lambda: critic.adam_step_allreduce_device(wrong.g, critic.adam_state(), 1e-3, 16, 2 * P),
                         lambda: critic.adam_step_allreduce_device(critic.adam_state().g, wrong, 1e-3, 16, 2 * P),
                         lambda: critic.adam_step_allreduce_device(critic.adam_state().g, critic.adam_state(), float('nan'), 16, 2 * P),
                         lambda: critic.merge_params(np.zeros((2, P + 1), np.float32)), lambda: critic.merge_params(np.zeros(P, np.float32)),
                         lambda: critic.merge_params(np.zeros((0, P), np.float32))):
                with pytest.raises(ValueError):
                    call()
        finally:
            other.close()
        # the numpy faces: pack is the flat order, merge the rank-ordered sum
        rs = np.random.RandomState(804)
        dW, db = [rs.uniform(-1, 1, w.shape).astype(np.float32) for w in Ws], [rs.uniform(-1, 1, b.shape).astype(np.float32) for b in bs]
        flat = critic.pack_params(dW, db)
        assert np.array_equal(flat, DP.flatten(dW, db))
        slots = np.stack([flat, flat * np.float32(3), -flat])
        mW, mb = critic.merge_params(slots)
        DP.eq_bits(DP.flatten(mW, mb), DP.rank_sum(slots), 'merge_params')
        # without a communicator the collectives of the faces raise the library's PMG_E_STATE
        from pybullet_multigoal_gym_amd._lib import PmgError
        state = critic.adam_state()
        d_work = env.handle.device_alloc(8 * P)
        for call in (lambda: critic.allreduce_grads_device(state.g, d_work, 2 * P), lambda: critic.adam_step_allreduce_device(state.g, state, 1e-3, d_work, 2 * P),
                     lambda: env.normalizer.update_ranks(goal=np.zeros((64, 3), np.float32)), lambda: env.normalizer.update_from_env_ranks(),
                     lambda: env.handle.comm_info()):
            with pytest.raises(PmgError, match='pmg_comm_init'):
                call()
        assert state.t == 0
        env.handle.device_free(d_work)
    finally:
        env.close()


class _OneRank:
    rank, world = 0, 1

    def allgather(self, obj):
        return [obj]


def test_check_data_parallel_names_what_is_wrong(emu_library):
    env = DP.AC.stepped(emu_library, 'reach', 8)
    shifted = DP.AC.stepped(emu_library, 'reach', 8, env_index_offset=8)
    try:
        for e in (env, shifted):
            DP.one_rank(e.handle)
        assert D.check_data_parallel(env, _OneRank()) == (0, 1) and D.check_data_parallel(env, _OneRank(), batch_local=34) == (0, 1)
        with pytest.raises(ValueError, match='env_index_offset'):
            D.check_data_parallel(shifted, _OneRank())
        for bad in (33, 0):
            with pytest.raises(ValueError, match='even'):
                D.check_data_parallel(env, _OneRank(), batch_local=bad)
        two = _OneRank()
        two.world = 2
        with pytest.raises(ValueError, match='communicator'):
            D.check_data_parallel(env, two)
        two.world, two.allgather = 1, lambda obj: [obj, [16, -1, '']]
        with pytest.raises(ValueError, match='unequal'):
            D.check_data_parallel(env, two)
    finally:
        env.close()
        shifted.close()
