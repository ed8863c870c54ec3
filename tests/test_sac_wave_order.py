"""CPU tier: pmg_k_sac and pmg_k_sac_target (four wavefronts on one LDS tile through the actor, the head's pass, the sum of log pi, the
rebuild of x' | a' and either critic) under permuted wavefront order, as tests/test_td3_wave_order.py does for their sibling: the identity
and the reverse list give the bits of the default scheduler, so every hand-over through the tile is fenced by a barrier.  The shapes are
(3, 12), (1, 20) -- Dx < A, where the siblings' descending hand-over would overwrite log-stds still to be read -- and (6, 3), with two critics
and a' kept in d_next_action and in the workspace."""
import sac_cases as SC
from test_wave_order import FOUR, Waves, _under_orders


def test_sac_kernels_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: SC.wave_order_run(emu_library))
    finally:
        waves.set(())
