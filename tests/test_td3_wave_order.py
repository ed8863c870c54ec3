"""CPU tier: pmg_k_td3_target (four wavefronts on one LDS tile through the actor, the hand-over with the noise, critic 1, the restore of
x' | a~ and critic 2) under permuted wavefront order, as tests/test_policy_grad_wave_order.py does for its sibling: the identity and the
reverse list give the bits of the default scheduler, so every hand-over through the tile is fenced by a barrier.  The shapes have
A > Dx + 8 (source and target columns of the hand-over overlap over more than one pass) and two critics, a~ kept in d_next_action and in
the workspace."""
import td3_cases as T3
from test_wave_order import FOUR, Waves, _under_orders


def test_td3_target_kernel_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: T3.wave_order_run(emu_library))
    finally:
        waves.set(())
