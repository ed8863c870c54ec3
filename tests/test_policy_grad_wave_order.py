"""CPU tier: the rows kernel of the policy gradient (pmg_k_policy_grad_rows: four wavefronts on one LDS tile through the actor's forward, the
hand-over, the critic's forward and transposed layers, the hand-back and the actor's transposed layers) under permuted wavefront order, as
tests/test_grad_wave_order.py does for its sibling: the identity and the reverse list give the bits of the default scheduler, so every
hand-over through the tile is fenced by a barrier."""
import policy_grad_cases as PC
from test_wave_order import FOUR, Waves, _under_orders


def test_policy_grad_rows_kernel_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: PC.wave_order_run(emu_library))
    finally:
        waves.set(())
