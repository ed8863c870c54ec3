"""CPU tier: the rows kernel of the policy gradient with the behaviour-cloning term (pmg_k_policy_grad_bc_rows: pmg_k_policy_grad_rows' passes
behind a demonstration pass of the critic, and the filter flags handed from the row's thread to the hand-back through LDS) under permuted
wavefront order, as tests/test_policy_grad_wave_order.py does for its sibling: the identity and the reverse list give the bits of the default
scheduler, so every hand-over through the tile and the filter's is fenced by a barrier."""
import policy_grad_bc_cases as BC
from test_wave_order import FOUR, Waves, _under_orders


def test_policy_grad_bc_rows_kernel_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: BC.wave_order_run(emu_library))
    finally:
        waves.set(())
