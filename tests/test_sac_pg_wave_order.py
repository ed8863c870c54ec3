"""CPU tier: pmg_k_sac_policy_grad_rows (four wavefronts on one LDS tile through the actor, the head's pass, the rebuilds, both critics forward
and backward, the pipelined hand-back and the actor's transposed layers) under permuted wavefront order, as tests/test_sac_wave_order.py does
for its sibling: the identity and the reverse list give the bits of the default scheduler, so every exchange through the tile is fenced by a
barrier.  The shapes are (3, 12), (1, 20) -- Dx < A, where the hand-back's writes overlap the ga still to be read -- and (6, 3), with two
critics, a kept in d_action and in the workspace, grads given, and a chunked run."""
import sac_pg_cases as SP
from test_wave_order import FOUR, Waves, _under_orders


def test_sac_policy_grad_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: SP.wave_order_run(emu_library))
    finally:
        waves.set(())
