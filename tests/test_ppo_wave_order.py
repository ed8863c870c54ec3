"""CPU tier: pmg_k_ppo_policy_grad_rows (four wavefronts on one LDS tile through the actor, the head's first pass, the row sums, the hand-back
of g_mu | g_ls and the actor's transposed layers) under permuted wavefront order, as tests/test_sac_pg_wave_order.py does for its sibling: the
identity and the reverse list give the bits of the default scheduler, so every exchange through the tile and through the per-row k beside it is
fenced by a barrier -- the ownership and barrier rules stated above the kernel.  The shapes are (2, 5) behind three hidden layers of 256,
(1, 20) -- 32 A = 640 (row, unit) pairs: three passes of the map, rows shared between wavefronts -- and (6, 3); grads given (one chain and
chunked) and d_ghead alone, where the stash is d_ghead."""
import ppo_cases as PP
from test_wave_order import FOUR, Waves, _under_orders


def test_ppo_policy_grad_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: PP.wave_order_run(emu_library))
    finally:
        waves.set(())
