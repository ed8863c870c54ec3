"""CPU tier: the rows kernel of the gradient (pmg_k_mlp_grad_rows: four wavefronts on one LDS tile through forward, head and the transposed
layers) under permuted wavefront order, as tests/test_wave_order.py does for the other kernels: the identity and the reverse list give the
bits of the default scheduler, so every hand-over through the tile is fenced by a barrier."""
import grad_cases as GC
from test_wave_order import FOUR, Waves, _under_orders


def test_grad_rows_kernel_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: GC.wave_order_run(emu_library))
    finally:
        waves.set(())
