"""CPU tier: the chunked gradient under permuted wavefront order, as tests/test_grad_wave_order.py does for the single chain.  The rows kernel
and the merge kernel (pmg_k_mlp_grad_merge: 256 threads, four wavefronts that share nothing) run under the identity and the reverse list and
give the bits of the default scheduler."""
import grad_chunk_cases as CC
from test_wave_order import FOUR, Waves, _under_orders


def test_chunked_gradient_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: CC.wave_order_run(emu_library))
    finally:
        waves.set(())
