"""CPU tier: the three kernels of the data-parallel merge under permuted wavefront order, as tests/test_grad_chunk_wave_order.py does for the
chunked gradient.  pmg_k_params_pack, pmg_k_params_merge_ranks and pmg_k_adam_merge_ranks run 256 threads, four wavefronts that share
nothing: under the identity and the reverse list they give the bits of the default scheduler."""
import dp_cases as DP
from test_wave_order import FOUR, Waves, _under_orders


def test_pack_merge_and_fused_adam_under_wavefront_orders(emu_library):
    waves = Waves(emu_library)
    try:
        _under_orders(waves, FOUR, lambda: DP.wave_order_run(emu_library))
    finally:
        waves.set(())
