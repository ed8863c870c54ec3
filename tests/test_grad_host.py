"""The update side through the numpy faces (env.actor / env.critic: grad, adam_step_device, soft_update_from; optim.AdamState) over the
emulator build of the C ABI, the bindings, and the numpy model of tests/grad_cases.py against float64 gradients of torch.autograd."""
import ctypes as C

import pytest

import grad_cases as GC
from pybullet_multigoal_gym_amd._lib import PmgAdam, PmgLibrary, PmgMlpGrad, PmgMlpParams


def test_abi_symbols_and_struct_sizes():
    for name in ('pmg_mlp_grad_work_floats', 'pmg_mlp_grad_device', 'pmg_mlp_adam_device', 'pmg_mlp_polyak_device'):
        assert name in PmgLibrary.SYMBOLS
    # as sizeof(pmg_mlp_params), sizeof(pmg_mlp_grad), sizeof(pmg_adam) in include/pmg.h on LP64
    assert (C.sizeof(PmgMlpParams), C.sizeof(PmgMlpGrad), C.sizeof(PmgAdam)) == (64, 168, 32)


@pytest.mark.parametrize('widths,out_act', GC.MODEL_NETS)
def test_the_model_is_the_gradient(widths, out_act):
    worst = worst32 = 0.0
    for B in (33, 101):
        for seed in GC.MODEL_SEEDS:
            chain, own32, same = GC.model_vs_autograd(widths, out_act, B, seed)
            print('%s B %d seed %d: chain model %.3g, torch float32 %.3g' % (widths, B, seed, chain, own32))
            assert same, ('the float32 and float64 ReLU masks differ: choose another seed', widths, B, seed)
            worst, worst32 = max(worst, chain), max(worst32, own32)
    print('%s: largest max|g32 - g64| / max|g64|: chain model %.3g (bar %.3g), torch float32 %.3g' % (widths, worst, GC.MODEL_TOL, worst32))
    assert worst <= GC.MODEL_TOL


def test_one_whole_update_through_the_faces(emu_library):
    GC.case_whole_update(emu_library)
