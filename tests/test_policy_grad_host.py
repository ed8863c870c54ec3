"""The policy gradient through the numpy faces (Actor.policy_grad, policy_grad_device, policy_grad_work_floats) over the emulator build of the
C ABI, the bindings, and the numpy model of tests/policy_grad_cases.py against float64 gradients of torch.autograd."""
import ctypes as C

import pytest

import grad_cases as GC
import policy_grad_cases as PC
from pybullet_multigoal_gym_amd._lib import PmgLibrary, PmgPolicyGrad


def test_abi_symbols_and_struct_size():
    for name in ('pmg_policy_grad_work_floats', 'pmg_policy_grad_device'):
        assert name in PmgLibrary.SYMBOLS
    assert C.sizeof(PmgPolicyGrad) == 120         # as sizeof(pmg_policy_grad) in include/pmg.h on LP64


@pytest.mark.parametrize('widths,out_act,critic_hidden', PC.MODEL_NETS)
def test_the_model_is_the_gradient(widths, out_act, critic_hidden):
    worst = 0.0
    for seed in PC.MODEL_SEEDS:
        err, same, outside = PC.model_vs_autograd(widths, out_act, critic_hidden, PC.MODEL_B, seed)
        print('%s seed %d: max|g32 - g64| / max|g64| = %.3g, %.0f %% of the outputs outside [-1, 1]' % (widths, seed, err, 100 * outside))
        assert same, ('the float32 and float64 ReLU masks or clip predicates differ: choose another seed', widths, seed)
        assert out_act or 0.25 < outside < 0.75, ('the clip is active on %.0f %% of the outputs, not on roughly half' % (100 * outside), widths, seed)
        worst = max(worst, err)
    print('%s: largest %.3g (bar %.3g)' % (widths, worst, GC.MODEL_TOL))
    assert worst <= GC.MODEL_TOL


def test_through_the_faces(emu_library):
    PC.case_through_the_faces(emu_library)
