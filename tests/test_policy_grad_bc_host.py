"""The policy gradient with the behaviour-cloning term through the numpy faces (Actor.policy_grad_bc, policy_grad_bc_device) over the emulator
build of the C ABI, the bindings, and the numpy model of tests/policy_grad_bc_cases.py against float64 gradients of torch.autograd."""
import ctypes as C

import pytest

import policy_grad_bc_cases as BC
import policy_grad_cases as PC
from pybullet_multigoal_gym_amd._lib import PmgLibrary, PmgPolicyBc


def test_abi_symbol_and_struct_size():
    assert 'pmg_policy_grad_bc_device' in PmgLibrary.SYMBOLS
    assert C.sizeof(PmgPolicyBc) == 56            # as sizeof(pmg_policy_bc) in include/pmg.h on LP64
    assert PmgPolicyBc.demo_begin.offset == 16 and PmgPolicyBc.d_filter.offset == 48


@pytest.mark.parametrize('q_filter', (1, 0))
@pytest.mark.parametrize('widths,out_act,critic_hidden', PC.MODEL_NETS)
def test_the_model_is_the_gradient(widths, out_act, critic_hidden, q_filter):
    worst = 0.0
    for seed in PC.MODEL_SEEDS:
        err, same, cloned = BC.model_vs_autograd(widths, out_act, critic_hidden, PC.MODEL_B, seed, q_filter)
        print('%s seed %d q_filter %d: max|g32 - g64| / max|g64| = %.3g, %.0f %% of the demonstration rows cloned' % (widths, seed, q_filter, err, 100 * cloned))
        assert same, ('the float32 and float64 ReLU masks, clip predicates or filters differ: choose another seed', widths, seed)
        assert cloned == 1.0 if not q_filter else 0.0 < cloned < 1.0, ('the filter passes %.0f %% of the demonstration rows' % (100 * cloned), widths, seed)
        worst = max(worst, err)
    print('%s: largest %.3g (bar %.3g)' % (widths, worst, BC.MODEL_TOL))
    assert worst <= BC.MODEL_TOL


def test_through_the_faces(emu_library):
    BC.case_through_the_faces(emu_library)
