"""The chunked reduction on the host side: the new entry points in the bindings, the chunked numpy model of tests/grad_chunk_cases.py against
float64 gradients of torch.autograd, the ValueErrors of the faces' chunk_rows, and one whole update through env.actor / env.critic over the
emulator build of the C ABI."""
import pytest

import grad_cases as GC
import grad_chunk_cases as CC
from pybullet_multigoal_gym_amd._lib import PmgHandle, PmgLibrary


def test_abi_symbols():
    for name in ('pmg_mlp_grad_chunked_work_floats', 'pmg_mlp_grad_chunked_device'):
        assert name in PmgLibrary.SYMBOLS
    assert hasattr(PmgHandle, 'mlp_grad_chunked_work_floats') and hasattr(PmgHandle, 'mlp_grad_chunked_device')


@pytest.mark.parametrize('widths,out_act', GC.MODEL_NETS)
def test_the_chunked_model_is_the_gradient(widths, out_act):
    worst = 0.0
    for seed in GC.MODEL_SEEDS:
        err, same = CC.chunk_model_vs_autograd(widths, out_act, seed)
        print('%s B %d R %d seed %d: chunked model %.3g' % (widths, CC.MODEL_B, CC.MODEL_R, seed, err))
        assert same, ('the float32 and float64 ReLU masks differ: choose another seed', widths, seed)
        worst = max(worst, err)
    print('%s: largest max|g32 - g64| / max|g64|: chunked model %.3g (bar %.3g)' % (widths, worst, CC.CHUNK_MODEL_TOL))
    assert worst <= CC.CHUNK_MODEL_TOL


def test_chunk_rows_is_validated_on_the_host(emu_library):
    CC.case_host_value_errors(emu_library)


def test_one_whole_update_through_the_faces(emu_library):
    CC.case_whole_update(emu_library)
