"""The fused SAC actor update on the CPU tier: the cases of tests/sac_pg_cases.py on the g++ build of the product sources
(pmg_k_sac_policy_grad_rows and pmg_k_sac_alpha with the fmaf body of the matrix step) over the fiber emulator, through the C ABI.  The emulator
proves the head's column map, the stashes in the workspace and in d_ghead, the rebuild in front of either critic from d_action and from the
workspace, the selection, the pipelined hand-back and the two chains of the temperature; the lane maps of the MFMA and the build's expf are
proven by tests/test_gpu_sac_pg.py."""
import pytest

import sac_pg_cases as SP


@pytest.mark.parametrize('case', SP.CASES)
def test_against_the_sequence_of_existing_calls(emu_library, case):
    SP.case_sequence(emu_library, (case,))


def test_the_cases_cover_both_critics_and_the_clamp():
    """by the model alone (tests/test_gpu_sac_pg.py asserts it on the device's own outputs): q1 < q2, q2 < q1, log-stds below, inside and above
    the clamp all occur over the cases"""
    assert SP.model_coverage() == SP.COVERAGE


def test_against_float64_autograd(emu_library):
    SP.case_autograd(emu_library)


@pytest.mark.parametrize('pair', SP.PAIRS)
def test_without_noise_and_entropy_is_the_ddpg_kernel(emu_library, pair):
    SP.case_is_policy_grad(emu_library, (pair,))


def test_edges(emu_library):
    SP.case_edges(emu_library)


def test_stale_tile_contents(emu_library):
    SP.case_stale_tile(emu_library)


def test_properties(emu_library):
    SP.case_properties(emu_library)


def test_temperature(emu_library):
    SP.case_alpha(emu_library)


def test_through_the_faces(emu_library):
    SP.case_host_face(emu_library)


def test_invalid_calls(emu_library):
    SP.case_invalid_calls(emu_library)
