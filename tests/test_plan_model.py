"""The plan model and its case set on the CPU alone (tests/plan_cases.py; no device code, no emulator): the cases keep clear of every
threshold and hold every class, the model's float64 kinematics are the oracle's, and the case set has teeth -- three plausible ways of
getting the plan wrong, built into the model, each give another schedule on at least one case."""
import numpy as np
import pytest

import plan_cases as PC


def test_no_env_within_a_band_and_every_class_present():
    PC.check_case_set()


def test_model_kinematics_are_the_oracles(built):
    import oracle_lib
    PC.check_fk_against_oracle(oracle_lib.fk_tip)


def test_sizes_cover_every_boundary_of_the_plan():
    sizes = {N for _, N in PC.CASES}
    assert sizes == set(PC.SIZES)
    assert {1, 63, 65, 1023, 1025, 16384, 16385, 65536 + 256} <= sizes
    for family in PC.FAMILIES + ('reach',):
        assert len({N for f, N in PC.CASES if f == family}) >= 2, family
    # count(1) % 4 != 0 (surplus rows of the last packed wavefront) and == 0 both occur
    rem = {len(PC.model(PC.case(f, N))['list1']) % 4 for f, N in PC.CASES if N <= 4097}
    assert rem == {0, 1, 2, 3}


@pytest.mark.parametrize('mutant', ['le_height', 'class2_first', 'per_workgroup'])
def test_case_set_catches_a_wrong_plan(mutant):
    """<= for < at the height test; class 2 in front of an unpromoted class 1; promotion decided per workgroup instead of from the
    grand totals: the schedule of each differs from the rule's on some case, so a plan that did the same would fail that case."""
    caught = []
    for family, N in PC.CASES:
        c = PC.case(family, N)
        good, bad = PC.model(c), PC.model(c, mutant)
        if not (np.array_equal(good['list0'], bad['list0']) and np.array_equal(good['list1'], bad['list1']) and good['promoted'] == bad['promoted']):
            caught.append(PC.case_id((family, N)))
    print(mutant, 'caught by', len(caught), 'cases:', ' '.join(caught[:8]))
    assert caught
