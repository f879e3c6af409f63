"""CPU: the inputs of tests/test_gpu_march4d_paths.py reach the branches they are for -- and only because of their knobs.  Every
condition is evaluated with the case's knobs (it must hold: the GPU test asserts the same before its GPU call) and with the knobs
back at their defaults (it must FAIL: the condition is about the branch, not about the field)."""
import pytest

import test_gpu_march4d_paths as T


@pytest.mark.parametrize("name", sorted(T.KNOB_CASES))
def test_input_reaches_the_branch_only_under_its_knobs(name):
    case = T.KNOB_CASES[name]
    case["cond"](T.case_env(name))
    with pytest.raises(AssertionError):
        case["cond"]({})
    with pytest.raises(AssertionError):
        case["cond"](dict(case["env"]))          # the knobs without CX_DEBUG=1 are not honoured either


def test_fuzz_slice_inputs():
    T.fuzz_slice_conditions()


def test_set_order_cases_build_their_fields():
    cases = T.set_order_cases()
    assert len(cases) == 18 and [k for k, _ in cases].count("exact") == 8 and [k for k, _ in cases].count("boundary") == 8
    for n, (kind, case) in enumerate(cases):
        A = T.set_order_field(case, n, (0, 1, 0, 1))
        assert int((A[0:2, 1:3, 0:2, 1:3] < 0).sum()) == 2 and not (A == 0).any()
