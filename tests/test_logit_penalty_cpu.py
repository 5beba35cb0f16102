"""``ops.decode.penalize_logits_`` on the CPU: the PyTorch path against the independent yardstick of
tests/penalty_helpers.py, bit for bit."""
import pytest
import torch

import penalty_helpers as ph


@pytest.mark.parametrize("name", list(ph.CASES))
def test_equals_the_yardstick(name):
    ph.check_case(ph.CASES[name](), "cpu")


def test_the_yardstick_itself_on_a_case_worked_by_hand():
    """w = [5, 9, 7, 5, 3, 5], g = 2: the window ends in 5, and 9 and 3 follow a 5 -> banned.  Id 5
    is seen three times: 2.5 / 1.25 = 2, minus (0.5 + 0.25 * 3) = 0.75; id 7 once, from -2: -2.5 - 0.75."""
    logits = torch.full((1, 12), 2.5)
    logits[0, 7] = -2.0
    got = ph.yardstick(logits, torch.tensor([[5, 9, 7, 5, 3, 5, 11]]), torch.tensor([6]), None, 1.25, 0.5, 0.25, 2)
    want = torch.full((1, 12), 2.5)
    want[0, 5], want[0, 9], want[0, 3] = 0.75, ph.NINF, ph.NINF
    want[0, 7] = -3.25
    assert torch.equal(got, want)
    assert ph.banned_set([4, 4, 4], 3) == {4} and ph.banned_set([4, 4, 4], 4) == set() and ph.banned_set([1, 2], 1) == {1, 2}


def test_defaults_change_nothing():
    ph.check_defaults_change_nothing("cpu")


def test_rejections():
    ph.check_rejections("cpu")


def test_other_dtypes_take_the_pytorch_path():
    case = ph.make_case(31, 3, 97, 65, 2, dtype=torch.float16, a_p=0.25)
    ph.check_case(case, "cpu")
    case = ph.make_case(32, 3, 97, 65, 2, dtype=torch.float64, hist_dtype=torch.int16, a_f=0.25)
    ph.check_case(case, "cpu")


def test_chunks_of_rows_do_not_change_the_result():
    case = ph.CASES["R70_V97_L65"]()
    a, la, hist, n, start = ph.place(case, "cpu")
    b, lb, _, _, _ = ph.place(case, "cpu")
    ph.penalize_logits_ref(la, hist, n, start=start, **ph.scalars(case))
    ph.penalize_logits_ref(lb, hist, n, start=start, chunk_elems=3 * 65 * 65, **ph.scalars(case))
    assert ph.same_bits(a, b)
