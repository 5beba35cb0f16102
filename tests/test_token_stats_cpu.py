"""``ops.decode.token_stats`` on the PyTorch path (CPU tensors) against the float64 evaluation of the
definition, on the inputs and with the checks of tests/token_stats_helpers.py."""
import math

import pytest
import torch

import token_stats_helpers as th
from distributed_pipeline_amd.ops.decode import token_stats, token_stats_ref


@pytest.mark.parametrize("dtype", th.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,R", th.CASES)
def test_against_float64(V, R, dtype):
    e_lp, e_en, worst = th.check_case(token_stats, "cpu", V, R, dtype)
    print(f"token_stats torch V={V} R={R} {dtype}: e32 logp {e_lp:.3g} entropy {e_en:.3g}, worst error / bound {worst:.3f}")


def test_ties_are_exact():
    th.check_ties(token_stats, "cpu")


def test_invariants():
    th.check_invariants(token_stats, "cpu")


def test_nonfinite_inputs():
    th.check_nonfinite(token_stats, "cpu")


def test_chunking_changes_nothing():
    logits, targets = th.case(257, 70)
    whole = token_stats_ref(logits, targets)
    parts = token_stats_ref(logits, targets, chunk_elems=257 * 7 + 3)  # 7 rows a chunk
    for a, b in zip(whole, parts):
        assert a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_other_float_dtypes_are_taken_as_fp32(dtype):
    logits, targets = th.case(1000, 70)
    x = logits.to(dtype)
    got = th._to_cpu(token_stats(x, targets))
    th.assert_matches(got, x, targets, th.e32_logp(x), th.e32_entropy())
    # int32, int16 targets
    for tdt in (torch.int32, torch.int16):
        t = targets.clamp(-1, 1000).to(tdt)
        a, b = token_stats(x, t), token_stats(x, t.long())
        assert all(torch.equal(p, q) for p, q in zip(a[1::2], b[1::2]))


def test_a_case_worked_by_hand():
    # logits log 1, log 2, log 4, log 1 -> p = 1/8, 2/8, 4/8, 1/8
    x = torch.tensor([[1.0, 2.0, 4.0, 1.0]]).log().repeat(4, 1)
    logp, rank, ent, top1 = token_stats(x, torch.tensor([0, 1, 2, 3]))
    assert rank.tolist() == [2, 1, 0, 3] and top1.tolist() == [2] * 4
    want = torch.tensor([1 / 8, 2 / 8, 4 / 8, 1 / 8]).log()
    assert torch.allclose(logp, want, rtol=0, atol=1e-6)
    h = -(2 * (1 / 8) * math.log(1 / 8) + (2 / 8) * math.log(2 / 8) + (4 / 8) * math.log(4 / 8))
    assert torch.allclose(ent, torch.full((4,), h), rtol=0, atol=1e-6)


def test_bad_arguments():
    x = torch.zeros(3, 5)
    with pytest.raises(ValueError):
        token_stats(x, torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        token_stats(x[0], torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError):
        token_stats(x, torch.zeros(3))
    with pytest.raises(ValueError):
        token_stats(x.long(), torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError):
        token_stats(torch.zeros(3, 0), torch.zeros(3, dtype=torch.long))
    out = token_stats(torch.zeros(0, 5), torch.zeros(0, dtype=torch.long))
    assert [o.shape for o in out] == [(0,)] * 4
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.float32, torch.int32]
