"""``ops.decode.penalize_logits_`` on the GPU: csrc/logit_penalty.hip against the independent
yardstick of tests/penalty_helpers.py and against the PyTorch path on the same device, bit for bit."""
import pytest
import torch

import penalty_helpers as ph
from distributed_pipeline_amd.ops._ext import get_ext

pytestmark = pytest.mark.gpu

ALL = {**ph.CASES, **ph.GPU_ONLY_CASES}


@pytest.mark.parametrize("name", list(ALL))
def test_equals_the_yardstick_and_the_pytorch_path(name):
    ph.check_case(ALL[name](), "cuda")


def test_defaults_change_nothing():
    ph.check_defaults_change_nothing("cuda")


def test_rejections():
    ph.check_rejections("cuda")


def test_which_cases_the_kernel_takes():
    """The binding says whether the kernel ran: up to 2048 history columns in fp32 and bf16 with int32
    and int64 ids; a longer history, another dtype and a wide ``n`` are left to the caller."""
    ext = get_ext(required=True)
    n = torch.full((2,), 3, dtype=torch.int32, device="cuda")

    def ran(Lh, dtype=torch.bfloat16, ids=torch.int64, n=n):
        logits = torch.zeros(2, 50, device="cuda", dtype=dtype)
        hist = torch.ones(2, Lh, dtype=ids, device="cuda")
        took = ext.penalize_logits(logits, hist, n, None, 1.0, 0.5, 0.0, 0)
        assert took == bool(logits[0, 1] == -0.5) and not logits[:, 2:].any()
        return took

    assert ran(2048) and ran(2048, torch.float32, torch.int32) and ran(1)
    assert not ran(2049) and not ran(8, torch.float16) and not ran(8, ids=torch.int16) and not ran(8, n=n.long())


def test_more_rows_than_one_grid_dimension_of_65535():
    """One workgroup per row in the grid's x dimension: 70000 rows, each with its own id."""
    R, V = 70000, 7
    logits = torch.zeros(R, V, device="cuda")
    hist = (torch.arange(R, device="cuda", dtype=torch.int32) % V).view(R, 1)
    n = torch.ones(R, dtype=torch.int32, device="cuda")
    ph.penalize_logits_(logits, hist, n, presence_penalty=1.0)
    want = torch.zeros(R, V, device="cuda")
    want.scatter_(1, hist.long(), -1.0)
    assert torch.equal(logits, want)
