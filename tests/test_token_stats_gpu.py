"""csrc/token_stats.hip (``ext.token_stats``, called directly) against the float64 evaluation of the
definition and against the PyTorch path, on the inputs and with the checks of
tests/token_stats_helpers.py."""
import pytest
import torch

import token_stats_helpers as th
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import token_stats, token_stats_ref

pytestmark = pytest.mark.gpu


def _kernel(logits, targets):
    out = get_ext().token_stats(logits, targets)
    assert out is not None, "the kernel must take fp32 / bf16 logits with V <= 65536 and int32 / int64 targets"
    assert len(out) == 4
    return out


@pytest.mark.parametrize("dtype", th.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,R", th.CASES)
def test_against_float64(V, R, dtype):
    covered = V <= 65536
    if not covered:  # declined by the binding, served by the PyTorch path on the device
        x, t = th.case(V, R, dtype)
        assert get_ext().token_stats(x.cuda(), t.cuda()) is None
    e_lp, e_en, worst = th.check_case(_kernel if covered else token_stats, "cuda", V, R, dtype)
    print(f"token_stats kernel V={V} R={R} {dtype}: e32 logp {e_lp:.3g} entropy {e_en:.3g}, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("V,R,dtype", [(257, 70, torch.float32), (4099, 70, torch.bfloat16), (50257, 70, torch.float32),
                                       (65536, 2, torch.bfloat16), (5, 70000, torch.float32)])
def test_agrees_with_the_torch_path_on_the_device(V, R, dtype):
    th.check_against_ref(_kernel, token_stats_ref, "cuda", V, R, dtype)


def test_ties_are_exact():
    th.check_ties(_kernel, "cuda")


def test_invariants():
    th.check_invariants(_kernel, "cuda")


def test_nonfinite_inputs():
    th.check_nonfinite(_kernel, "cuda")


def test_the_op_runs_the_kernel():
    logits, targets = th.case(4099, 70)
    a, b = token_stats(logits.cuda(), targets.cuda()), _kernel(logits.cuda(), targets.cuda())
    for p, q in zip(a, b):
        assert p.is_cuda and p.cpu().numpy().tobytes() == q.cpu().numpy().tobytes()
    # targets of another integer dtype, or on the CPU, are brought to the kernel's
    c = token_stats(logits.cuda(), targets.clamp(-1, 4099).to(torch.int16))
    assert torch.equal(c[1], a[1]) and torch.equal(c[3], a[3])


def test_uncovered_cases_take_the_torch_path():
    ext = get_ext()
    logits, targets = th.case(1000, 70)
    assert ext.token_stats(logits, targets) is None                                   # CPU tensors
    x, t = logits.cuda(), targets.cuda()
    assert ext.token_stats(x.half(), t) is None                                       # dtype
    assert ext.token_stats(x.double(), t) is None
    assert ext.token_stats(x[:, ::2], t) is None                                      # last stride 2
    assert ext.token_stats(x, t.to(torch.int16)) is None                              # target dtype
    assert ext.token_stats(x, targets) is None                                        # targets on another device
    assert ext.token_stats(torch.zeros(2, 65537, device="cuda"), t[:2]) is None       # V > 65536
    assert ext.token_stats(torch.zeros(0, 5, device="cuda"), t[:0]) is None           # no rows
    with pytest.raises(RuntimeError):
        ext.token_stats(x, t[:3])
    # the op then runs the PyTorch path on the device
    for args, cpu in (((x.half(), t), (logits.half(), targets)), ((x[:, ::2], t), (logits[:, ::2], targets))):
        got = th._to_cpu(token_stats(*args))
        th.assert_matches(got, cpu[0], cpu[1], th.e32_logp(cpu[0]), th.e32_entropy())
    out = token_stats(torch.zeros(0, 5, device="cuda"), t[:0])
    assert all(o.is_cuda and o.shape == (0,) for o in out)
