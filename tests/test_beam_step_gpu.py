"""csrc/beam_step.hip (``ext.beam_step``, called directly) against the float64 evaluation of the
definition and against the PyTorch path, on the inputs and with the checks of tests/beam_helpers.py."""
import pytest
import torch

import beam_helpers as bh
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import beam_step, beam_step_ref

pytestmark = pytest.mark.gpu


def _kernel(logits, scores, finished, eos_id, fill):
    out = get_ext().beam_step(logits, scores, finished, eos_id, fill)
    assert out is not None, "the kernel must take fp32 / bf16 logits with V <= 65536 and W <= 8"
    assert len(out) == 5
    return out[:4]


def _kernel5(logits, scores, finished, eos_id, fill):
    return get_ext().beam_step(logits, scores, finished, eos_id, fill)


@pytest.mark.parametrize("kind", ["plain", "mixed"])
@pytest.mark.parametrize("W", bh.WS)
@pytest.mark.parametrize("V", bh.VS)
def test_exact_picks_and_agreement_with_the_torch_path(V, W, kind):
    (ns, par, tok, nf), gap = bh.check_exact(_kernel, "cuda", V, W, kind)
    print(f"beam_step kernel V={V} W={W} {kind}: smallest gap = {gap:.1f} e32")
    logits, scores, finished = bh.case(V, W, kind)
    e32 = bh.e32_of(logits, scores, finished)
    rs, rp, rt, rf = beam_step_ref(logits, scores, finished, eos_id=17, fill=5)
    assert torch.equal(par, rp) and torch.equal(tok, rt) and torch.equal(nf, rf)
    assert ((ns.double() - rs.double()).abs() <= 4 * e32 + 2.0 ** -23 * rs.double().abs()).all()
    again = _kernel(bh.strided(logits, "cuda"), scores.cuda(), finished.cuda(), 17, 5)
    for a, b in zip((ns, par, tok, nf), again):
        assert a.numpy().tobytes() == b.cpu().numpy().tobytes()  # bit for bit


@pytest.mark.parametrize("V,W", [(3000, 3), (4099, 8), (50257, 2)])
def test_bf16_logits_agree_with_float64_on_the_bf16_values(V, W):
    _, gap = bh.check_exact(_kernel, "cuda", V, W, "mixed", dtype=torch.bfloat16)
    print(f"beam_step kernel bf16 V={V} W={W}: smallest gap = {gap:.1f} e32")


def test_ties_are_exact():
    bh.check_ties(_kernel, "cuda")


def test_logp_is_the_picks_own_term():
    bh.check_logp(_kernel5, "cuda")


def test_finished_beams():
    bh.check_finished(_kernel, "cuda")


def test_degenerate_inputs():
    bh.check_degenerate(_kernel, "cuda")


def test_uncovered_cases_take_the_torch_path():
    ext = get_ext()
    logits, scores, finished = bh.case(3000, 2, "plain")
    assert ext.beam_step(logits, scores, finished, -1, 0) is None                        # CPU tensors
    x, s, f = logits.cuda(), scores.cuda(), finished.cuda()
    assert ext.beam_step(x.half(), s, f, -1, 0) is None                                   # dtype
    assert ext.beam_step(x.expand(3, 2, 3000)[:, :, ::2], s, f, -1, 0) is None            # last stride 2
    wide = torch.randn(1, 9, 64, generator=torch.Generator().manual_seed(3)).cuda()
    s9, f9 = torch.zeros(1, 9, device="cuda"), torch.zeros(1, 9, dtype=torch.bool, device="cuda")
    assert ext.beam_step(wide, s9, f9, -1, 0) is None                                     # W > 8
    big = torch.randn(1, 1, 65537, device="cuda")
    assert ext.beam_step(big, s9[:, :1].contiguous(), f9[:, :1].contiguous(), -1, 0) is None  # V > 65536
    # the op then runs the PyTorch path on the device: the same picks as on the CPU (the ten best
    # of these 576 candidates lie far further apart than fp32 rounding)
    for args, cpu in (((wide, s9, f9), (wide.cpu(), s9.cpu(), f9.cpu())),
                      ((x[:, :, ::2], s, f), (logits[:, :, ::2], scores, finished))):
        got, want = beam_step(*args), beam_step_ref(*cpu)
        assert all(g.is_cuda for g in got)
        assert torch.equal(got[1].cpu(), want[1]) and torch.equal(got[2].cpu(), want[2])
        assert torch.allclose(got[0].cpu(), want[0], rtol=0, atol=1e-5)
