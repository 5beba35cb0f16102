"""``ops.decode.beam_step`` on the CPU (the PyTorch path, ``beam_step_ref``) against a float64
evaluation of the definition: exact picks under an asserted separation of the candidates, the tie
rule, finished beams and degenerate rows (tests/beam_helpers.py holds the checks)."""
import pytest
import torch

import beam_helpers as bh
from distributed_pipeline_amd.ops.decode import beam_step, beam_step_ref


def _step(logits, scores, finished, eos_id, fill):
    return beam_step(logits, scores, finished, eos_id=eos_id, fill=fill)


@pytest.mark.parametrize("kind", ["plain", "mixed"])
@pytest.mark.parametrize("W", bh.WS)
@pytest.mark.parametrize("V", bh.VS)
def test_exact_picks(V, W, kind):
    _, gap = bh.check_exact(_step, "cpu", V, W, kind)
    print(f"beam_step cpu V={V} W={W} {kind}: smallest gap = {gap:.1f} e32")


def test_ties_are_exact():
    bh.check_ties(_step, "cpu")


def test_logp_is_the_picks_own_term():
    bh.check_logp(lambda x, s, f, eos, fill: beam_step(x, s, f, eos_id=eos, fill=fill, return_logp=True), "cpu")


def test_finished_beams():
    bh.check_finished(_step, "cpu")


def test_degenerate_inputs():
    bh.check_degenerate(_step, "cpu")


def test_chunking_and_dtypes_do_not_change_the_result():
    logits, scores, finished = bh.case(3000, 3, "mixed")
    want = beam_step_ref(logits, scores, finished, eos_id=17, fill=5)
    for chunk in (1, 3, 4, 1000):
        got = beam_step_ref(logits, scores, finished, eos_id=17, fill=5, chunk=chunk)
        assert all(torch.equal(a, b) for a, b in zip(want, got))
    got = beam_step(logits.double(), scores, finished, eos_id=17, fill=5)  # another dtype: the same path
    assert all(torch.equal(a, b) for a, b in zip(want, got))


def test_argument_checks():
    logits, scores, finished = bh.case(3000, 2, "plain")
    with pytest.raises(ValueError):
        beam_step(logits[0], scores, finished)
    with pytest.raises(ValueError):
        beam_step(logits, scores[:, :1], finished)
    with pytest.raises(ValueError):
        beam_step(logits, scores.double(), finished)
    with pytest.raises(ValueError):
        beam_step(logits, scores, finished.int())
