"""``GPT2LMModel.beam_search`` on the GPU: the ``TINY`` model in bf16 on the native kernels
(csrc/attn_decode.hip through the table in every layer, csrc/beam_step.hip per token), built as
``test_generate_gpu.py`` builds it (tests/beam_search_helpers.py holds the checks)."""
import functools

import pytest
import torch

import beam_search_helpers as bsh
from decode_helpers import TINY
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.parallel.ddp import DDPEngine

pytestmark = pytest.mark.gpu

VOCAB = TINY["vocab_size"]


@functools.lru_cache(maxsize=None)
def _model(heads):
    torch.manual_seed(0)
    nat = build_model(precision="bf16", num_heads=heads, **TINY).cuda().eval()
    eng = DDPEngine(nat, shadow_dtype=torch.bfloat16)  # attaches the bf16 weight shadows
    return nat, eng


@pytest.mark.parametrize("heads", [4, 2])
def test_one_beam_is_greedy_generate(heads):
    bsh.check_one_beam_is_greedy(_model(heads)[0], "cuda", VOCAB)


@pytest.mark.parametrize("heads,W", [(4, 2), (4, 4), (2, 4)])
def test_equals_a_search_that_reorders_the_cache(heads, W):
    """The table kernel folds the same values in the same order as the plain kernel on a gathered
    cache, so tokens, lengths and scores are equal exactly."""
    bsh.check_against_reordering(_model(heads)[0], "cuda", VOCAB, W)


def test_scores_are_the_teacher_forced_log_probabilities():
    """The bound is four times the greedy path's own difference, measured in the same run (one beam
    is ``generate(temperature=0)`` and comes with its score; with and without ``eos_id``, so on rows
    that stop early and on rows that run all 24 tokens).  Measured on the MI355X: beams (W = 4, 12
    hypotheses) 1.54e-05, greedy path (6 hypotheses) 8.78e-06, at |score| near 150 where one fp32
    ulp is 1.53e-05.  On this stack the logits of a decode step do not depend on the rows beside it,
    so both figures are rounding alone: of each step's ``logp`` term and of the one final rounding
    of the float64 sum.  (With the scores taken from ``beam_step``'s fp32 running sums instead, the
    beams' figure was 4.59e-05, three ulps of 24 fp32 additions, over the bound of 3.51e-05: that
    is why ``beam_search`` adds the terms up in float64.)"""
    d_beam, d_greedy = bsh.check_scores_against_teacher_forcing(_model(4)[0], "cuda", VOCAB, 4)
    print(f"beam_search gpu: max |score - teacher forced| = {d_beam:.3e}, greedy path {d_greedy:.3e}")
    assert d_beam <= 4 * d_greedy, (d_beam, d_greedy)


@pytest.mark.parametrize("W", [2, 4])
def test_ordering_and_lengths(W):
    bsh.check_ordering_and_lengths(_model(4)[0], "cuda", VOCAB, W)


def test_cache_and_table_invariants():
    bsh.check_cache_and_table(_model(4)[0], "cuda", VOCAB, 3)
