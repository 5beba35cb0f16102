"""The logit processors in ``GPT2LMModel.generate`` / ``beam_search`` on the GPU: the ``TINY`` model in
bf16 on the native kernels (csrc/logit_penalty.hip on every step's logits), built as
``test_generate_gpu.py`` builds it, with 4 heads (D = 64) and 2 heads (D = 128);
tests/penalty_helpers.py holds the checks."""
import functools

import pytest
import torch

import penalty_helpers as ph
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
def test_generate_equals_the_written_out_loop(heads):
    ph.check_generate_equals_the_written_out_loop(_model(heads)[0], "cuda", VOCAB)


@pytest.mark.parametrize("heads", [4, 2])
def test_no_repeat_ngram_ends_the_repeats(heads):
    ph.check_no_repeat_ngram(_model(heads)[0], "cuda", VOCAB)


def test_min_new_tokens_holds_off_eos():
    ph.check_min_new_tokens(_model(4)[0], "cuda", VOCAB)


def test_penalize_prompt_is_the_window():
    ph.check_penalize_prompt_is_the_window(_model(4)[0], "cuda", VOCAB)


@pytest.mark.parametrize("heads,W", [(4, 2), (4, 4), (2, 4)])
def test_beam_search_equals_a_search_that_reorders_histories(heads, W):
    ph.check_beam_search_equals_the_reordering_search(_model(heads)[0], "cuda", VOCAB, W)


def test_default_keywords_are_the_calls_without_them():
    ph.check_defaults_are_the_calls_without(_model(4)[0], "cuda", VOCAB)


def test_lookahead_raises():
    ph.check_lookahead_raises(_model(4)[0], "cuda", VOCAB)
