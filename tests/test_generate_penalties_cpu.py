"""The logit processors in ``GPT2LMModel.generate`` / ``beam_search`` and in ``run.generate`` on the CPU
(fp32 PyTorch paths throughout) on the ``TINY`` model; tests/penalty_helpers.py holds the checks."""
import json

import pytest
import torch

import penalty_helpers as ph
from decode_helpers import TINY
from distributed_pipeline_amd.models import build_model

VOCAB = TINY["vocab_size"]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(precision="fp32", num_heads=4, **TINY).eval()


def test_generate_equals_the_written_out_loop(model):
    ph.check_generate_equals_the_written_out_loop(model, "cpu", VOCAB)


def test_no_repeat_ngram_ends_the_repeats(model):
    ph.check_no_repeat_ngram(model, "cpu", VOCAB)


def test_min_new_tokens_holds_off_eos(model):
    ph.check_min_new_tokens(model, "cpu", VOCAB)


def test_penalize_prompt_is_the_window(model):
    ph.check_penalize_prompt_is_the_window(model, "cpu", VOCAB)


@pytest.mark.parametrize("W", [2, 4])
def test_beam_search_equals_a_search_that_reorders_histories(model, W):
    ph.check_beam_search_equals_the_reordering_search(model, "cpu", VOCAB, W)


def test_default_keywords_are_the_calls_without_them(model):
    ph.check_defaults_are_the_calls_without(model, "cpu", VOCAB)


def test_lookahead_raises(model):
    ph.check_lookahead_raises(model, "cpu", VOCAB)


# ---- run.generate --------------------------------------------------------------------------------

COMMON = ["--model", "gpt2", "--config_name", "tiny", "--hidden_size", "64", "--num_layers", "2", "--num_heads", "2",
          "--vocab_size", "200", "--seq_len", "32", "--dropout", "0.0", "--precision", "fp32", "--dataset", "synthetic",
          "--batch_size", "3", "--num_batches", "2", "--prompt_len", "8", "--max_new_tokens", "12"]
EXPLICIT_DEFAULTS = ["--repetition_penalty", "1.0", "--presence_penalty", "0.0", "--frequency_penalty", "0.0",
                     "--no_repeat_ngram", "0", "--min_new_tokens", "0", "--penalize_prompt", "true"]


def _generate(*extra):
    from run import generate
    return generate.main(generate.create_parser().parse_args([*COMMON, *extra]))


def test_run_generate_with_the_flags(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # this file is about the CPU paths
    torch.manual_seed(0)
    net = build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2, vocab_size=200,
                      seq_len=32, dropout=0.0, precision="fp32")
    ck = tmp_path / "model_000002.pt"
    torch.save(net.state_dict(), ck)

    def rows(name, *extra):
        out = tmp_path / name
        _generate("--model_path", str(ck), "--out_path", str(out), *extra)
        return out.read_bytes()

    def conts(data):
        return [json.loads(line) for line in data.splitlines()]

    plain = rows("a.jsonl", "--temperature", "0")
    assert rows("b.jsonl", "--temperature", "0", *EXPLICIT_DEFAULTS) == plain  # the same bytes as without the flags
    sampled = rows("c.jsonl", "--noise", "philox", "--top_k", "20")
    assert rows("d.jsonl", "--noise", "philox", "--top_k", "20", *EXPLICIT_DEFAULTS) == sampled

    held = conts(rows("e.jsonl", "--temperature", "0", "--no_repeat_ngram", "2", "--repetition_penalty", "1.2",
                      "--presence_penalty", "0.1", "--frequency_penalty", "0.1"))
    assert len(held) == 6 and held != conts(plain)
    for row in held:
        assert len(row["continuation"]) == 12
        assert ph.repeated_ngrams(row["prompt"], row["continuation"], 2) == 0
    assert sum(ph.repeated_ngrams(r["prompt"], r["continuation"], 2) for r in conts(plain)) > 0

    eos = conts(plain)[0]["continuation"][0]
    cut = conts(rows("f.jsonl", "--temperature", "0", "--eos_id", str(eos)))
    assert cut[0]["continuation"] == []
    late = conts(rows("g.jsonl", "--temperature", "0", "--eos_id", str(eos), "--min_new_tokens", "4"))
    assert all(len(r["continuation"]) >= 4 for r in late)

    # with sampling, philox noise and beams
    for i, extra in enumerate([("--top_k", "10", "--top_p", "0.9"), ("--noise", "philox", "--top_p", "0.8"),
                               ("--num_beams", "3"), ("--num_beams", "2", "--penalize_prompt", "false")]):
        got = conts(rows(f"h{i}.jsonl", *extra, "--no_repeat_ngram", "3", "--repetition_penalty", "1.1"))
        assert len(got) == 6
        for row in got:
            assert ph.repeated_ngrams(row["prompt"] if "false" not in extra else [], row["continuation"], 3) == 0


@pytest.mark.parametrize("extra,match", [
    (("--repetition_penalty", "0"), "repetition_penalty"), (("--repetition_penalty", "-1.5"), "repetition_penalty"),
    (("--no_repeat_ngram", "-1"), "no_repeat_ngram"), (("--min_new_tokens", "-1", "--eos_id", "3"), "min_new_tokens"),
    (("--min_new_tokens", "13", "--eos_id", "3"), "min_new_tokens"), (("--min_new_tokens", "2"), "eos_id"),
    (("--lookahead", "4", "--temperature", "0", "--repetition_penalty", "1.2"), "lookahead"),
    (("--lookahead", "4", "--temperature", "0", "--presence_penalty", "0.5"), "lookahead"),
    (("--lookahead", "4", "--temperature", "0", "--frequency_penalty", "0.5"), "lookahead"),
    (("--lookahead", "4", "--temperature", "0", "--no_repeat_ngram", "2"), "lookahead"),
    (("--lookahead", "4", "--temperature", "0", "--min_new_tokens", "2", "--eos_id", "3"), "lookahead"),
    (("--lookahead", "4", "--temperature", "0", "--penalize_prompt", "false"), "lookahead")])
def test_run_generate_rejects_before_a_checkpoint_is_read(tmp_path, monkeypatch, extra, match):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    missing = tmp_path / "no_such_dir" / "model_000002.pt"
    with pytest.raises(ValueError, match=match):
        _generate("--model_path", str(missing), *extra)
    # the same path with accepted flags gets as far as looking for the checkpoint
    with pytest.raises(FileNotFoundError):
        _generate("--model_path", str(missing), "--repetition_penalty", "1.2", "--no_repeat_ngram", "2")
