"""``GPT2LMModel.beam_search`` on the CPU (fp32 PyTorch paths throughout) on the ``TINY`` model, and
``python -m run.generate --num_beams`` (tests/beam_search_helpers.py holds the checks)."""
import json

import pytest
import torch

import beam_search_helpers as bsh
from decode_helpers import TINY
from distributed_pipeline_amd.models import build_model

VOCAB = TINY["vocab_size"]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(precision="fp32", num_heads=4, **TINY).eval()


def test_one_beam_is_greedy_generate(model):
    bsh.check_one_beam_is_greedy(model, "cpu", VOCAB)


@pytest.mark.parametrize("W", [2, 4])
def test_equals_a_search_that_reorders_the_cache(model, W):
    bsh.check_against_reordering(model, "cpu", VOCAB, W)


def test_scores_are_the_teacher_forced_log_probabilities(model):
    """The bound is four times the greedy path's own difference, measured in the same run (one beam
    is ``generate(temperature=0)`` and comes with its score; with and without ``eos_id``, so on rows
    that stop early and on rows that run all 24 tokens).  Measured on this model and these prompts
    (fp32): beams (W = 4) 6.86e-06, greedy path 9.20e-06 - the rounding of each step's ``logp`` term
    and of the one final rounding of their float64 sum, at |score| near 150."""
    d_beam, d_greedy = bsh.check_scores_against_teacher_forcing(model, "cpu", VOCAB, 4)
    print(f"beam_search cpu: max |score - teacher forced| = {d_beam:.3e}, greedy path {d_greedy:.3e}")
    assert d_beam <= 4 * d_greedy, (d_beam, d_greedy)


@pytest.mark.parametrize("W", [2, 4])
def test_ordering_and_lengths(model, W):
    bsh.check_ordering_and_lengths(model, "cpu", VOCAB, W)


def test_cache_and_table_invariants(model):
    bsh.check_cache_and_table(model, "cpu", VOCAB, 3)


# ---- run.generate --------------------------------------------------------------------------------

COMMON = ["--model", "gpt2", "--config_name", "tiny", "--hidden_size", "64", "--num_layers", "2", "--num_heads", "2",
          "--vocab_size", "200", "--seq_len", "32", "--dropout", "0.0", "--precision", "fp32", "--dataset", "synthetic",
          "--batch_size", "3", "--num_batches", "2", "--prompt_len", "8", "--max_new_tokens", "6"]


def _generate(*extra):
    from run import generate
    return generate.main(generate.create_parser().parse_args([*COMMON, *extra]))


def test_run_generate_with_beams(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # this file is about the CPU paths
    torch.manual_seed(0)
    net = build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2, vocab_size=200,
                      seq_len=32, dropout=0.0, precision="fp32")
    ck = tmp_path / "model_000001.pt"
    torch.save(net.state_dict(), ck)

    def rows(name, *extra):
        out = tmp_path / name
        _generate("--model_path", str(ck), "--out_path", str(out), "--temperature", "0", *extra)
        return out.read_bytes()

    plain = rows("a.jsonl")
    assert rows("b.jsonl", "--num_beams", "1") == plain  # the same bytes as without the flag
    beams = [json.loads(line) for line in rows("c.jsonl", "--num_beams", "3", "--keep_beams", "true").splitlines()]
    assert len(beams) == 6
    for row, ref in zip(beams, [json.loads(line) for line in plain.splitlines()]):
        assert set(row) == {"prompt", "continuation", "reference", "beams", "beam_scores"}
        assert row["prompt"] == ref["prompt"] and row["reference"] == ref["reference"]
        assert len(row["beams"]) == len(row["beam_scores"]) == 3 and row["continuation"] == row["beams"][0]
        assert all(a >= b for a, b in zip(row["beam_scores"], row["beam_scores"][1:]))
        assert all(isinstance(i, int) and 0 <= i < 200 for b in row["beams"] for i in b)
    lean = [json.loads(line) for line in rows("d.jsonl", "--num_beams", "3").splitlines()]
    assert [set(r) for r in lean] == [{"prompt", "continuation", "reference"}] * 6
    assert [r["continuation"] for r in lean] == [r["continuation"] for r in beams]


@pytest.mark.parametrize("extra", [("--num_beams", "0"), ("--num_beams", "2", "--top_k", "5"),
                                   ("--num_beams", "2", "--top_p", "0.9"), ("--num_beams", "2", "--noise", "philox"),
                                   ("--num_beams", "300"), ("--num_beams", "200", "--batch_size", "1000000")])
def test_run_generate_rejects_before_a_checkpoint_is_read(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    missing = tmp_path / "no_such_dir" / "model_000001.pt"
    with pytest.raises(ValueError, match="num_beams"):
        _generate("--model_path", str(missing), *extra)
    # the same path with accepted flags gets as far as looking for the checkpoint
    with pytest.raises(FileNotFoundError):
        _generate("--model_path", str(missing), "--num_beams", "2")
