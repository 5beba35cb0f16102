"""Distinct n-gram counts on the CPU (the PyTorch path of ``ops.text.ngram_distinct``), the dist-n /
div-n metrics of utils/diversity.py and ``python -m run.eval --diversity true``.  Every comparison
is exact; the oracle is Python sets of n-gram tuples."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_pipeline_amd.ops import text
from distributed_pipeline_amd.ops.text import ngram_distinct
from utils.diversity import dist_n, dist_n_batch, distinct_ngrams, div_n, div_n_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def set_counts(seqs):
    """[K + 1][4] distinct n-gram counts of the id lists ``seqs`` and of their union, by inline sets."""
    rows = [[len({tuple(s[i:i + n]) for i in range(len(s) - n + 1)}) for n in range(1, 5)] for s in seqs]
    rows.append([len({tuple(s[i:i + n]) for s in seqs for i in range(len(s) - n + 1)}) for n in range(1, 5)])
    return rows


def random_groups(G, K, L, vocab, seed, poison="inside"):
    """tokens [G, K, L], lens [G, K] with the lengths 0, 1, 2, 3 and L forced in, ids in [0, vocab)
    and the tails beyond each length poisoned: with ids that also occur inside it or with -1."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, vocab, (G, K, L), generator=g)
    lens = torch.randint(0, L + 1, (G, K), generator=g)
    flat = lens.view(-1)
    for at, n in enumerate((0, 1, 2, 3, L)):
        flat[(at * 7) % flat.numel()] = min(n, L)
    if poison == "minus_one":
        tokens[torch.arange(L).view(1, 1, L) >= lens.unsqueeze(-1)] = -1
    return tokens, lens


def lists_of(tokens, lens):
    G, K, _ = tokens.shape
    return [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(G)]


def oracle(tokens, lens):
    G, K, _ = tokens.shape
    return torch.tensor([set_counts(grp) for grp in lists_of(tokens, lens)], dtype=torch.int32).reshape(G, K + 1, 4)


SHAPES = [(3, 2, 1, 3), (5, 3, 7, 3), (4, 10, 64, 4), (2, 16, 130, 5), (70, 4, 33, 3), (3, 1, 9, 2),
          (1, 16, 256, 2), (2, 17, 5, 3), (2, 2, 257, 3)]


@pytest.mark.parametrize("G,K,L,vocab", SHAPES)
def test_fallback_against_the_set_oracle(G, K, L, vocab):
    tokens, lens = random_groups(G, K, L, vocab, seed=G * 1000 + K * 100 + L)
    d = ngram_distinct(tokens, lens)
    want = oracle(tokens, lens)
    assert d.dtype == torch.int32 and d.shape == (G, K + 1, 4)
    assert torch.equal(d, want)
    assert torch.equal(text._ngram_distinct_torch(tokens, lens.clamp(0, L)), want)
    # the list versions count the same
    for grp, rows in zip(lists_of(tokens, lens), want.tolist()):
        assert [[distinct_ngrams(s, n) for n in range(1, 5)] for s in grp] == rows[:-1]
    # the invariants of the definition
    n = torch.arange(1, 5).view(1, 1, 4)
    per, uni = d[:, :K].long(), d[:, K].long()
    assert bool((per <= (lens.unsqueeze(-1) - n + 1).clamp_min(0)).all())
    assert bool((per.max(1).values <= uni).all()) and bool((uni <= per.sum(1)).all())
    if K == 1:
        assert torch.equal(d[:, 1], d[:, 0])
    assert int(ngram_distinct(tokens, torch.zeros_like(lens)).abs().sum()) == 0
    if G * K * L > 2000:
        return
    # int32 ids, a non-contiguous view, lengths beyond [0, L], -1 beyond the lengths: the same counts
    assert torch.equal(ngram_distinct(tokens.to(torch.int32), lens.to(torch.int32)), d)
    wide = torch.full((G, K, 2 * L), vocab - 1, dtype=tokens.dtype)
    wide[:, :, ::2] = tokens
    assert torch.equal(ngram_distinct(wide[:, :, ::2], lens), d)
    over = torch.where(lens == L, lens + 5, torch.where(lens == 0, lens - 3, lens))
    assert torch.equal(ngram_distinct(tokens, over), d)
    t2, l2 = random_groups(G, K, L, vocab, seed=G * 1000 + K * 100 + L, poison="minus_one")
    assert torch.equal(l2, lens) and torch.equal(ngram_distinct(t2, l2), d)


def test_fallback_is_chunked_over_groups(monkeypatch):
    tokens, lens = random_groups(9, 3, 8, 3, seed=5)
    whole = ngram_distinct(tokens, lens)
    assert torch.equal(whole, oracle(tokens, lens))
    monkeypatch.setattr(text, "_FALLBACK_ELEMS", 2 * 3 * 3 * 8 * 8)  # two groups per chunk, a last one alone
    assert torch.equal(ngram_distinct(tokens, lens), whole)


def test_empty_shapes_give_zeros():
    for shape in [(0, 3, 8), (4, 0, 8), (4, 3, 0)]:
        d = ngram_distinct(torch.zeros(shape, dtype=torch.long), torch.zeros(shape[:2], dtype=torch.long))
        assert d.shape == (shape[0], shape[1] + 1, 4) and d.dtype == torch.int32 and int(d.abs().sum()) == 0
    with pytest.raises(ValueError):
        ngram_distinct(torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        ngram_distinct(torch.zeros(2, 3, 4, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long))


def test_order_independence():
    tokens, lens = random_groups(6, 5, 12, 3, seed=9)
    d = ngram_distinct(tokens, lens)
    perm = torch.tensor([3, 0, 4, 2, 1])
    dp = ngram_distinct(tokens[:, perm], lens[:, perm])
    assert torch.equal(dp[:, :5], d[:, perm]) and torch.equal(dp[:, 5], d[:, 5])


def test_hand_values():
    assert distinct_ngrams([1, 2, 1, 2, 1], 2) == 2 and dist_n([1, 2, 1, 2, 1], 2) == 2 / 4
    assert div_n([[1, 2, 3], [1, 2, 3], [3, 2, 1]], 2) == 4 / 6
    assert dist_n([1, 2, 1, 2, 1], 1) == 2 / 5 and dist_n([1, 2, 3], 3) == 1.0
    for n in range(1, 5):
        assert dist_n([], n) == 0.0 == div_n([], n) == div_n([[], []], n)
        assert distinct_ngrams([], n) == 0
    assert dist_n([1, 2, 3], 4) == 0.0 == div_n([[1, 2, 3], [4]], 4)
    assert div_n([[1, 2, 3], [4]], 1) == 4 / 4 and div_n([[7, 7, 7, 7, 7], [7, 7, 7, 7]], 4) == 1 / 3


@pytest.mark.parametrize("G,K,L,vocab", [(12, 4, 10, 3), (9, 6, 14, 4), (5, 1, 6, 3), (6, 3, 5, 2)])
def test_batch_forms_equal_the_list_versions(G, K, L, vocab):
    tokens, lens = random_groups(G, K, L, vocab, seed=K * 10 + L)
    for g in range(0, G, 2):  # duplicates (other junk beyond the length) and an empty candidate
        n = int(lens[g, 0])
        tokens[g, K - 1, :n] = tokens[g, 0, :n]
        lens[g, K - 1] = n
    lens[1, 0] = 0
    lists = lists_of(tokens, lens)
    dist, div = dist_n_batch(tokens, lens), div_n_batch(tokens, lens)
    assert dist.dtype == torch.float64 and dist.shape == (G, K, 4) and not dist.is_cuda
    assert div.dtype == torch.float64 and div.shape == (G, 4) and not div.is_cuda
    assert torch.equal(dist, torch.tensor([[[dist_n(s, n) for n in range(1, 5)] for s in grp] for grp in lists],
                                          dtype=torch.float64))
    assert torch.equal(div, torch.tensor([[div_n(grp, n) for n in range(1, 5)] for grp in lists],
                                         dtype=torch.float64))


def test_unigram_count_is_the_dist1_of_run_eval():
    tokens, lens = random_groups(40, 1, 23, 6, seed=2)
    d = ngram_distinct(tokens, lens)[:, 0, 0].tolist()
    for (rec,), d1 in zip(lists_of(tokens, lens), d):
        today = len(set(rec)) / len(rec) if rec else 0.0
        assert today == (d1 / len(rec) if rec else 0.0) == dist_n(rec, 1)


ROWS = [
    {"source": [9], "reference": [1, 2, 3, 5], "recover": [1, 2, 3, 4, 1, 2, 3, 4, 1],
     "candidates": [[1, 2, 3, 4, 1, 2, 3, 4, 1], [1, 2, 3, 4, 5, 6], [1, 2]]},
    {"source": [9], "reference": [1, 2, 3, 4], "recover": [1, 2, 3, 4],
     "candidates": [[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]]},
    {"source": [9], "reference": [1, 2], "recover": [],
     "candidates": [[], [7, 7], [7, 8]]},
    {"source": [9], "reference": [1, 2], "recover": [5, 5, 5, 5, 5, 6],
     "candidates": [[5, 5, 5, 5, 5, 6], [5, 5, 5, 5, 5]]},
    {"source": [9], "reference": [3], "recover": [3, 3], "candidates": [[3, 3]]},
]
PLAIN_KEYS = {"n", "bleu", "len", "dist1", "self_bleu"}


def _write(tmp_path, rows, name="out.jsonl"):
    path = tmp_path / name
    path.write_text("".join(json.dumps(r) + "\n" for r in rows))
    return path


def _mean(xs):
    return sum(xs) / len(xs)


def _check_diversity(out):
    for n in (2, 3, 4):
        assert out[f"dist{n}"] == _mean([dist_n(r["recover"], n) for r in ROWS])
    multi = [r["candidates"] for r in ROWS if len(r["candidates"]) > 1]  # K = 3 rows first, then K = 2
    assert len(multi) == 4
    assert out["div4"] == _mean([div_n(c, 4) for c in multi])
    assert out["dist4"] > 0.0 and out["div4"] > 0.0
    assert out["dist1"] == _mean([dist_n(r["recover"], 1) for r in ROWS])


def test_run_eval_diversity_on_a_hand_written_file(tmp_path):
    path = _write(tmp_path, ROWS)
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "run.eval", "--path", str(path), "--diversity", "true"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == PLAIN_KEYS | {"dist2", "dist3", "dist4", "div4"}
    _check_diversity(out)


def test_run_eval_main_flag_combinations(tmp_path, capsys):
    from run.eval import create_parser, evaluate, main
    path = str(_write(tmp_path, ROWS))
    # without the flag: exactly today's keys and values
    plain = main(create_parser().parse_args(["--path", path]))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == plain
    assert set(plain) == PLAIN_KEYS
    assert plain == evaluate(ROWS, torch.device("cpu"), 4096, False)
    # with it: the same numbers plus the four new ones, in small batches as well
    out = main(create_parser().parse_args(["--path", path, "--diversity", "true", "--batch_size", "2"]))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert set(out) == PLAIN_KEYS | {"dist2", "dist3", "dist4", "div4"}
    _check_diversity(out)
    assert {k: out[k] for k in ("n", "bleu", "len", "dist1")} == {k: plain[k] for k in ("n", "bleu", "len", "dist1")}
    # combined with --rouge_l true: both groups of keys
    both = main(create_parser().parse_args(["--path", path, "--diversity", "true", "--rouge_l", "true"]))
    assert set(both) == PLAIN_KEYS | {"rouge_l", "self_rouge_l", "dist2", "dist3", "dist4", "div4"}
    _check_diversity(both)
    assert both == evaluate(ROWS, torch.device("cpu"), 4096, True, True)
    # rows without candidates (or with one): no div4
    bare = [{k: v for k, v in r.items() if k != "candidates"} for r in ROWS[:3]] + [ROWS[4]]
    out2 = evaluate(bare, torch.device("cpu"), diversity=True)
    assert set(out2) == {"n", "bleu", "len", "dist1", "dist2", "dist3", "dist4"}
    assert out2["dist2"] == _mean([dist_n(r["recover"], 2) for r in bare])


def test_eval_settings_carry_the_flag():
    from config.eval import EvalSettings
    e = EvalSettings.from_argparse(EvalSettings.to_argparse().parse_args(["--path", "x.jsonl"]))
    assert e.diversity is False
    e = EvalSettings.from_argparse(EvalSettings.to_argparse().parse_args(["--path", "x.jsonl", "--diversity", "true"]))
    assert e.diversity is True and EvalSettings(**json.loads(e.json())) == e
