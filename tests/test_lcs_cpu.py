"""LCS lengths on the CPU (the PyTorch path of ``ops.text.lcs_lengths``), ROUGE-L (utils/rouge.py),
MBR selection by ROUGE-L, ``python -m run.eval --rouge_l true`` and ``run.sample --mbr_metric``.
Every comparison is exact; the oracle is the textbook dynamic programme ``utils.rouge.lcs_length``."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_pipeline_amd.ops import text
from distributed_pipeline_amd.ops.text import lcs_lengths
from utils.mbr import mbr_select, mbr_select_batch
from utils.rouge import lcs_length, pairwise_rouge_l, rouge_l, rouge_l_from_lcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_groups(G, K, L, vocab, seed):
    """tokens [G, K, L], lens [G, K] with the lengths 0, 1, 63, 64, 65 and L forced in where L
    allows them, ids in [0, vocab), the tails holding ids that also occur inside the lengths."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, vocab, (G, K, L), generator=g)
    lens = torch.randint(0, L + 1, (G, K), generator=g)
    flat = lens.view(-1)
    for at, n in enumerate(n for n in (0, 1, 63, 64, 65, L) if n <= L):
        flat[(at * 5) % flat.numel()] = n
    return tokens, lens


def lists_of(tokens, lens):
    G, K, _ = tokens.shape
    return [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(G)]


def oracle(tokens, lens):
    G, K, _ = tokens.shape
    want = torch.zeros(G, K, K, dtype=torch.int32)
    for g, grp in enumerate(lists_of(tokens, lens)):
        for i in range(K):
            for j in range(i, K):
                want[g, i, j] = want[g, j, i] = lcs_length(grp[i], grp[j])
    return want


@pytest.mark.parametrize("G,K,L,vocab", [(3, 2, 1, 3), (5, 3, 7, 3), (2, 16, 20, 3), (3, 1, 9, 2), (2, 3, 70, 3)])
def test_fallback_against_the_dynamic_programme(G, K, L, vocab):
    tokens, lens = random_groups(G, K, L, vocab, seed=G * 100 + L)
    want = oracle(tokens, lens)
    out = lcs_lengths(tokens, lens)
    assert out.dtype == torch.int32 and out.shape == (G, K, K)
    assert torch.equal(out, want)
    assert torch.equal(text._lcs_lengths_torch(tokens, lens.to(torch.int32)), want)
    assert torch.equal(out, out.transpose(1, 2))
    assert torch.equal(torch.diagonal(out, dim1=1, dim2=2), lens.to(torch.int32))
    # int32 ids, a non-contiguous view, lengths beyond [0, L], -1 beyond the lengths: the same lengths
    assert torch.equal(lcs_lengths(tokens.to(torch.int32), lens.to(torch.int32)), want)
    wide = torch.full((G, K, 2 * L), vocab - 1, dtype=tokens.dtype)
    wide[:, :, ::2] = tokens
    assert torch.equal(lcs_lengths(wide[:, :, ::2], lens), want)
    over = torch.where(lens == L, lens + 5, torch.where(lens == 0, lens - 3, lens))
    assert torch.equal(lcs_lengths(tokens, over), want)
    beyond = torch.arange(L).view(1, 1, L) >= lens.unsqueeze(-1)
    assert torch.equal(lcs_lengths(tokens.masked_fill(beyond, -1), lens), want)
    assert int(lcs_lengths(tokens, torch.zeros_like(lens)).abs().sum()) == 0


def test_fallback_is_chunked_over_groups(monkeypatch):
    tokens, lens = random_groups(9, 3, 8, 3, seed=5)
    whole = lcs_lengths(tokens, lens)
    monkeypatch.setattr(text, "_FALLBACK_ELEMS", 2 * 3 * 3 * 9)  # two groups per chunk, a last one alone
    assert torch.equal(lcs_lengths(tokens, lens), whole)
    assert lcs_lengths(tokens[:0], lens[:0]).shape == (0, 3, 3)


def test_argument_checks():
    with pytest.raises(ValueError):
        lcs_lengths(torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        lcs_lengths(torch.zeros(2, 3, 4, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(ValueError):
        lcs_lengths(torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.long))


def test_hand_values():
    assert lcs_length([1, 2, 3, 4], [1, 2, 3, 5]) == 3
    assert lcs_length([], [1, 2]) == 0 == lcs_length([1, 2], []) == lcs_length([], [])
    assert lcs_length([1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1]) == 1
    assert lcs_length([1, 3, 5, 7, 9, 1], [9, 1, 3, 7, 1, 5]) == 4  # 1 3 7 1
    assert lcs_length("ABCBDAB", "BDCABA") == 4
    assert rouge_l([1, 2, 3, 4], [1, 2, 3, 5]) == 0.75 == rouge_l_from_lcs(3, 4, 4)
    assert rouge_l([], [1, 2]) == 0.0 == rouge_l([1, 2], []) == rouge_l([], [])
    assert rouge_l_from_lcs(0, 0, 0) == 0.0 == rouge_l_from_lcs(0, 3, 0) == rouge_l([7, 8], [1, 2])
    a = [4, 4, 2, 9, 1]
    assert rouge_l(a, a) == 1.0
    # precision 2 / 2, recall 2 / 4
    assert rouge_l([1, 2], [1, 2, 3, 4]) == 2 * 1.0 * 0.5 / 1.5 == rouge_l_from_lcs(2, 2, 4)


def groups_with_duplicates(G, K, L, vocab, seed):
    """Random groups where some candidates are copies of another (with other junk beyond the
    length) and some are empty."""
    tokens, lens = random_groups(G, K, L, vocab, seed)
    for g in range(G):
        if K > 1 and g % 2 == 0:
            src, dst = g % K, (g + 1 + g // K) % K
            n = int(lens[g, src])
            tokens[g, dst, :n] = tokens[g, src, :n]
            lens[g, dst] = n
        if K > 2 and g % 3 == 0:
            lens[g, (g + 2) % K] = 0
    return tokens, lens


@pytest.mark.parametrize("G,K,L,vocab", [(12, 4, 10, 3), (9, 6, 14, 4), (5, 1, 6, 3), (6, 3, 5, 2)])
def test_mbr_select_batch_equals_mbr_select_for_both_metrics(G, K, L, vocab):
    tokens, lens = groups_with_duplicates(G, K, L, vocab, seed=K * 10 + L)
    lists = lists_of(tokens, lens)
    assert mbr_select_batch(tokens, lens, metric="rouge_l") == [mbr_select(c, metric="rouge_l") for c in lists]
    # the default metric is BLEU, as before the argument existed
    bleu = [mbr_select(c) for c in lists]
    assert mbr_select_batch(tokens, lens) == bleu == mbr_select_batch(tokens, lens, metric="bleu")
    assert [mbr_select(c, metric="bleu") for c in lists] == bleu
    pr = pairwise_rouge_l(tokens, lens)
    assert pr.dtype == torch.float64 and pr.shape == (G, K, K)
    assert pr.tolist() == [[[rouge_l(a, b) for b in c] for a in c] for c in lists]


def test_mbr_select_metrics_ties_empties_and_unknown():
    A, B = [5, 6, 7, 8, 9], [5, 6, 1, 2, 3]
    groups = [[A, A, B], [B, A, A], [A, A, A], [[], [], []]]
    tokens = torch.tensor([[s + [9] * (5 - len(s)) for s in grp] for grp in groups])
    lens = torch.tensor([[len(s) for s in grp] for grp in groups])
    for metric in ("bleu", "rouge_l"):
        assert mbr_select_batch(tokens, lens, metric=metric) == [0, 1, 0, 0]
        assert [mbr_select(grp, metric=metric) for grp in groups] == [0, 1, 0, 0]
    assert mbr_select_batch(tokens, lens) == [0, 1, 0, 0] == [mbr_select(grp) for grp in groups]
    # Q and R share nothing; each shares a scattered subsequence of 3 with P: the last one wins
    P, Q, R = [1, 2, 3, 4, 5, 6], [1, 7, 2, 7, 3, 7], [8, 4, 8, 5, 8, 6]
    assert mbr_select([Q, R, P], metric="rouge_l") == 2 == mbr_select_batch(
        torch.tensor([[Q, R, P]]), torch.tensor([[6, 6, 6]]), metric="rouge_l")[0]
    with pytest.raises(ValueError):
        mbr_select(groups[0], metric="meteor")
    with pytest.raises(ValueError):
        mbr_select_batch(tokens, lens, metric="meteor")


def _f(lcs, len_h, len_r):
    p, r = lcs / len_h, lcs / len_r
    return 2 * p * r / (p + r)


def test_run_eval_rouge_l_on_a_hand_written_file(tmp_path):
    rows = [
        {"source": [9], "reference": [1, 2, 3, 5], "recover": [1, 2, 3, 4],
         "candidates": [[1, 2, 3, 4], [1, 2, 3, 5], [1, 2]]},
        {"source": [9], "reference": [1, 2, 3, 4], "recover": [1, 2, 3, 4],
         "candidates": [[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]]},
        {"source": [9], "reference": [1, 2], "recover": [],
         "candidates": [[], [7, 7], [7, 8]]},
    ]
    path = tmp_path / "out.jsonl"
    path.write_text("".join(json.dumps(r) + "\n" for r in rows))
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "run.eval", "--path", str(path), "--rouge_l", "true"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"n", "bleu", "len", "dist1", "self_bleu", "rouge_l", "self_rouge_l"}
    # by hand: LCS 3 of 4 and 4 tokens; identical; an empty hypothesis
    assert out["rouge_l"] == (0.75 + 1.0 + 0.0) / 3
    # the candidates' LCS lengths by hand, [i][j]; an empty candidate scores 0 against everything
    lcs = [[[4, 3, 2], [3, 4, 2], [2, 2, 2]], [[4, 4, 4]] * 3, [[0, 0, 0], [0, 2, 1], [0, 1, 2]]]
    lens = [[4, 4, 2], [4, 4, 4], [0, 2, 2]]
    selfs = [sum(_f(c[i][j], n[i], n[j]) if c[i][j] else 0.0 for i in range(3) for j in range(3) if i != j) / 6
             for c, n in zip(lcs, lens)]
    assert selfs[1] == 1.0 and selfs[2] == (0.5 + 0.5) / 6
    assert out["self_rouge_l"] == sum(selfs) / 3
    # without the flag: exactly the keys and values of before; in-process, and rows without candidates
    from run.eval import create_parser, evaluate, main
    plain = main(create_parser().parse_args(["--path", str(path)]))
    assert set(plain) == {"n", "bleu", "len", "dist1", "self_bleu"}
    assert all(plain[k] == out[k] for k in plain)
    assert evaluate(rows, torch.device("cpu")) == plain
    bare = [{k: v for k, v in r_.items() if k != "candidates"} for r_ in rows]
    out2 = evaluate(bare, torch.device("cpu"), batch_size=2, rouge_l=True)
    assert set(out2) == {"n", "bleu", "len", "dist1", "rouge_l"} and out2["rouge_l"] == out["rouge_l"]


def test_settings_round_trip_the_new_fields(tmp_path):
    from config.eval import EvalSettings
    from config.sample import SampleSettings
    from config.train import TrainSettings
    s = SampleSettings()
    assert s.mbr_metric == "bleu" and "mbr_metric" not in TrainSettings.model_fields
    p = SampleSettings.to_argparse(add_json=True)
    s = SampleSettings.from_argparse(p.parse_args(["--mbr", "3", "--mbr_metric", "rouge_l"]))
    assert (s.mbr, s.mbr_metric) == (3, "rouge_l")
    assert SampleSettings(**json.loads(s.json())).mbr_metric == "rouge_l"
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"mbr_metric": "rouge_l", "lr": 1e-4}))  # lr: a key only training reads
    assert SampleSettings.from_argparse(p.parse_args(["--config_json", str(cfg)])).mbr_metric == "rouge_l"
    assert SampleSettings.from_argparse(
        p.parse_args(["--config_json", str(cfg), "--mbr_metric", "bleu"])).mbr_metric == "bleu"
    with pytest.raises(SystemExit):
        p.parse_args(["--mbr_metric", "nope"])
    with pytest.raises(ValueError):
        SampleSettings(mbr_metric="nope")
    # rejected before anything is loaded: the model path does not exist
    from run.sample import main
    with pytest.raises(ValueError):
        main({"mbr_metric": "nope", "model_path": str(tmp_path / "missing")})

    e = EvalSettings.from_argparse(EvalSettings.to_argparse().parse_args(["--path", "x.jsonl"]))
    assert e.rouge_l is False
    e = EvalSettings.from_argparse(EvalSettings.to_argparse().parse_args(["--path", "x.jsonl", "--rouge_l", "true"]))
    assert e.rouge_l is True and EvalSettings(**json.loads(e.json())) == e


def test_run_sample_picks_by_rouge_l(tmp_path):
    """``run.sample --mbr 3 --mbr_metric rouge_l`` on a freshly initialised tiny model (the CPU path):
    every written ``recover`` is the ROUGE-L pick among the written candidates."""
    from config.sample import SampleSettings
    from utils.initialization import create_model_from_config
    cfg = {"model": "diffuseq", "config_name": "tiny", "vocab_size": 1200, "seq_len": 16, "hidden_dim": 16,
           "hidden_t_dim": 16, "dropout": 0.0, "diffusion_steps": 8, "precision": "fp32", "dataset": "jsonl",
           "data_dir": str(tmp_path)}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    words = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu".split()
    with open(tmp_path / "test.jsonl", "w") as f:  # hashed word ids (no vocab.txt): 1000 .. 1199
        for i in range(6):
            f.write(json.dumps({"src": " ".join(words[i:i + 4]), "trg": " ".join(words[i + 3:i + 7])}) + "\n")
    torch.manual_seed(0)
    model = create_model_from_config(**SampleSettings(**cfg).dict())
    torch.save(model.state_dict(), tmp_path / "model_000000.pt")
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    env.pop("LOCAL_RANK", None)
    out = tmp_path / "out.jsonl"
    s = subprocess.run([sys.executable, "-m", "run.sample", "--config_json", str(tmp_path / "cfg.json"),
                        "--model_path", str(tmp_path), "--out_path", str(out), "--batch_size", "3",
                        "--num_batches", "2", "--step", "4", "--noise", "philox", "--mbr", "3",
                        "--mbr_metric", "rouge_l", "--keep_candidates", "true"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert s.returncode == 0, s.stdout[-3000:] + s.stderr[-3000:]
    rows = [json.loads(line) for line in open(out)]
    assert len(rows) == 6
    for row in rows:
        assert len(row["candidates"]) == 3
        assert row["recover"] == row["candidates"][mbr_select(row["candidates"], metric="rouge_l")]
    assert len({json.dumps(c) for row in rows for c in row["candidates"]}) > 1  # the candidates differ
