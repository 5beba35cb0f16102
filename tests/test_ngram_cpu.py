"""Clipped n-gram match counts on the CPU (the PyTorch path of ``ops.text.ngram_matches``), the
closed-form BLEU, batched MBR selection and ``python -m run.eval``.  Every comparison is exact; the
oracle is the ``Counter`` code of utils/mbr.py."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_pipeline_amd.ops.text import ngram_matches
from utils import mbr
from utils.mbr import bleu_from_counts, mbr_select, mbr_select_batch, pairwise_bleu, sentence_bleu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counter_matches(seqs):
    """[K][K][4] clipped match counts of the id lists ``seqs`` by the Counter formula."""
    out = []
    for a in seqs:
        row = []
        for b in seqs:
            row.append([sum(min(c, mbr._ngrams(b, n)[g]) for g, c in mbr._ngrams(a, n).items())
                        for n in range(1, 5)])
        out.append(row)
    return out


def random_groups(G, K, L, vocab, seed, poison="inside", dtype=torch.int64):
    """tokens [G, K, L], lens [G, K] with the lengths 0, 1, 2, 3 and L forced in, ids in
    [0, vocab) and the tails beyond each length poisoned: with ids that also occur inside it
    ("inside") or with -1."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, vocab, (G, K, L), generator=g, dtype=dtype)
    lens = torch.randint(0, L + 1, (G, K), generator=g)
    flat = lens.view(-1)
    for at, n in enumerate((0, 1, 2, 3, L)):
        flat[(at * 7) % flat.numel()] = min(n, L)
    if poison == "minus_one":
        beyond = torch.arange(L).view(1, 1, L) >= lens.unsqueeze(-1)
        tokens[beyond] = -1
    return tokens, lens


def oracle(tokens, lens):
    G, K, L = tokens.shape
    return torch.tensor([counter_matches([tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)])
                         for g in range(G)], dtype=torch.int32).reshape(G, K, K, 4)


@pytest.mark.parametrize("G,K,L,vocab", [(6, 3, 7, 2), (4, 5, 12, 3), (3, 2, 1, 2), (5, 4, 9, 5), (2, 1, 6, 2)])
def test_fallback_against_the_counter_oracle(G, K, L, vocab):
    tokens, lens = random_groups(G, K, L, vocab, seed=G * 100 + L)
    m = ngram_matches(tokens, lens)
    assert m.dtype == torch.int32 and m.shape == (G, K, K, 4)
    assert torch.equal(m, oracle(tokens, lens))
    # int32 ids, a non-contiguous view, lengths beyond [0, L], -1 beyond the lengths: the same counts
    assert torch.equal(ngram_matches(tokens.to(torch.int32), lens.to(torch.int32)), m)
    wide = torch.full((G, K, 2 * L), vocab - 1, dtype=tokens.dtype)
    wide[:, :, ::2] = tokens
    assert not wide[:, :, ::2].is_contiguous()
    assert torch.equal(ngram_matches(wide[:, :, ::2], lens), m)
    over = torch.where(lens == L, lens + 5, lens)
    over = torch.where(lens == 0, lens - 3, over)
    assert torch.equal(ngram_matches(tokens, over), m)
    t2, l2 = random_groups(G, K, L, vocab, seed=G * 100 + L, poison="minus_one")
    assert torch.equal(l2, lens) and torch.equal(ngram_matches(t2, l2), m)


def test_fallback_is_chunked_over_groups(monkeypatch):
    from distributed_pipeline_amd.ops import text
    tokens, lens = random_groups(9, 3, 8, 3, seed=5)
    whole = ngram_matches(tokens, lens)
    monkeypatch.setattr(text, "_FALLBACK_ELEMS", 2 * 3 * 3 * 8 * 8)  # two groups per chunk, a last one alone
    assert torch.equal(ngram_matches(tokens, lens), whole)
    assert ngram_matches(tokens[:0], lens[:0]).shape == (0, 3, 3, 4)


def test_symmetry_and_diagonal():
    tokens, lens = random_groups(8, 6, 11, 3, seed=3)
    m = ngram_matches(tokens, lens)
    assert torch.equal(m, m.transpose(1, 2))
    n = torch.arange(1, 5).view(1, 1, 4)
    diag = (lens.unsqueeze(-1) - n + 1).clamp_min(0).to(torch.int32)
    assert torch.equal(torch.diagonal(m, dim1=1, dim2=2).permute(0, 2, 1), diag)


def test_bleu_from_counts_is_what_sentence_bleu_ends_with():
    # the pinned values of tests/test_sampler_cpu.py
    assert bleu_from_counts(3, 2, 1, 0, 4, 4) == sentence_bleu([1, 2, 3, 4], [1, 2, 3, 5])
    assert bleu_from_counts(3, 2, 1, 0, 4, 4) == pytest.approx(0.1875 ** 0.25, abs=1e-12)
    assert bleu_from_counts(4, 3, 2, 1, 4, 4) == sentence_bleu([1, 2, 3, 4], [1, 2, 3, 4])
    assert bleu_from_counts(4, 3, 2, 1, 4, 4) == pytest.approx(1.0, abs=1e-12)
    assert bleu_from_counts(0, 0, 0, 0, 0, 2) == 0.0 == sentence_bleu([], [1, 2])
    assert bleu_from_counts(0, 0, 0, 0, 2, 2) == 0.0 == sentence_bleu([7, 8], [1, 2])
    assert bleu_from_counts(2, 1, 0, 0, 2, 4) == sentence_bleu([1, 2], [1, 2, 3, 4])
    # and on random pairs, from the counts of ngram_matches
    tokens, lens = random_groups(10, 2, 9, 3, seed=11)
    m = ngram_matches(tokens, lens).tolist()
    for g in range(10):
        a, b = (tokens[g, k, :int(lens[g, k])].tolist() for k in range(2))
        assert bleu_from_counts(*m[g][0][1], len(a), len(b)) == sentence_bleu(a, b)
        assert bleu_from_counts(*m[g][1][0], len(b), len(a)) == sentence_bleu(b, a)


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
def test_mbr_select_batch_equals_mbr_select(G, K, L, vocab):
    tokens, lens = groups_with_duplicates(G, K, L, vocab, seed=K * 10 + L)
    lists = [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(G)]
    assert mbr_select_batch(tokens, lens) == [mbr_select(c) for c in lists]
    pb = pairwise_bleu(tokens, lens)
    assert pb.dtype == torch.float64 and pb.shape == (G, K, K)
    assert pb.tolist() == [[[sentence_bleu(a, b) for b in c] for a in c] for c in lists]


def test_mbr_select_batch_ties_and_empties():
    A, B = [5, 6, 7, 8, 9], [5, 6, 1, 2, 3]
    groups = [[A, A, B], [B, A, A], [A, A, A], [[], [], []]]
    tokens = torch.tensor([[s + [9] * (5 - len(s)) for s in grp] for grp in groups])
    lens = torch.tensor([[len(s) for s in grp] for grp in groups])
    assert mbr_select_batch(tokens, lens) == [0, 1, 0, 0] == [mbr_select(grp) for grp in groups]


def test_recover_parts_is_split_sample():
    from run.sample import recover_parts, split_sample
    g = torch.Generator().manual_seed(4)
    B, K, L = 7, 3, 12
    recs = [torch.randint(0, 4, (B, L), generator=g) for _ in range(K)]  # 0: the pad id, often
    recs[1][2, :] = 3                                                     # no pad at all
    n_src = torch.tensor([0, 1, 5, 11, 12, 3, 7])
    mask = (torch.arange(L).view(1, L) >= n_src.view(B, 1)).long()
    tokens, lens = recover_parts(recs, mask, 0)
    assert tokens.shape == (B, K, L) and lens.shape == (B, K)
    for b in range(B):
        for k in range(K):
            want = split_sample(recs[k][b], mask[b], recs[k][b], 0)[2]
            assert tokens[b, k, :int(lens[b, k])].tolist() == want


def test_run_eval_on_a_hand_written_file(tmp_path):
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
    r = subprocess.run([sys.executable, "-m", "run.eval", "--path", str(path)], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"n", "bleu", "len", "dist1", "self_bleu"}
    assert out["n"] == 3
    b0 = sentence_bleu([1, 2, 3, 4], [1, 2, 3, 5])
    assert b0 == pytest.approx(0.1875 ** 0.25, abs=1e-12)
    assert out["bleu"] == (b0 + sentence_bleu([1, 2, 3, 4], [1, 2, 3, 4]) + 0.0) / 3
    assert out["len"] == 8 / 3
    assert out["dist1"] == (1.0 + 1.0 + 0.0) / 3
    selfs = []
    for row in rows:
        c = row["candidates"]
        selfs.append(sum(sentence_bleu(c[i], c[j]) for i in range(3) for j in range(3) if i != j) / 6)
    assert selfs[2] > 0.0  # [7, 7] against [7, 8]: one unigram
    assert out["self_bleu"] == sum(selfs) / 3
    # rows without candidates: no self_bleu
    plain = tmp_path / "plain.jsonl"
    plain.write_text("".join(json.dumps({k: v for k, v in r_.items() if k != "candidates"}) + "\n" for r_ in rows))
    from run.eval import create_parser, main
    out2 = main(create_parser().parse_args(["--path", str(plain)]))
    assert "self_bleu" not in out2 and out2["bleu"] == out["bleu"] and out2["dist1"] == out["dist1"]
