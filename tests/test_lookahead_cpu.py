"""Lookahead decoding on the CPU (fp32 PyTorch path): ``attention_decode_block`` against float64 and
against the sequential calls, ``lookup_draft`` against a list implementation, ``generate_lookahead``
against ``generate(temperature=0)``, and ``python -m run.generate --lookahead``."""
import json
import os
import subprocess
import sys

import pytest
import torch

from decode_block_helpers import block_counts, list_lookup, lookahead_loop, oracle_draft, ref64_block
from decode_helpers import bits, guarded_caches
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops.decode import (attention_decode_block, attention_decode_block_ref,
                                                 attention_decode_ref, lookup_draft)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 40
PLENS = [3, 7, 12, 1]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2,
                       vocab_size=300, seq_len=64, dropout=0.0, precision="fp32").eval()


@pytest.fixture(scope="module")
def prompts():
    return torch.randint(0, 300, (4, 12), generator=torch.Generator().manual_seed(2))


@pytest.fixture(scope="module")
def greedy_ref(model, prompts):
    """``generate(temperature=0)`` once, with the precondition of every equality below: along the
    greedy paths every top-2 margin of the fp32 full forward exceeds 1e-3 (the cached path is within
    1e-4 of the full forward), so no arg-max hangs on the rounding of either path."""
    toks, new_lens = model.generate(prompts, torch.tensor(PLENS), N, temperature=0)
    margin = float("inf")
    with torch.no_grad():
        for b, p in enumerate(PLENS):
            seq = torch.cat([prompts[b, :p], toks[b]])
            top = model(seq[None])[0, p - 1:p + N - 1].topk(2, -1).values
            margin = min(margin, (top[:, 0] - top[:, 1]).min().item())
    print(f"smallest top-2 margin along the greedy paths: {margin:.3e}")
    assert margin > 1e-3, margin
    return toks, new_lens


# ---- ops.decode.attention_decode_block (PyTorch path) ---------------------------------------

@pytest.mark.parametrize("T", [1, 2, 5, 8])
def test_torch_block_matches_float64_and_the_sequential_calls(T):
    H, D, Lmax = 2, 16, 64
    g = torch.Generator().manual_seed(11)
    lens = [0, 7, 31, 60, 63, -1, Lmax, 20]
    counts = [T, 1, T, T, T, T, T, 0] if T > 1 else None
    B = len(lens)
    buf, k, v = guarded_caches(B, H, Lmax, D, "cpu", torch.float32)
    k.copy_(torch.randn(B, H, Lmax, D, generator=g))
    v.copy_(torch.randn(B, H, Lmax, D, generator=g))
    qkv = torch.randn(B, T, 3 * H * D, generator=g)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    counts_t = None if counts is None else torch.tensor(counts, dtype=torch.int32)
    want = ref64_block(qkv, k, v, lens, H, counts)
    # the sequential calls, on a copy
    buf2 = buf.clone()
    k2, v2 = buf2[0, :, :, 3:3 + Lmax], buf2[1, :, :, 3:3 + Lmax]
    c = block_counts(lens, counts, T, Lmax)
    seq = torch.stack([attention_decode_ref(qkv[:, j], k2, v2, torch.tensor(
        [n + j if j < c[b] else -1 for b, n in enumerate(lens)], dtype=torch.int32), H) for j in range(T)], 1)
    before = buf.clone()
    out = attention_decode_block(qkv, k, v, lens_t, H, counts=counts_t)
    assert out.shape == (B, T, H * D) and out.dtype == torch.float32
    assert torch.equal(out, seq) and torch.equal(buf, buf2)
    assert ((out.double() - want).abs() <= 2.0 ** -23 * want.abs() + 2e-5).all()
    new = qkv.view(B, T, 3, H, D)
    for b, n in enumerate(lens):
        for j in range(T):
            if j < c[b]:
                before[0, b, :, 3 + n + j], before[1, b, :, 3 + n + j] = new[b, j, 1], new[b, j, 2]
            else:
                assert not out[b, j].any()
    assert c[3] == min(T, 4) and c[4] == 1 and c[5] == c[6] == 0 and c[7] == (1 if counts is None else 0)
    assert torch.equal(bits(buf), bits(before))  # nothing else was written
    assert lens_t.tolist() == lens and (counts is None or counts_t.tolist() == counts)


def test_block_rejects_bad_shapes():
    H, D, Lmax = 2, 16, 8
    k, v = torch.zeros(2, H, Lmax, D), torch.zeros(2, H, Lmax, D)
    lens = torch.zeros(2, dtype=torch.int32)
    for T in (0, 9):
        with pytest.raises(ValueError):
            attention_decode_block(torch.zeros(2, T, 3 * H * D), k, v, lens, H)
    with pytest.raises(ValueError):
        attention_decode_block(torch.zeros(2, 2, 3 * H * D), k, v, lens, H, counts=torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        attention_decode_block_ref(torch.zeros(2, 2, 3 * H * D), k, v, lens, H, counts=torch.zeros(3, dtype=torch.int32))


# ---- ops.decode.lookup_draft ----------------------------------------------------------------

def _both(rows, n, g, M):
    width = max(len(r) for r in rows)
    h = torch.tensor([list(r) + [0] * (width - len(r)) for r in rows], dtype=torch.long)
    draft, k = lookup_draft(h, torch.tensor(n), ngram=g, max_draft=M)
    want = [list_lookup(h[b].tolist(), n[b], g, M) for b in range(len(rows))]
    assert draft.dtype == torch.long and k.dtype == torch.long and draft.shape == (len(rows), M)
    assert draft.tolist() == [w[0] for w in want] and k.tolist() == [w[1] for w in want]
    return draft.tolist(), k.tolist()


def test_lookup_draft_hand_cases():
    # no match
    assert _both([[1, 2, 3, 4, 5, 6]], [6], 2, 3) == ([[0, 0, 0]], [0])
    # p = 1: the row repeats its last token
    assert _both([[9, 4, 4, 0, 0]], [3], 1, 4) == ([[4, 4, 4, 4]], [4])
    # p = 3 with max_draft = 7: the copy runs into its own output
    assert _both([[1, 2, 3, 1, 2, 3, 1, 2]], [8], 2, 7) == ([[3, 1, 2, 3, 1, 2, 3]], [7])
    # the latest earlier occurrence wins: "1 2" at 0 (-> 7) and at 3 (-> 8)
    assert _both([[1, 2, 7, 1, 2, 8, 1, 2]], [8], 2, 2) == ([[8, 1]], [2])
    # n < g + 1; n = 0; n beyond Lh is clamped to Lh; what lies behind n is not history
    assert _both([[5, 5, 5, 5]], [2], 2, 3) == ([[0, 0, 0]], [0])
    assert _both([[5, 5, 5, 5]], [0], 1, 3) == ([[0, 0, 0]], [0])
    assert _both([[1, 2, 1, 2]], [9], 2, 3) == ([[1, 2, 1]], [3])
    assert _both([[1, 2, 3, 1, 2]], [3], 2, 2) == ([[0, 0]], [0])
    # a history shorter than g + 1, and max_draft = 0
    assert _both([[3, 3]], [2], 2, 3) == ([[0, 0, 0]], [0])
    assert _both([[3, 3, 3]], [3], 1, 0) == ([[]], [0])
    with pytest.raises(ValueError):
        lookup_draft(torch.zeros(1, 4, dtype=torch.long), torch.tensor([4]), ngram=0, max_draft=2)


def test_lookup_draft_random_histories():
    g = torch.Generator().manual_seed(12)
    h = torch.randint(0, 4, (64, 37), generator=g)
    n = torch.randint(0, 41, (64,), generator=g).tolist()
    for ngram in (1, 2, 3):
        for M in (1, 3, 7):
            _, k = _both(h.tolist(), n, ngram, M)
            assert max(k) == M and (ngram < 3 or min(k) == 0)  # both outcomes occur


# ---- generate_lookahead ----------------------------------------------------------------------

@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("T", [2, 4, 8])
def test_lookahead_equals_greedy_generate(model, prompts, greedy_ref, T, g):
    want, want_lens = greedy_ref
    cache = model.init_cache(4, 12 + N)
    toks, new_lens, stats = model.generate_lookahead(prompts, torch.tensor(PLENS), N, lookahead=T, ngram=g,
                                                     cache=cache, return_stats=True)
    assert torch.equal(toks, want) and torch.equal(new_lens, want_lens)
    assert cache.lens.tolist() == [p + N - 1 for p in PLENS]  # the last token has not been run
    assert 0 <= stats["accepted"] <= stats["proposed"] and 1 <= stats["model_calls"] <= N - 1
    print(f"T={T} ngram={g}: {stats}")
    # the written-out loop: the same numbers, step for step
    t2, l2, s2, c2 = lookahead_loop(model, prompts, torch.tensor(PLENS), N, T, g)
    assert torch.equal(t2, toks) and l2 == new_lens.tolist() and s2 == stats
    assert c2.lens.tolist() == cache.lens.tolist()


def test_lookahead_with_eos_mid_block_and_a_cache_that_fills(model, prompts, greedy_ref):
    free, _ = greedy_ref
    lens = torch.tensor(PLENS)
    # the oracle accepts whole blocks, so with T = 8 output position 5 lies inside the first block
    eos = int(free[0, 5])
    for T, draft in ((8, oracle_draft(free, PLENS, 300)), (4, None)):
        c1, c2 = model.init_cache(4, 12 + N), model.init_cache(4, 12 + N)
        want, want_lens = model.generate(prompts, lens, N, temperature=0, eos_id=eos, cache=c1)
        toks, new_lens = model.generate_lookahead(prompts, lens, N, lookahead=T, eos_id=eos, cache=c2, draft=draft)
        first = free[0].tolist().index(eos)
        assert want_lens[0] == first + 1 and toks[0, first + 1:].eq(eos).all() and c2.lens[0] == -1
        assert torch.equal(toks, want) and torch.equal(new_lens, want_lens)
        assert c2.lens.tolist() == c1.lens.tolist()
    # a 20-row cache: a prompt of p tokens can run 20 - p more, so 21 - p tokens are chosen
    for T in (2, 4, 8):
        c1, c2 = model.init_cache(4, 20), model.init_cache(4, 20)
        want, want_lens = model.generate(prompts, lens, N, temperature=0, cache=c1)
        toks, new_lens = model.generate_lookahead(prompts, lens, N, lookahead=T, cache=c2, check_every=0)
        assert want_lens.tolist() == [18, 14, 9, 20]
        assert torch.equal(toks, want) and torch.equal(new_lens, want_lens)
        assert c2.lens.tolist() == c1.lens.tolist() == [-1] * 4


@pytest.mark.parametrize("T", [2, 4, 8])
def test_oracle_drafts_take_the_exact_number_of_calls(model, prompts, greedy_ref, T):
    want, want_lens = greedy_ref
    toks, new_lens, stats = model.generate_lookahead(prompts, torch.tensor(PLENS), N, lookahead=T,
                                                     draft=oracle_draft(want, PLENS, 300), return_stats=True)
    assert torch.equal(toks, want) and torch.equal(new_lens, want_lens)
    assert stats["model_calls"] == -(-(N - 1) // T)
    assert stats["accepted"] == stats["proposed"]


@pytest.mark.parametrize("T", [4, 8])
def test_corrupted_oracle_drafts_are_rejected_where_they_are_wrong(model, prompts, greedy_ref, T):
    want, want_lens = greedy_ref
    corrupt = torch.zeros(4, N, dtype=torch.bool)
    for b, at in enumerate(([3, 17], [1, 2, 30], [39], [10, 11, 12, 13])):
        corrupt[b, at] = True
    draft = oracle_draft(want, PLENS, 300, corrupt)
    toks, new_lens, stats = model.generate_lookahead(prompts, torch.tensor(PLENS), N, lookahead=T, draft=draft,
                                                     return_stats=True)
    assert torch.equal(toks, want) and torch.equal(new_lens, want_lens)
    t2, l2, s2, _ = lookahead_loop(model, prompts, torch.tensor(PLENS), N, T, draft=draft)
    assert torch.equal(t2, toks) and l2 == new_lens.tolist() and s2 == stats
    # every row meets each of its wrong guesses at most once, and a wrong guess is never accepted:
    # per row, the guesses accepted are the right ones in front of the first wrong one of each block
    acc = 0
    for b in range(4):
        pos = 1
        while pos < N:
            c = min(T, N - pos)  # the block: output position pos - 1 and guesses for pos .. pos + c - 2
            a = 0
            while a + 1 < c and not corrupt[b, pos + a]:
                a += 1
            acc += a
            pos += a + 1
    assert stats["accepted"] == acc and stats["accepted"] < stats["proposed"]


def test_lookahead_rejects_bad_arguments_before_any_work(model, prompts):
    for kw in (dict(lookahead=1), dict(lookahead=9), dict(lookahead=4, ngram=0)):
        with pytest.raises(ValueError):
            model.generate_lookahead(prompts, torch.tensor(PLENS), 4, cache=object(), **kw)


# ---- python -m run.generate --lookahead --------------------------------------------------------

def test_run_generate_lookahead(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1", WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck = tmp_path / "ck"
    common = ["--model", "gpt2", "--config_name", "tiny", "--vocab_size", "200", "--seq_len", "32",
              "--dropout", "0.0", "--precision", "fp32", "--dataset", "synthetic", "--data_loader_workers", "0"]
    r = subprocess.run([sys.executable, "-m", "run.train", *common, "--batch_size", "4", "--microbatch", "4",
                        "--learning_steps", "2", "--save_interval", "2", "--log_interval", "1",
                        "--eval_interval", "100", "--ema_rate", "0.9", "--checkpoint_path", str(ck)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def generate(out, *extra, ok=True):
        s = subprocess.run([sys.executable, "-m", "run.generate", "--config_json", str(ck / "training_args.json"),
                            "--model_path", str(ck), "--out_path", str(out), "--batch_size", "3",
                            "--num_batches", "2", "--prompt_len", "8", "--max_new_tokens", "16", *extra],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert (s.returncode == 0) == ok, s.stdout[-3000:] + s.stderr[-3000:]
        return (open(out, "rb").read() if ok else None), s.stdout + s.stderr

    plain, log = generate(tmp_path / "a.jsonl", "--temperature", "0")
    assert "### lookahead" not in log
    off, log = generate(tmp_path / "b.jsonl", "--temperature", "0", "--lookahead", "0")
    assert off == plain and "### lookahead" not in log
    look, log = generate(tmp_path / "c.jsonl", "--temperature", "0", "--lookahead", "4")
    assert look == plain and len([json.loads(x) for x in look.splitlines()]) == 6
    line = [x for x in log.splitlines() if x.startswith("### lookahead 4:")]
    assert len(line) == 1 and "model calls" in line[0] and "guesses accepted" in line[0], log
    look3, _ = generate(tmp_path / "d.jsonl", "--temperature", "0", "--lookahead", "8", "--lookup_ngram", "1")
    assert look3 == plain
    # rejected before any checkpoint is read
    for extra, word in ((("--lookahead", "1", "--temperature", "0"), "--lookahead must"),
                        (("--lookahead", "9", "--temperature", "0"), "--lookahead must"),
                        (("--lookahead", "-2", "--temperature", "0"), "--lookahead must"),
                        (("--lookahead", "4", "--temperature", "0", "--lookup_ngram", "0"), "--lookup_ngram must"),
                        (("--lookahead", "4"), "needs --temperature 0"),
                        (("--lookahead", "4", "--temperature", "0.7"), "needs --temperature 0"),
                        (("--lookahead", "4", "--temperature", "0", "--num_beams", "2"), "excludes --num_beams")):
        _, log = generate(tmp_path / "x.jsonl", *extra, ok=False)
        assert word in log and "### loading" not in log, (extra, log[-500:])
