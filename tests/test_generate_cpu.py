"""GPT-2 generation on the CPU (fp32 PyTorch path): the cached ``prefill`` / ``decode_step`` against
the full forward, greedy ``generate`` against the uncached loop, ``utils.lm_sampling``, the
PyTorch ``attention_decode`` against float64, and ``python -m run.generate``."""
import json
import os
import subprocess
import sys

import pytest
import torch

from decode_helpers import RAGGED_LENS, bits, guarded_caches, ref64, teacher_forced
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops.decode import attention_decode, attention_decode_ref
from utils import lm_sampling as lms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2,
                       vocab_size=300, seq_len=64, dropout=0.0, precision="fp32").eval()


def test_cached_logits_match_the_full_forward(model):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 300, (4, 40), generator=g)
    plens = [1, 5, 17, 24]
    with torch.no_grad():
        full = model(ids)
    got, _ = teacher_forced(model, ids, plens, 24)
    assert len(got) == sum(40 - p + 1 for p in plens)
    err = max((got[(b, p)] - full[b, p]).abs().max().item() for (b, p) in got)
    assert err <= 1e-4, err


def _uncached_greedy(model, prompt, n):
    seq = prompt.clone()
    for _ in range(n):
        with torch.no_grad():
            seq = torch.cat([seq, lms.greedy(model(seq[None])[0, -1:])])
    return seq[len(prompt):]


def test_greedy_generate_equals_the_uncached_loop(model):
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 300, (3, 10), generator=g)
    plens = [3, 7, 10]
    toks, new_lens = model.generate(ids, torch.tensor(plens), 8, temperature=0)
    assert toks.shape == (3, 8) and new_lens.tolist() == [8, 8, 8]
    for b, p in enumerate(plens):
        assert toks[b].tolist() == _uncached_greedy(model, ids[b, :p], 8).tolist()


def test_generate_parks_rows_at_eos_and_at_a_full_cache(model):
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 300, (3, 6), generator=g)
    lens = torch.tensor([6, 4, 6])
    free, _ = model.generate(ids, lens, 6, temperature=0)
    eos = int(free[0, 2])
    first = free[0].tolist().index(eos)
    cache = model.init_cache(3, 12)
    toks, new_lens = model.generate(ids, lens, 6, temperature=0, eos_id=eos, cache=cache, check_every=2)
    assert toks[0].tolist() == free[0, :first + 1].tolist() + [eos] * (5 - first)
    assert new_lens[0] == first + 1 and cache.lens[0] == -1
    for b in (1, 2):
        if eos not in free[b].tolist():
            assert toks[b].tolist() == free[b].tolist() and new_lens[b] == 6
    # a cache of 8 rows: a prompt of 6 has room to run 2 tokens, so a third can still be chosen
    small = model.init_cache(3, 8)
    toks, new_lens = model.generate(ids, lens, 6, temperature=0, cache=small)
    assert new_lens.tolist() == [3, 5, 3]
    assert toks[0].tolist() == free[0, :3].tolist() + [0, 0, 0]
    assert toks[1].tolist() == free[1, :5].tolist() + [0]
    assert small.lens.tolist() == [-1, -1, -1]


# ---- utils.lm_sampling ---------------------------------------------------------------------

def _kept(x):
    return (x > float("-inf")).nonzero().flatten().tolist()


def test_top_k_keeps_ties_with_the_kth():
    x = torch.tensor([[1.0, 3.0, 2.0, 2.0, 0.5, 2.0]])
    assert _kept(lms.filter_top_k(x, 2)[0]) == [1, 2, 3, 5]
    assert _kept(lms.filter_top_k(x, 1)[0]) == [1]
    assert torch.equal(lms.filter_top_k(x, 0), x) and torch.equal(lms.filter_top_k(x, 6), x)
    kept = lms.filter_top_k(x, 2)
    assert torch.equal(kept[kept > float("-inf")], x[0, [1, 2, 3, 5]])


def test_top_p_keeps_the_smallest_prefix_that_reaches_p():
    probs = torch.tensor([[0.1, 0.4, 0.2, 0.3]])
    x = probs.log()
    assert _kept(lms.filter_top_p(x, 0.35)[0]) == [1]            # 0.4 reaches 0.35
    assert _kept(lms.filter_top_p(x, 0.5)[0]) == [1, 3]          # 0.4 < 0.5 <= 0.7
    assert _kept(lms.filter_top_p(x, 0.75)[0]) == [1, 2, 3]      # 0.7 < 0.75 <= 0.9
    assert _kept(lms.filter_top_p(x, 1.0)[0]) == [0, 1, 2, 3]
    assert _kept(lms.filter_top_p(x, 1e-9)[0]) == [1]            # never fewer than one
    assert torch.equal(lms.filter_top_p(x, 0.0), x)
    assert torch.equal(lms.filter_logits(x, 0, 0.0), x)
    # top_k first, top_p on what it kept: of {0.4, 0.3} renormalised, 0.4 / 0.7 reaches 0.5
    assert _kept(lms.filter_logits(x, 2, 0.5)[0]) == [1]


def test_greedy_ties_go_to_the_lowest_id():
    x = torch.tensor([[0.0, 2.0, 2.0, 1.0], [5.0, 1.0, 5.0, 5.0], [float("nan"), 1.0, 0.0, 1.0]])
    assert lms.greedy(x).tolist() == [1, 0, 1]
    assert lms.sample_next(x, temperature=0, generator=torch.Generator().manual_seed(0)).tolist() == [1, 0, 1]


def test_seeded_draws_reproduce_and_respect_the_filters():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2000, 50, generator=g)

    def draw(seed, **kw):
        return lms.sample_next(x, generator=torch.Generator().manual_seed(seed), **kw)

    a, b = draw(7, temperature=0.8, top_k=5), draw(7, temperature=0.8, top_k=5)
    assert torch.equal(a, b) and not torch.equal(a, draw(8, temperature=0.8, top_k=5))
    allowed = lms.filter_top_k(x / 0.8, 5) > float("-inf")
    assert allowed.sum(-1).eq(5).all() and allowed.gather(1, a[:, None]).all()
    c = draw(9, temperature=1.3, top_p=0.6)
    allowed = lms.filter_top_p(x / 1.3, 0.6) > float("-inf")
    assert allowed.gather(1, c[:, None]).all() and not allowed.all()
    with pytest.raises(ValueError):
        lms.sample_next(x, temperature=-1.0)
    with pytest.raises(ValueError):
        lms.sample_next(x, top_p=1.5)


# ---- ops.decode.attention_decode (PyTorch path) ---------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_torch_attention_decode_matches_float64(dtype):
    H, D, Lmax = 2, 16, 1024
    g = torch.Generator().manual_seed(5)
    for lens in (RAGGED_LENS[:12], RAGGED_LENS[12:], [-1, 3, Lmax, 0, Lmax + 5, Lmax - 1]):
        B = len(lens)
        buf, k, v = guarded_caches(B, H, Lmax, D, "cpu", dtype)
        k.copy_(torch.randn(B, H, Lmax, D, generator=g))
        v.copy_(torch.randn(B, H, Lmax, D, generator=g))
        qkv = torch.randn(B, 3 * H * D, generator=g).to(dtype)
        lens_t = torch.tensor(lens, dtype=torch.int32)
        want = ref64(qkv, k, v, lens_t, H)
        before = buf.clone()
        out = attention_decode(qkv, k, v, lens_t, H)
        assert out.dtype == dtype and out.shape == (B, H * D)
        # one rounding of the output to its dtype (an ulp allowed) + the fp32 sums over <= 1024 keys
        ulp = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -8
        assert ((out.double() - want).abs() <= ulp * want.abs() + 2e-5).all()
        new = qkv.view(B, 3, H, D)
        for b, n in enumerate(lens):
            if 0 <= n < Lmax:
                assert torch.equal(k[b, :, n], new[b, 1]) and torch.equal(v[b, :, n], new[b, 2])
                before[0, b, :, 3 + n], before[1, b, :, 3 + n] = new[b, 1], new[b, 2]
            else:
                assert not out[b].any()
        assert torch.equal(bits(buf), bits(before))  # nothing else was written
        assert torch.equal(lens_t, torch.tensor(lens, dtype=torch.int32))


def test_torch_attention_decode_ignores_what_lies_beyond_lens():
    H, D, Lmax = 2, 16, 64
    g = torch.Generator().manual_seed(6)
    k, v = torch.randn(3, H, Lmax, D, generator=g), torch.randn(3, H, Lmax, D, generator=g)
    qkv = torch.randn(3, 3 * H * D, generator=g)
    lens = torch.tensor([0, 9, 62], dtype=torch.int32)
    outs = []
    for fill in (0.0, float("nan")):
        kk, vv = k.clone(), v.clone()
        for b, n in enumerate(lens.tolist()):
            kk[b, :, n + 1:] = fill
            vv[b, :, n + 1:] = fill
        outs.append(attention_decode_ref(qkv, kk, vv, lens, H))
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[0], outs[1])


# ---- python -m run.generate ------------------------------------------------------------------

def test_run_generate_entry_point(tmp_path):
    """A 2-step tiny GPT-2 training run on the CPU, then ``python -m run.generate`` on its
    checkpoint directory."""
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
    assert (ck / "model_000002.pt").exists()

    def generate(out, *extra, ok=True, cfg=ck / "training_args.json"):
        s = subprocess.run([sys.executable, "-m", "run.generate", "--config_json", str(cfg),
                            "--model_path", str(ck), "--out_path", str(out), "--batch_size", "3",
                            "--num_batches", "2", "--prompt_len", "8", "--max_new_tokens", "6", *extra],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert (s.returncode == 0) == ok, s.stdout[-3000:] + s.stderr[-3000:]
        return ([json.loads(line) for line in open(out)] if ok else None), s.stdout + s.stderr

    rows, log = generate(tmp_path / "a.jsonl", "--top_k", "20")
    assert "model_000002.pt" in log and len(rows) == 3 * 2
    for row in rows:
        assert set(row) == {"prompt", "continuation", "reference"}
        assert len(row["prompt"]) == 8 and len(row["reference"]) == 6 and len(row["continuation"]) <= 6
        assert all(isinstance(i, int) and 0 <= i < 200 for key in row for i in row[key])
    assert generate(tmp_path / "b.jsonl", "--top_k", "20")[0] == rows                  # same seed, same file
    assert generate(tmp_path / "c.jsonl", "--top_k", "20", "--seed", "7")[0] != rows
    greedy = generate(tmp_path / "d.jsonl", "--temperature", "0", "--seed", "1")[0]
    greedy2 = generate(tmp_path / "e.jsonl", "--temperature", "0", "--seed", "2")[0]
    assert greedy == greedy2 and [r_["prompt"] for r_ in greedy] == [r_["prompt"] for r_ in rows]
    eos = greedy[0]["continuation"][2]
    cut = generate(tmp_path / "f.jsonl", "--temperature", "0", "--seed", "1", "--eos_id", str(eos))[0]
    assert cut[0]["continuation"] == greedy[0]["continuation"][:greedy[0]["continuation"].index(eos)]

    # rejected before any checkpoint is read: nothing is loaded, so no "### loading" line
    _, log = generate(tmp_path / "g.jsonl", "--max_new_tokens", "25", ok=False)
    assert "exceeds seq_len" in log and "### loading" not in log
    _, log = generate(tmp_path / "h.jsonl", "--top_p", "1.5", ok=False)
    assert "top_p" in log and "### loading" not in log
    _, log = generate(tmp_path / "i.jsonl", "--temperature", "-1", ok=False)
    assert "temperature" in log and "### loading" not in log
    bad = tmp_path / "diffuseq.json"
    cfg = json.load(open(ck / "training_args.json"))
    cfg["model"] = "diffuseq"
    bad.write_text(json.dumps(cfg))
    _, log = generate(tmp_path / "j.jsonl", ok=False, cfg=bad)
    assert "gpt2" in log and "### loading" not in log
