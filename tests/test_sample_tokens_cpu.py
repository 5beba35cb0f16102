"""``ops.decode.sample_tokens`` on the CPU (its PyTorch path): the Philox replica against plain
Python integers, top-k, top-p, the draw, batch independence, the distribution, degenerate rows,
``GPT2LMModel.generate(noise_seed=...)`` in fp32 and ``python -m run.generate --noise philox``.
The checks and the float64 yardstick are in ``sample_helpers.py``; the kernel runs the same ones
in ``test_sample_tokens_gpu.py``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_helpers as sh
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops import decode
from distributed_pipeline_amd.ops.decode import sample_tokens, sample_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


def _philox4_int(k0, k1, c):
    """csrc/common.h philox4 on Python ints."""
    c0, c1, c2, c3 = c
    for _ in range(7):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def test_uniform_replica_matches_integer_philox():
    assert decode.SM_DOMAIN == 0x536D706C  # a domain of its own: reverse_step.hip's is 0x52657653
    for seed, step, row_base, V in ((7, 0, 0, 8), (2 ** 40 + 7, 3, 5, 257), (2 ** 64 + 2 ** 63 + 9, 2 ** 32 - 1, 2 ** 33, 1000)):
        B, V4 = 3, (V + 3) // 4
        u = sample_uniforms(seed, step, row_base, B, V)
        assert u.shape == (B, V) and u.dtype == torch.float32
        n = (u.double() * 2 ** 24)
        assert (n == n.round()).all() and (n.long() % 2 == 1).all() and (u > 0).all() and (u < 1).all()
        for b, v in ((0, 0), (1, 5), (2, V - 1), (2, V // 2)):
            grp = ((row_base + b) * V4 + v // 4) & (2 ** 64 - 1)
            r = _philox4_int(seed & M32, step & M32, (grp & M32, grp >> 32, (seed >> 32) & M32, decode.SM_DOMAIN))
            assert u[b, v].item() == (2 * (r[v & 3] >> 9) + 1) / 2 ** 24, (seed, b, v)
    base = sample_uniforms(7, 3, 5, 2, 257)
    for other in ((7, 4, 5), (7 + 2 ** 32, 3, 5), (7, 3, 6), (8, 3, 5)):
        assert not torch.equal(base, sample_uniforms(*other, 2, 257))
    # row_base shifts rows: row 1 of base 5 is row 0 of base 6
    assert torch.equal(base[1], sample_uniforms(7, 3, 6, 1, 257)[0])


@pytest.mark.parametrize("V,B", sh.SHAPES)
def test_top_k_is_exact(V, B):
    sh.check_top_k_exact(V, B, "cpu")


def test_top_k_keeps_ties_with_the_kth():
    sh.check_top_k_ties("cpu")


@pytest.mark.parametrize("V,B", sh.SHAPES)
def test_top_p_sandwich(V, B):
    """tau64(p + d) <= thr <= tau64(p - d) with d = 1e-4, derived: the masses are fp32 sums of at most
    65536 non-negative terms, each exp good to a few ulp; any tree or per-thread-then-tree order is
    within about 1e-6 relative of the true sum, and only a fully sequential fp32 order could reach
    65536 * 2^-24 = 4e-3 (this path's cumulative sum accumulates in double on the CPU)."""
    sh.check_top_p_sandwich(V, B, "cpu")


def test_top_p_pinned_cases():
    sh.check_top_p_pinned("cpu")


@pytest.mark.parametrize("V,B", sh.SHAPES)
def test_draw_is_the_perturbed_argmax(V, B):
    """eps = 1e-4, derived: scores stay below 128, where an fp32 ulp is 7.6e-6; the division, the sum
    and g each round within one ulp at that size, so one score is within about 1.2e-5 of its float64
    value and the margin across two scores is four times that."""
    worst = sh.check_draw(V, B, "cpu")
    print(f"V={V} B={B}: largest float64 score gap of a drawn token = {worst:.3e} (eps {sh.EPS})")


def test_batch_independence_and_reproducibility():
    sh.check_batch_independence("cpu")


def test_distribution_chi_squared():
    """seed 20240: the statistic is 1.083 on 3 degrees of freedom (4 kept ids), against the 1 - 1e-4
    quantile 21.108."""
    stat, bound, n = sh.check_distribution("cpu")
    print(f"chi2 = {stat:.3f} on {n - 1} degrees of freedom, bound {bound}")
    assert n == 4 and stat < bound, (stat, bound)


def test_degenerate_rows():
    sh.check_degenerate("cpu")


def test_temperature_zero_is_greedy_and_bad_arguments_raise():
    from utils.lm_sampling import greedy
    x = torch.randn(5, 300, generator=torch.Generator().manual_seed(8))
    x[2, 7] = x[2].max()  # a tie: the lowest id
    assert torch.equal(sample_tokens(x, temperature=0, seed=1, step=0), greedy(x))
    tok, thr, kept = sample_tokens(x, temperature=0, seed=1, step=0, return_stats=True)
    assert torch.equal(tok, greedy(x)) and torch.equal(thr, x.amax(-1)) and kept.tolist() == [0] * 5
    with pytest.raises(ValueError):
        sample_tokens(x, temperature=-1.0, seed=1, step=0)
    with pytest.raises(ValueError):
        sample_tokens(x[0], temperature=1.0, seed=1, step=0)
    # other dtypes take the same path
    a = sample_tokens(x.double(), temperature=0.9, top_k=20, seed=1, step=0)
    assert torch.equal(a, sample_tokens(x, temperature=0.9, top_k=20, seed=1, step=0))


# ---- GPT2LMModel.generate(noise_seed=...) ----------------------------------------------------

@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2,
                       vocab_size=300, seq_len=64, dropout=0.0, precision="fp32").eval()


def test_generate_with_noise_seed_equals_the_written_out_loop(model):
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 300, (3, 10), generator=g)
    lens = torch.tensor([3, 7, 10], dtype=torch.int32)
    kw = dict(temperature=0.9, top_k=40, top_p=0.95)
    gen = torch.Generator().manual_seed(5)
    state = gen.get_state()
    a, na = model.generate(ids, lens, 8, noise_seed=11, row_base=4, generator=gen, **kw)
    assert torch.equal(gen.get_state(), state)  # the generator is not touched
    b, nb = model.generate(ids, lens, 8, noise_seed=11, row_base=4, **kw)
    assert torch.equal(a, b) and torch.equal(na, nb) and na.tolist() == [8] * 3
    assert not torch.equal(a, model.generate(ids, lens, 8, noise_seed=12, row_base=4, **kw)[0])
    assert not torch.equal(a, model.generate(ids, lens, 8, noise_seed=11, row_base=5, **kw)[0])
    cache = model.init_cache(3, 18)
    logits = model.prefill(ids, lens, cache)
    toks = []
    for t in range(8):
        toks.append(sample_tokens(logits, seed=11, step=t, row_base=4, **kw))
        if t < 7:
            logits = model.decode_step(toks[-1], cache)
    assert torch.equal(a, torch.stack(toks, 1))
    # without noise_seed the loop is the generator's, as before
    c = model.generate(ids, lens, 8, generator=torch.Generator().manual_seed(5), **kw)[0]
    d = model.generate(ids, lens, 8, generator=torch.Generator().manual_seed(5), noise_seed=None, **kw)[0]
    assert torch.equal(c, d) and not torch.equal(c, a)
    # temperature 0 stays greedy whatever the seed
    assert torch.equal(model.generate(ids, lens, 8, temperature=0, noise_seed=11)[0],
                       model.generate(ids, lens, 8, temperature=0)[0])


def test_generate_with_noise_seed_parks_a_row_at_eos(model):
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 300, (3, 6), generator=g)
    lens = torch.tensor([6, 4, 6], dtype=torch.int32)
    kw = dict(temperature=0.9, top_k=40, noise_seed=11)
    free, _ = model.generate(ids, lens, 6, **kw)
    eos = int(free[0, 2])
    first = free[0].tolist().index(eos)
    cache = model.init_cache(3, 12)
    toks, new_lens = model.generate(ids, lens, 6, eos_id=eos, cache=cache, check_every=2, **kw)
    assert toks[0].tolist() == free[0, :first + 1].tolist() + [eos] * (5 - first)
    assert new_lens[0] == first + 1 and cache.lens[0] == -1
    for b in (1, 2):
        row = free[b].tolist()
        cut = row.index(eos) + 1 if eos in row else 6
        assert toks[b].tolist() == row[:cut] + [eos] * (6 - cut) and new_lens[b] == cut


# ---- python -m run.generate --noise philox ---------------------------------------------------

def test_run_generate_with_philox_noise(tmp_path):
    """A 2-step tiny GPT-2 training run on the CPU, then ``python -m run.generate --noise philox``."""
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

    def generate(out, *extra, ok=True, cfg=ck / "training_args.json"):
        s = subprocess.run([sys.executable, "-m", "run.generate", "--config_json", str(cfg),
                            "--model_path", str(ck), "--out_path", str(out), "--batch_size", "3",
                            "--num_batches", "2", "--prompt_len", "8", "--max_new_tokens", "6", *extra],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert (s.returncode == 0) == ok, s.stdout[-3000:] + s.stderr[-3000:]
        return ([json.loads(line) for line in open(out)] if ok else None), s.stdout + s.stderr

    rows, _ = generate(tmp_path / "a.jsonl", "--noise", "philox", "--top_k", "20")
    assert len(rows) == 6 and all(0 <= i < 200 for row in rows for i in row["continuation"])
    assert generate(tmp_path / "b.jsonl", "--noise", "philox", "--top_k", "20")[0] == rows
    assert generate(tmp_path / "c.jsonl", "--noise", "philox", "--top_k", "20", "--seed", "7")[0] != rows
    # the default is the generator path, and a different stream
    torch_rows = generate(tmp_path / "d.jsonl", "--top_k", "20")[0]
    assert generate(tmp_path / "e.jsonl", "--noise", "torch", "--top_k", "20")[0] == torch_rows != rows
    # rejected before any checkpoint is read
    _, log = generate(tmp_path / "f.jsonl", "--noise", "nope", ok=False)
    assert "nope" in log and "### loading" not in log
    # the settings round-trip through --config_json
    cfg = json.load(open(ck / "training_args.json"))
    cfg.update(noise="philox", top_k=20)
    (tmp_path / "philox.json").write_text(json.dumps(cfg))
    assert generate(tmp_path / "g.jsonl", cfg=tmp_path / "philox.json")[0] == rows
    cfg["noise"] = "nope"
    (tmp_path / "nope.json").write_text(json.dumps(cfg))
    _, log = generate(tmp_path / "h.jsonl", ok=False, cfg=tmp_path / "nope.json")
    assert "nope" in log and "### loading" not in log
