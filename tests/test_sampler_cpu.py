"""Respaced / DDIM DiffuSeq sampling on the CPU (fp32 PyTorch path): the schedule of
``GaussianDiffusion.reverse_schedule``, ``sample_seq2seq`` with ``steps`` / ``sampler`` / ``top_p``
/ ``noise_seed``, MBR selection (utils/mbr.py) and the new ``python -m run.sample`` flags.

Tiny model as in test_decode_cpu.py: vocabulary 100, 16 positions, 8 diffusion steps, fp32."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_pipeline_amd.models import TransformerNetModel, create_gaussian_diffusion
from distributed_pipeline_amd.ops import diffusion as dops
from utils.mbr import mbr_select, sentence_bleu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, L, E, T = 100, 16, 16, 8


def _model(seed=0):
    torch.manual_seed(seed)
    m = TransformerNetModel(vocab_size=V, input_dims=E, hidden_t_dim=16, seq_len=L, config_name="tiny",
                            dropout=0.0, compute_dtype=torch.float32)
    with torch.no_grad():  # rows of one norm: a row's own logit beats every other row's clearly
        w = torch.randn(V, E)
        m.word_embedding.weight.copy_(4.0 * w / w.norm(dim=-1, keepdim=True))
        m.lm_head.bias.copy_(0.1 * torch.randn(V))
    return m.eval()


def _batch(B=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    mask[:, 6:] = 1
    return {"input_ids": ids, "input_mask": mask}


class _Oracle(torch.nn.Module):
    """Predicts the true x_start whatever it is given; decoding helpers come from ``module``."""

    def __init__(self, net, x_start):
        super().__init__()
        self.module, self.x_start, self.ts = net, x_start, []

    def forward(self, x, t):
        self.ts.append(float(t[0]))
        return self.x_start.to(x.dtype)


# ---- schedule ------------------------------------------------------------------------------
def test_kept_timesteps():
    d = create_gaussian_diffusion(steps=2000)
    assert d.kept_timesteps(2) == [0, 1999]
    assert d.kept_timesteps(3) == [0, 1000, 1999]  # (2 * 1999 + 2) // 4 = 1000
    assert d.kept_timesteps(2000) == list(range(2000))
    k = d.kept_timesteps(200)
    assert len(k) == 200 and k[0] == 0 and k[-1] == 1999 and all(b > a for a, b in zip(k, k[1:]))
    assert k == [(2 * i * 1999 + 199) // 398 for i in range(200)]
    sched = d.reverse_schedule(200)
    assert [row[0] for row in sched] == k[::-1]
    for bad in (0, 1, 2001, -3):
        with pytest.raises(ValueError):
            d.reverse_schedule(bad)
    with pytest.raises(ValueError):
        d.reverse_schedule(4, "heun")


@pytest.mark.parametrize("sigma_small", [False, True])
def test_full_chain_ancestral_equals_the_tables(sigma_small):
    d = create_gaussian_diffusion(steps=2000, sigma_small=sigma_small)
    for sched in (d.reverse_schedule(), d.reverse_schedule(2000, "ancestral")):
        t, a, b, s = (np.array(col) for col in zip(*sched[::-1]))
        assert t.tolist() == list(range(2000))
        np.testing.assert_allclose(a, d.posterior_mean_coef1, rtol=0, atol=1e-12)
        np.testing.assert_allclose(b, d.posterior_mean_coef2, rtol=0, atol=1e-12)
        var = d.posterior_variance if sigma_small else d.betas
        np.testing.assert_allclose(s[1:] ** 2, var[1:], rtol=0, atol=1e-12)
        assert s[0] == 0.0  # the last update (t = 0) adds no noise


@pytest.mark.parametrize("steps", [3, 200, 2000])
def test_ddim_eta_one_is_ancestral_with_the_small_variance(steps):
    d = create_gaussian_diffusion(steps=2000, sigma_small=True)
    anc = np.array(d.reverse_schedule(steps, "ancestral"))
    ddim = np.array(d.reverse_schedule(steps, "ddim", 1.0))
    np.testing.assert_allclose(ddim, anc, rtol=0, atol=1e-12)
    det = np.array(d.reverse_schedule(steps, "ddim", 0.0))
    assert (det[:, 3] == 0).all() and anc[-1, 3] == 0 and (anc[:-1, 3] > 0).all()
    # the last update returns the prediction itself
    np.testing.assert_allclose(det[-1, 1:3], [1.0, 0.0], atol=1e-12)
    np.testing.assert_allclose(anc[-1, 1:3], [1.0, 0.0], atol=1e-12)


# ---- op (PyTorch path) ------------------------------------------------------------------------
def test_reverse_step_pytorch_path_formula_and_noise():
    g = torch.Generator().manual_seed(0)
    x, xs, pred = (torch.randn(2, 5, 8, generator=g) for _ in range(3))
    mask = torch.tensor([[0, 0, 1, 1, 1], [0, 1, 1, 1, 0]])
    W = torch.randn(7, 8, generator=g)
    idx = torch.tensor([[0, 1, 2, 3, 7], [6, -1, 5, 4, 3]])
    z = torch.randn(2, 5, 8, generator=g)
    kw = dict(x_start=xs, mask=mask, a=0.3, b=0.6, s=0.2, seed=4, step=2)
    out, o16 = dops.reverse_step(x, pred=pred, noise=z, want_bf16=True, **kw)
    ref = torch.where(mask.unsqueeze(-1) == 0, xs, 0.3 * pred + 0.6 * x + 0.2 * z)
    torch.testing.assert_close(out, ref)
    assert torch.equal(o16, out.to(torch.bfloat16))
    out, o16 = dops.reverse_step(x, idx=idx, weight=W, scale=2.5, noise=z, **kw)
    ok = ((idx >= 0) & (idx < 7)).unsqueeze(-1)
    x0 = 2.5 * W[idx.clamp(0, 6)] * ok
    torch.testing.assert_close(out, torch.where(mask.unsqueeze(-1) == 0, xs, 0.3 * x0 + 0.6 * x + 0.2 * z))
    assert o16 is None
    # own noise: reproducible per (seed, step), different across them, truncated by top_p
    draw = lambda **k: dops.reverse_step(None, x_start=xs, mask=torch.ones_like(mask), a=0.0, b=0.0, s=1.0,  # noqa: E731
                                         **{**dict(seed=4, step=2), **k})[0]
    assert torch.equal(draw(), draw())
    assert not torch.equal(draw(), draw(seed=5)) and not torch.equal(draw(), draw(step=3))
    zt = draw(top_p=0.9)
    assert float(zt.abs().max()) <= 0.9 and float(zt.abs().max()) > 0.6
    with pytest.raises(ValueError):
        dops.reverse_step(None, a=0.0, b=0.0, s=1.0, seed=0, step=0)
    with pytest.raises(ValueError):
        dops.reverse_step(None, x_start=xs, a=0.0, b=1.0, s=0.0, seed=0, step=0)


def test_truncated_noise_has_the_truncated_normal_moments():
    g = torch.Generator().manual_seed(1)
    z = dops.draw_noise((1 << 18,), torch.device("cpu"), g, 2.0).double()
    assert float(z.abs().max()) <= 2.0
    n = z.numel()
    assert abs(float(z.mean())) < 6 * (0.77374 / n) ** 0.5
    assert abs(float(z.var()) / 0.77374 - 1) < 0.02  # 1 - 2 tau phi(tau) / erf(tau / sqrt 2); s.e. ~ 0.3%


# ---- sampler ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ancestral", "ddim"])
@pytest.mark.parametrize("noise_seed", [None, 11])
def test_oracle_model_recovers_the_input(sampler, noise_seed):
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    oracle = _Oracle(net, net.get_embeds(batch["input_ids"]).detach())
    out = diff.sample_seq2seq(oracle, batch, steps=3, sampler=sampler, eta=0.5, top_p=0.9, noise_seed=noise_seed,
                              generator=torch.Generator().manual_seed(3))
    assert set(out) == {"tokens", "x0", "source_mask"}
    assert torch.equal(out["tokens"], batch["input_ids"])
    assert torch.equal(out["source_mask"], batch["input_mask"] == 0)
    # the model is asked at the ORIGINAL timesteps of the 3 kept steps, rescaled to 1000
    assert oracle.ts == [k * 1000.0 / T for k in (7, 4, 0)]


def test_noise_seed_path_reproduces_and_depends_on_the_seed():
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    run = lambda s, **k: diff.sample_seq2seq(net, batch, steps=4, sampler="ddim", eta=1.0, noise_seed=s, **k)  # noqa: E731
    a, b, c = run(5), run(5), run(6)
    assert a["x0"].shape == (4, L, E) and a["x0"].dtype == torch.float32
    src = batch["input_mask"] == 0
    assert torch.equal(a["tokens"][src], batch["input_ids"][src])
    assert torch.equal(a["x0"][src], net.get_embeds(batch["input_ids"])[src])
    assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["x0"], b["x0"])
    assert not torch.equal(a["x0"], c["x0"])


def test_default_call_is_the_full_ancestral_loop():
    """No new keyword: exactly p_sample_loop's result (the path test_decode_cpu.py pins)."""
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    a = diff.sample_seq2seq(net, batch, generator=torch.Generator().manual_seed(5))
    x_start = net.get_embeds(batch["input_ids"])
    c = net.rounding_offsets()
    x0 = diff.p_sample_loop(net, x_start.shape, mask=batch["input_mask"], x_start=x_start,
                            denoised_fn=lambda x, t: net.round_to_embeds(x, c),
                            generator=torch.Generator().manual_seed(5))
    assert torch.equal(a["x0"], x0)


@pytest.mark.parametrize("noise_seed", [None, 2])
@pytest.mark.parametrize("clamp_step,expect", [(None, 3), (-1, 0), (0, 1), (3, 1), (4, 2), (7, 3)])
def test_clamp_step_counts_against_original_timesteps(noise_seed, clamp_step, expect):
    """3 kept steps of T = 8 are the original timesteps 7, 4, 0."""
    net, batch = _model(), _batch(2)
    diff = create_gaussian_diffusion(steps=T)
    counted = []
    orig = net.nearest_tokens
    net.nearest_tokens = lambda x, c=None: (counted.append(1), orig(x, c))[1]
    diff.sample_seq2seq(net, batch, steps=3, clamp_step=clamp_step, noise_seed=noise_seed)
    assert len(counted) == expect


# ---- MBR ----------------------------------------------------------------------------------------
def test_sentence_bleu_and_mbr_select():
    assert sentence_bleu([1, 2, 3, 4], [1, 2, 3, 5]) == pytest.approx(0.1875 ** 0.25, abs=1e-12)
    assert sentence_bleu([1, 2, 3, 4], [1, 2, 3, 4]) == pytest.approx(1.0, abs=1e-12)
    assert sentence_bleu([], [1, 2]) == 0.0 and sentence_bleu([7, 8], [1, 2]) == 0.0
    # brevity penalty: a 2-token prefix of a 4-token reference
    assert sentence_bleu([1, 2], [1, 2, 3, 4]) == pytest.approx(
        np.exp(1 - 4 / 2) * (1.0 * (2 / 2) * (1 / 1) * (1 / 1)) ** 0.25, abs=1e-12)
    A, B = [5, 6, 7, 8, 9], [5, 6, 1, 2, 3]
    assert mbr_select([A, A, B]) == 0 and mbr_select([B, A, A]) == 1
    assert mbr_select([A, A, A]) == 0 and mbr_select([A]) == 0
    assert mbr_select([[], [], []]) == 0


# ---- entry point ----------------------------------------------------------------------------------
def test_sample_settings_defaults_of_the_new_flags():
    from config.sample import SampleSettings
    from config.train import TrainSettings
    s = SampleSettings()
    assert (s.step, s.sampler, s.ddim_eta, s.top_p, s.mbr, s.noise, s.keep_candidates) == (
        0, "ancestral", 0.0, 0.0, 1, "torch", False)
    for name in ("step", "sampler", "ddim_eta", "top_p", "mbr", "noise", "keep_candidates"):
        assert name not in TrainSettings.model_fields
    p = SampleSettings.to_argparse(add_json=True)
    s = SampleSettings.from_argparse(p.parse_args(["--step", "4", "--sampler", "ddim", "--noise", "philox",
                                                   "--keep_candidates", "true"]))
    assert (s.step, s.sampler, s.noise, s.keep_candidates) == (4, "ddim", "philox", True)
    with pytest.raises(SystemExit):
        p.parse_args(["--sampler", "heun"])


def test_run_sample_mbr_candidates_are_the_single_seed_runs(tmp_path):
    """A 2-step tiny training run, then ``run.sample --mbr 3 --noise philox`` on a 6-line jsonl
    split (the synthetic dataset draws other samples for another seed): candidate c is the
    ``recover`` of a ``--mbr 1`` run with seed + c."""
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1", WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck = tmp_path / "ck"
    words = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu".split()
    with open(tmp_path / "test.jsonl", "w") as f:  # hashed word ids (no vocab.txt): 1000 .. 1199
        for i in range(6):
            f.write(json.dumps({"src": " ".join(words[i:i + 4]), "trg": " ".join(words[i + 3:i + 7])}) + "\n")
    common = ["--model", "diffuseq", "--config_name", "tiny", "--vocab_size", "1200", "--seq_len", "16",
              "--hidden_dim", "16", "--hidden_t_dim", "16", "--dropout", "0.0", "--diffusion_steps", "8",
              "--precision", "fp32", "--dataset", "synthetic", "--data_loader_workers", "0"]
    r = subprocess.run([sys.executable, "-m", "run.train", *common, "--batch_size", "4", "--microbatch", "4",
                        "--learning_steps", "2", "--save_interval", "2", "--log_interval", "1",
                        "--eval_interval", "100", "--ema_rate", "0.9", "--checkpoint_path", str(ck)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def sample(out, *extra):
        s = subprocess.run([sys.executable, "-m", "run.sample", "--config_json", str(ck / "training_args.json"),
                            "--model_path", str(ck), "--out_path", str(out), "--batch_size", "3",
                            "--num_batches", "2", "--step", "4", "--sampler", "ddim", "--ddim_eta", "1.0",
                            "--top_p", "0.9", "--noise", "philox", "--dataset", "jsonl",
                            "--data_dir", str(tmp_path), *extra],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert s.returncode == 0, s.stdout[-3000:] + s.stderr[-3000:]
        return [json.loads(line) for line in open(out)]

    rows = sample(tmp_path / "mbr.jsonl", "--mbr", "3", "--seed", "102")
    assert len(rows) == 6
    for row in rows:
        assert set(row) == {"source", "reference", "recover"}
        assert all(isinstance(i, int) and 0 <= i < 1200 for k in row for i in row[k])
    kept = sample(tmp_path / "kept.jsonl", "--mbr", "3", "--seed", "102", "--keep_candidates", "true")
    singles = [sample(tmp_path / f"s{c}.jsonl", "--seed", str(102 + c)) for c in range(3)]
    for i, row in enumerate(kept):
        assert set(row) == {"source", "reference", "recover", "candidates"}
        assert row["candidates"] == [singles[c][i]["recover"] for c in range(3)]
        assert row["recover"] == row["candidates"][mbr_select(row["candidates"])] == rows[i]["recover"]
        assert row["source"] == rows[i]["source"] == singles[0][i]["source"]
    assert len({json.dumps(r_["recover"]) for s_ in singles for r_ in s_}) > 1  # the seeds differ
