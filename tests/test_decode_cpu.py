"""DiffuSeq decoding on the CPU (fp32 PyTorch path): rounding wrappers of the model, the reverse
loop's ``clamp_step`` / ``generator`` keywords, ``sample_seq2seq`` and ``python -m run.sample``.

Tiny model: ``config_name="tiny"``, vocabulary 100, 16 positions, 8 diffusion steps, fp32."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_pipeline_amd.models import TransformerNetModel, create_gaussian_diffusion
from distributed_pipeline_amd.ops import nn as ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, L, E, T = 100, 16, 16, 8


def _model(scale=1.0, seed=0):
    torch.manual_seed(seed)
    m = TransformerNetModel(vocab_size=V, input_dims=E, hidden_t_dim=16, seq_len=L, config_name="tiny",
                            dropout=0.0, compute_dtype=torch.float32, emb_scale_factor=scale)
    with torch.no_grad():
        # rows of one norm (4), so a row's own logit |e|^2 = 16 beats every other row's by a clear
        # margin, as a trained rounding head's does; a small bias that still enters the scores
        w = torch.randn(V, E)
        m.word_embedding.weight.copy_(4.0 * w / w.norm(dim=-1, keepdim=True))
        m.lm_head.bias.copy_(0.1 * torch.randn(V))
    return m.eval()


def _batch(B=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    mask[:, 6:] = 1  # 6 source positions, 10 target positions
    return {"input_ids": ids, "input_mask": mask}


class _Oracle(torch.nn.Module):
    """Predicts the true x_start whatever it is given; decoding helpers come from ``module``."""

    def __init__(self, net, x_start):
        super().__init__()
        self.module, self.x_start = net, x_start

    def forward(self, x, t):
        return self.x_start.to(x.dtype)


@pytest.mark.parametrize("clamp_step", [None, -1])
def test_oracle_model_recovers_the_input(clamp_step):
    """clamp_step None: rounding at every step; -1: t <= -1 never holds, so at none."""
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    oracle = _Oracle(net, net.get_embeds(batch["input_ids"]).detach())
    out = diff.sample_seq2seq(oracle, batch, clamp_step=clamp_step, generator=torch.Generator().manual_seed(3))
    assert set(out) == {"tokens", "x0", "source_mask"}
    assert torch.equal(out["tokens"], batch["input_ids"])
    assert torch.equal(out["source_mask"], batch["input_mask"] == 0)


def test_real_model_reproducible_and_source_kept():
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    run = lambda s: diff.sample_seq2seq(net, batch, generator=torch.Generator().manual_seed(s))  # noqa: E731
    a, b, c = run(5), run(5), run(6)
    assert a["tokens"].shape == (4, L) and a["tokens"].dtype == torch.int64
    assert a["x0"].shape == (4, L, E) and a["x0"].dtype == torch.float32
    src = batch["input_mask"] == 0
    assert torch.equal(a["tokens"][src], batch["input_ids"][src])
    assert int(a["tokens"].min()) >= 0 and int(a["tokens"].max()) < V
    assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["x0"], b["x0"])
    assert not torch.equal(a["x0"], c["x0"])


def test_wrappers_agree_with_brute_force():
    net = _model()
    W, b = net.word_embedding.weight.detach(), net.lm_head.bias.detach()
    x = torch.randn(3, 7, E, generator=torch.Generator().manual_seed(2))
    d2 = ((x.reshape(-1, 1, E) - W.unsqueeze(0)) ** 2).sum(-1)            # [21, V]
    near = d2.argmin(-1).view(3, 7)
    assert (d2.sort(-1).values[:, 1] - d2.sort(-1).values[:, 0]).min() > 1e-3  # no near-ties: argmin is safe
    assert torch.equal(net.nearest_tokens(x), near)
    assert torch.equal(net.nearest_tokens(x, net.rounding_offsets()), near)
    r = net.round_to_embeds(x)
    assert r.dtype == torch.float32 and torch.equal(r, W[near])           # rows of the table, exactly
    logits = x.reshape(-1, E) @ W.t() + b
    assert (logits.sort(-1).values[:, -1] - logits.sort(-1).values[:, -2]).min() > 1e-4
    assert torch.equal(net.decode_tokens(x), logits.argmax(-1).view(3, 7))
    assert torch.equal(net.decode_tokens(x), net.get_logits(x).argmax(-1))


def test_linear_argmax_ties_go_to_the_lowest_index_and_chunks_agree(monkeypatch):
    # small integers: every product and partial sum is exact in fp32, so equal rows score equal
    # whatever order the matmul adds in
    W = torch.randint(-3, 4, (50, E), generator=torch.Generator().manual_seed(4)).float()
    W[[17, 33, 49]] = W[3].clone()
    x = W[[3, 20, 3]].clone()
    idx, best = ops.linear_argmax(x, W, nearest=True)
    assert idx.tolist() == [3, 20, 3]
    assert torch.allclose(best, 0.5 * (x * x).sum(-1))
    monkeypatch.setattr(ops, "_ARGMAX_CHUNK_BYTES", 4 * 50)                # one token per chunk
    idx1, best1 = ops.linear_argmax(x, W, nearest=True)
    assert torch.equal(idx1, idx) and torch.equal(best1, best)
    # precomputed offsets, a bias, and a NaN row: in range, neighbours unaffected
    c = ops.row_half_sqnorm(W)
    assert torch.equal(ops.linear_argmax(x, W, c=c)[0], idx)
    bias = torch.zeros(50)
    bias[7] = 1e3
    assert ops.linear_argmax(x, W, bias)[0].tolist() == [7, 7, 7]
    x[1] = float("nan")
    assert ops.linear_argmax(x, W, nearest=True)[0].tolist() == [3, 0, 3]
    e_idx, e_best = ops.linear_argmax(x[:0], W)
    assert e_idx.shape == (0,) and e_best.shape == (0,)


def test_emb_scale_factor_gives_the_same_tokens_on_scaled_inputs():
    n1, n2 = _model(1.0), _model(2.5)
    assert torch.equal(n1.word_embedding.weight, n2.word_embedding.weight)
    ids = torch.randint(0, V, (2, 9), generator=torch.Generator().manual_seed(7))
    x = n1.get_embeds(ids).detach() + 0.3 * torch.randn(2, 9, E, generator=torch.Generator().manual_seed(8))
    t1 = n1.nearest_tokens(x)
    assert torch.equal(n2.nearest_tokens(2.5 * x), t1)
    assert torch.allclose(n2.round_to_embeds(2.5 * x), 2.5 * n1.round_to_embeds(x))
    assert torch.equal(n2.round_to_embeds(2.5 * x), n2.get_embeds(t1))


@pytest.mark.parametrize("k", [0, 3, T - 1])
def test_clamp_step_k_rounds_k_plus_one_times(k):
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    x_start = net.get_embeds(batch["input_ids"]).detach()
    calls = []

    def fn(x, t):
        calls.append(int(t[0]))
        return x

    diff.p_sample_loop(net, x_start.shape, mask=batch["input_mask"], x_start=x_start, denoised_fn=fn, clamp_step=k)
    assert calls == list(range(k, -1, -1))
    calls.clear()
    diff.p_sample_loop(net, x_start.shape, mask=batch["input_mask"], x_start=x_start, denoised_fn=fn)
    assert len(calls) == T

    counted = []
    orig = net.round_to_embeds
    net.round_to_embeds = lambda x, c=None: (counted.append(1), orig(x, c))[1]
    diff.sample_seq2seq(net, batch, clamp_step=k)
    assert len(counted) == k + 1


def test_sample_settings_accept_a_training_config(tmp_path):
    from config.sample import SampleSettings
    from config.train import TrainSettings
    cfg = tmp_path / "training_args.json"
    cfg.write_text(TrainSettings(vocab_size=200, seq_len=16, diffusion_steps=8, batch_size=4, seed=9).json())
    p = SampleSettings.to_argparse(add_json=True)
    s = SampleSettings.from_argparse(p.parse_args(["--config_json", str(cfg), "--num_batches", "2"]))
    assert (s.vocab_size, s.diffusion_steps, s.batch_size, s.seed, s.num_batches) == (200, 8, 4, 9, 2)
    assert s.split == "test" and s.clamp_step == -1 and s.use_ema == "" and s.model_path == ""
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"vocab_size": 200, "no_such_setting": 1}))
    with pytest.raises(Exception):
        SampleSettings.from_argparse(p.parse_args(["--config_json", str(bad)]))


def test_run_sample_entry_point(tmp_path):
    """A 2-step tiny training run, then ``python -m run.sample`` on its checkpoint directory.
    (Vocabulary 200 here: the synthetic dataset draws its tokens above the [CLS] / [SEP] ids.)"""
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1", WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck = tmp_path / "ck"
    common = ["--model", "diffuseq", "--config_name", "tiny", "--vocab_size", "200", "--seq_len", "16",
              "--hidden_dim", "16", "--hidden_t_dim", "16", "--dropout", "0.0", "--diffusion_steps", "8",
              "--precision", "fp32", "--dataset", "synthetic", "--data_loader_workers", "0"]
    r = subprocess.run([sys.executable, "-m", "run.train", *common, "--batch_size", "4", "--microbatch", "4",
                        "--learning_steps", "2", "--save_interval", "2", "--log_interval", "1",
                        "--eval_interval", "100", "--ema_rate", "0.9", "--checkpoint_path", str(ck)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (ck / "model_000002.pt").exists() and (ck / "ema_0.9_000002.pt").exists()

    def sample(out, *extra):
        s = subprocess.run([sys.executable, "-m", "run.sample", "--config_json", str(ck / "training_args.json"),
                            "--model_path", str(ck), "--out_path", str(out), "--batch_size", "3",
                            "--num_batches", "2", *extra],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert s.returncode == 0, s.stdout[-3000:] + s.stderr[-3000:]
        return [json.loads(line) for line in open(out)], s.stdout

    rows, log = sample(tmp_path / "out.jsonl")
    assert "model_000002.pt" in log
    assert len(rows) == 2 * 3
    for row in rows:
        assert set(row) == {"source", "reference", "recover"}
        assert row["source"][0] == 101 and row["source"][-1] == 102 and 0 not in row["reference"]
        assert all(isinstance(i, int) and 0 <= i < 200 for k in row for i in row[k])
    rows_ema, log_ema = sample(tmp_path / "ema.jsonl", "--use_ema", "0.9", "--clamp_step", "3")
    assert "ema_0.9_000002.pt" in log_ema and len(rows_ema) == 6
    assert [r_["source"] for r_ in rows_ema] == [r_["source"] for r_ in rows]
