"""``ops.decode.linear_rows`` and ``decode_linears`` where no kernel runs, and ``run.generate --decode_linears``."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops.decode import linear_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = {"none": lambda t: t, "gelu": F.gelu, "tanh": torch.tanh, "silu": F.silu}


@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_rows_cpu_matches_float64(dtype, act):
    """Bound: K = 96 fp32 roundings of a sum of magnitude below 8, and for bf16 one ulp of the output."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 96, generator=g).to(dtype)
    w = (torch.randn(33, 96, generator=g) / 96 ** 0.5).to(dtype)
    for bias in (None, torch.randn(33, generator=g).to(dtype)):
        want = ACTS[act](F.linear(x.double(), w.double(), None if bias is None else bias.double()))
        got = linear_rows(x, w, bias, act=act)
        tol = (2.0 ** -8 if dtype == torch.bfloat16 else 0.0) * want.abs() + 96 * 2.0 ** -23 * 8
        assert got.dtype == dtype and got.shape == (5, 33) and ((got.double() - want).abs() <= tol).all()
    assert linear_rows(x[:0], w).shape == (0, 33)
    with pytest.raises(ValueError):
        linear_rows(x, w[:, :64])


def test_rows_in_fp32_is_the_default_call():
    torch.manual_seed(0)
    model = build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2, vocab_size=300,
                        seq_len=64, dropout=0.0, precision="fp32").eval()
    ids = torch.randint(0, 300, (3, 12), generator=torch.Generator().manual_seed(1))
    lens = torch.tensor([12, 5, 1], dtype=torch.int32)
    calls = (lambda **kw: model.generate(ids, lens, 8, temperature=0, **kw),
             lambda **kw: model.beam_search(ids, lens, 4, num_beams=2, **kw),
             lambda **kw: model.generate_lookahead(ids, lens, 8, lookahead=3, **kw))
    for call in calls:
        assert torch.equal(call(decode_linears="rows")[0], call()[0])
        with pytest.raises(ValueError, match="decode_linears"):
            call(decode_linears="nope")


def test_run_generate_decode_linears(tmp_path):
    """A 2-step tiny GPT-2 training run on the CPU, then ``python -m run.generate`` with and without the flag."""
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1", WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck = tmp_path / "ck"
    r = subprocess.run([sys.executable, "-m", "run.train", "--model", "gpt2", "--config_name", "tiny", "--vocab_size", "200",
                        "--seq_len", "32", "--dropout", "0.0", "--precision", "fp32", "--dataset", "synthetic",
                        "--data_loader_workers", "0", "--batch_size", "4", "--microbatch", "4", "--learning_steps", "2",
                        "--save_interval", "2", "--log_interval", "1", "--eval_interval", "100", "--ema_rate", "0.9",
                        "--checkpoint_path", str(ck)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def generate(out, *extra, ok=True, cfg=ck / "training_args.json"):
        s = subprocess.run([sys.executable, "-m", "run.generate", "--config_json", str(cfg), "--model_path", str(ck),
                            "--out_path", str(tmp_path / out), "--batch_size", "3", "--num_batches", "2", "--prompt_len", "8",
                            "--max_new_tokens", "6", "--temperature", "0", *extra],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert (s.returncode == 0) == ok, s.stdout[-3000:] + s.stderr[-3000:]
        return (tmp_path / out).read_bytes() if ok else None, s.stdout + s.stderr

    plain, _ = generate("a.jsonl")
    assert generate("b.jsonl", "--decode_linears", "tile")[0] == plain
    rows, log = generate("c.jsonl", "--decode_linears", "rows")
    assert "model_000002.pt" in log and rows == plain and len(rows.splitlines()) == 6  # fp32: both run F.linear
    cfg = dict(json.load(open(ck / "training_args.json")), decode_linears="rows")
    (tmp_path / "rows.json").write_text(json.dumps(cfg))
    assert generate("d.jsonl", cfg=tmp_path / "rows.json")[0] == rows
    _, log = generate("e.jsonl", "--decode_linears", "nope", ok=False)  # rejected before the checkpoint is read
    assert "decode_linears" in log and "### loading" not in log
