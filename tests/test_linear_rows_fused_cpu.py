"""``linear_rows(ln=, residual=)`` and ``decode_linears="rows_fused"`` where no kernel runs, and ``run.generate`` with it."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_pipeline_amd.ops.decode import linear_rows
from test_linear_rows_fp8_cpu import _tiny  # (fp32 tiny GPT-2 on the CPU, ids, lens)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ln,res", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pytorch_path_matches_float64(dtype, ln, res):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(5, 96, generator=g) + 50).to(dtype)
    w, b = (torch.randn(33, 96, generator=g) / 96 ** 0.5).to(dtype), torch.randn(33, generator=g).to(dtype)
    gm, bt, r = torch.randn(96, generator=g).to(dtype), torch.randn(96, generator=g).to(dtype), torch.randn(5, 33, generator=g).to(dtype)
    got = linear_rows(x, w, b, act="gelu", ln=(gm, bt, 1e-5) if ln else None, residual=r if res else None)
    a = F.layer_norm(x.double(), (96,), gm.double(), bt.double(), 1e-5) if ln else x.double()
    want = F.gelu(F.linear(a, w.double(), b.double())) + (r.double() if res else 0)
    # fp32: sums of 96 terms; bf16: a and y rounded once each (2^-8 relative), a's rounding seen through |W| ~ 1 per row
    tol = 1e-4 if dtype == torch.float32 else 2.0 ** -7 * (want.abs() + a.abs().max())
    assert got.dtype == dtype and ((got.double() - want).abs() <= tol).all()


def test_rows_fused_on_the_cpu_is_tile():
    model, ids, lens = _tiny()
    for a, b in zip(model.generate(ids, lens, 6, temperature=0, decode_linears="rows_fused"),
                    model.generate(ids, lens, 6, temperature=0)):
        assert torch.equal(a, b)


def test_run_generate_rows_fused(tmp_path):
    """A 2-step tiny GPT-2 run on the CPU, then ``run.generate`` with the mode as a flag and through ``--config_json``."""
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1", WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck = tmp_path / "ck"
    train = ("--model gpt2 --config_name tiny --vocab_size 200 --seq_len 32 --dropout 0.0 --precision fp32 --dataset synthetic "
             "--data_loader_workers 0 --batch_size 4 --microbatch 4 --learning_steps 2 --save_interval 2 --log_interval 1 "
             "--eval_interval 100 --ema_rate 0.9 --checkpoint_path").split() + [str(ck)]
    r = subprocess.run([sys.executable, "-m", "run.train"] + train, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    cfg = dict(json.loads((ck / "training_args.json").read_text()), decode_linears="rows_fused")
    (tmp_path / "gen.json").write_text(json.dumps(cfg))
    outs = []
    for extra in (["--config_json", str(ck / "training_args.json"), "--decode_linears", "rows_fused"],
                  ["--config_json", str(tmp_path / "gen.json")]):
        s = subprocess.run([sys.executable, "-m", "run.generate", "--model_path", str(ck), "--out_path",
                            str(tmp_path / "out.jsonl"), "--batch_size", "3", "--num_batches", "2", "--prompt_len", "8",
                            "--max_new_tokens", "6", "--temperature", "0"] + extra, cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=240)
        assert s.returncode == 0, (s.stdout + s.stderr)[-3000:]
        outs.append((tmp_path / "out.jsonl").read_text())
    assert len(outs[0].splitlines()) == 6 and outs[0] == outs[1]
