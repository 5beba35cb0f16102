"""``ops.decode.linear_rows_fp8`` and ``decode_linears="rows_fp8"`` where no kernel runs, and ``run.generate`` with it."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops.decode import kv_dequantize, kv_quantize_ref, linear_rows_fp8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = {"none": lambda t: t, "gelu": F.gelu, "tanh": torch.tanh, "silu": F.silu}


@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_rows_fp8_cpu_is_the_definition(dtype, act):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 96, generator=g).to(dtype)
    w = torch.randn(33, 96, generator=g) / 96 ** 0.5
    w[4] = 0.0
    codes, exp = kv_quantize_ref(w)
    assert not codes[4].any() and exp[4] == 0
    for bias in (None, torch.randn(33, generator=g).to(dtype)):
        want = ACTS[act](F.linear(x.float(), kv_dequantize(codes, exp), None if bias is None else bias.float())).to(dtype)
        got = linear_rows_fp8(x, codes, exp, bias, act=act)
        assert got.dtype == dtype and torch.equal(got, want)
    assert linear_rows_fp8(x[:0], codes, exp).shape == (0, 33)
    for bad in (lambda: linear_rows_fp8(x, codes[:, :64], exp), lambda: linear_rows_fp8(x, codes, exp[:32]),
                lambda: linear_rows_fp8(x, codes.float(), exp), lambda: linear_rows_fp8(x, codes, exp, act="relu")):
        with pytest.raises(ValueError):
            bad()


def _tiny():
    torch.manual_seed(0)
    model = build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2, vocab_size=300,
                        seq_len=64, dropout=0.0, precision="fp32").eval()
    ids = torch.randint(0, 300, (3, 12), generator=torch.Generator().manual_seed(1))
    return model, ids, torch.tensor([12, 5, 1], dtype=torch.int32)


def test_rows_fp8_model_snapshot_and_bad_mode():
    model, ids, lens = _tiny()
    with torch.no_grad():
        for name, p in model.named_parameters():  # fixed points of the format: both modes see the same weight values
            if p.dim() == 2 and "wpe" not in name:
                p.copy_(kv_dequantize(*kv_quantize_ref(p)))
    cache = model.init_cache(3, 16)
    model.prefill(ids, lens, cache)
    buf, at = cache.buf.clone(), cache.lens.clone()

    def step(**kw):  # one decode step from the same prefilled cache, whatever the weights have become since
        cache.buf.copy_(buf), cache.lens.copy_(at)
        return model.decode_step(ids[:, 0], cache, **kw)

    plain = step()
    fp8 = step(decode_linears="rows_fp8")  # builds the snapshot on first use
    assert torch.allclose(fp8, plain, rtol=1e-4, atol=1e-4) and "_decode_w8" not in "".join(model.state_dict())
    with torch.no_grad():
        model.h[0].mlp_fc.weight.mul_(2.0)
    assert torch.equal(step(decode_linears="rows_fp8"), fp8)  # the snapshot, not the new weight
    model.quantize_decode_weights()
    again = step(decode_linears="rows_fp8")
    assert torch.allclose(again, step(), rtol=1e-4, atol=1e-4) and not torch.equal(again, fp8)
    for call in (lambda **kw: model.generate(ids, lens, 4, temperature=0, **kw),
                 lambda **kw: model.beam_search(ids, lens, 4, num_beams=2, **kw),
                 lambda **kw: model.generate_lookahead(ids, lens, 4, lookahead=3, **kw),
                 lambda **kw: model.generate_samples(ids, lens, 4, num_samples=2, temperature=0, **kw)):
        assert call(decode_linears="rows_fp8")[0].shape[-1] == 4
        with pytest.raises(ValueError, match="decode_linears"):
            call(decode_linears="nope")


def test_run_generate_rows_fp8(tmp_path):
    """A 2-step tiny GPT-2 training run on the CPU, then ``python -m run.generate --decode_linears rows_fp8``."""
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
    for mode, ok in (("rows_fp8", True), ("nope", False)):
        s = subprocess.run([sys.executable, "-m", "run.generate", "--config_json", str(ck / "training_args.json"),
                            "--model_path", str(ck), "--out_path", str(tmp_path / "out.jsonl"), "--batch_size", "3",
                            "--num_batches", "2", "--prompt_len", "8", "--max_new_tokens", "6", "--temperature", "0",
                            "--decode_linears", mode], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        log = s.stdout + s.stderr
        assert (s.returncode == 0) == ok, log[-3000:]
        if ok:
            assert len((tmp_path / "out.jsonl").read_text().splitlines()) == 6
        else:  # rejected before the checkpoint is read
            assert "decode_linears" in log and "### loading" not in log
