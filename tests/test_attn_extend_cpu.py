"""``ops.decode.attention_extend`` (its PyTorch twin), ``GPT2LMModel.extend`` / ``prefill(chunk=C)`` /
``generate(prefill_chunk=C)`` in fp32 on the CPU, and ``python -m run.generate --prefill_chunk``."""
import json
import os
import subprocess
import sys

import pytest
import torch

from decode_block_helpers import block_counts, ref64_block
from decode_helpers import TINY, guarded_caches
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops.decode import attention_extend, attention_extend_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T", [1, 9, 40])
def test_ref_against_float64(T):
    H, D, Lmax = 2, 16, 64
    g = torch.Generator().manual_seed(T)
    lens, counts = [0, 7, 30, -1, Lmax, Lmax - 5], [T, T + 3, T - 1, T, T, T]
    buf, k, v = guarded_caches(6, H, Lmax, D, "cpu", dtype=torch.float32)
    k.copy_(torch.randn(6, H, Lmax, D, generator=g)), v.copy_(torch.randn(6, H, Lmax, D, generator=g))
    c, n = block_counts(lens, counts, T, Lmax), torch.tensor(lens, dtype=torch.int32)
    for b, m in enumerate(lens):  # what lies at and beyond lens + c_b never reaches the output
        if 0 <= m < Lmax:
            k[b, :, m + c[b]:], v[b, :, m + c[b]:] = float("nan"), float("nan")
    qkv = torch.randn(6, T, 3 * H * D, generator=g)
    want, before = ref64_block(qkv, k, v, lens, H, counts), buf.clone()
    for op in (attention_extend, attention_extend_ref):
        buf.copy_(before)
        out = op(qkv, k, v, n, H, counts=torch.tensor(counts, dtype=torch.int32))
        assert ((out.double() - want).abs() <= 2e-5).all()  # fp32 sums over <= 64 keys of unit-normal values
        expect = before.clone()
        for b, m in enumerate(lens):
            assert not out[b, c[b]:].any()
            for j in range(c[b]):
                expect[0, b, :, 3 + m + j], expect[1, b, :, 3 + m + j] = qkv.view(6, T, 3, H, D)[b, j, 1:].unbind(0)
        assert torch.equal(buf.nan_to_num(7.0), expect.nan_to_num(7.0))
    with pytest.raises(ValueError):
        attention_extend(qkv, k, v, n, H + 1)


def test_model_extend_prefill_and_generate():
    torch.manual_seed(0)
    model = build_model(precision="fp32", num_heads=4, **TINY).eval()
    ids = torch.randint(1000, 3000, (3, 40), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        full, cache = model(ids), model.init_cache(3, 48)
        cache.lens = torch.tensor([0, -1, 0], dtype=torch.int32)
        hid = torch.cat([model.extend(ids[:, :13], cache), model.extend(ids[:, 13:], cache)], 1)  # a warm cache
        assert cache.lens.tolist() == [40, -1, 40]
        assert ((hid @ model.wte.weight.t())[[0, 2]] - full[[0, 2]]).abs().max() < 1e-4
        lens = torch.tensor([40, 1, 22], dtype=torch.int32)
        a, b = (model.prefill(ids, lens, model.init_cache(3, 48), chunk=C) for C in (0, 7))
        top2 = a.topk(2).values
        assert (a - b).abs().max() < 1e-4 and ((top2[:, 0] - top2[:, 1]) > 2e-4).all()
        assert torch.equal(model.generate(ids, lens, 5, temperature=0)[0],
                           model.generate(ids, lens, 5, temperature=0, prefill_chunk=7)[0])
        for call in (lambda c: model.extend(ids, c), lambda c: model.prefill(ids, lens, c, chunk=7)):
            with pytest.raises(ValueError):
                call(model.init_cache(3, 48, kv_dtype="fp8"))


def test_run_generate_prefill_chunk(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck, run = tmp_path / "ck", dict(cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    r = subprocess.run([sys.executable, "-m", "run.train", "--model", "gpt2", "--config_name", "tiny", "--vocab_size",
                        "200", "--seq_len", "32", "--dropout", "0.0", "--precision", "fp32", "--dataset", "synthetic",
                        "--data_loader_workers", "0", "--batch_size", "4", "--microbatch", "4", "--learning_steps", "2",
                        "--save_interval", "2", "--log_interval", "1", "--eval_interval", "100", "--ema_rate", "0.9",
                        "--checkpoint_path", str(ck)], **run)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def generate(name, *extra, ok=True, cfg=ck / "training_args.json"):
        s = subprocess.run([sys.executable, "-m", "run.generate", "--config_json", str(cfg), "--model_path", str(ck),
                            "--out_path", str(tmp_path / name), "--batch_size", "3", "--prompt_len", "20",
                            "--max_new_tokens", "6", "--temperature", "0", *extra], **run)
        assert (s.returncode == 0) == ok, s.stdout[-3000:] + s.stderr[-3000:]
        return open(tmp_path / name, "rb").read() if ok else s.stdout + s.stderr

    plain, chunked = generate("a.jsonl"), generate("c.jsonl", "--prefill_chunk", "8")
    assert generate("b.jsonl", "--prefill_chunk", "0") == plain
    assert [json.loads(x)["prompt"] for x in chunked.splitlines()] == [json.loads(x)["prompt"] for x in plain.splitlines()]
    cfg = dict(json.load(open(ck / "training_args.json")), prefill_chunk=8)  # the round trip through --config_json
    (tmp_path / "chunk.json").write_text(json.dumps(cfg))
    assert generate("d.jsonl", cfg=tmp_path / "chunk.json") == chunked
    for extra in (["--prefill_chunk", "-1"], ["--prefill_chunk", "8", "--kv_dtype", "fp8"],
                  ["--prefill_chunk", "8", "--num_beams", "2"], ["--prefill_chunk", "8", "--lookahead", "4"]):
        log = generate("e.jsonl", *extra, ok=False)
        assert "prefill_chunk" in log and "### loading" not in log
