"""Several samples per prompt on the CPU: the PyTorch ``attention_decode_grouped`` against float64, ``decode_step`` over a
``GroupKVCache`` against the plain cache on repeated prompts, ``generate_samples``, ``run.generate --num_samples``."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops.decode import attention_decode_grouped
from run.generate import create_parser, main
from test_attn_decode_grouped_gpu import ref64_grouped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLENS, G = [3, 7, 12, 1], 3


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2,
                       vocab_size=300, seq_len=64, dropout=0.0, precision="fp32").eval()


def test_torch_attention_decode_grouped_matches_float64():
    B, H, D, Lp, Ls, g = 3, 2, 16, 9, 5, torch.Generator().manual_seed(1)
    R, pl, sl = B * G, [0, 9, 10], [0, 4, -1, 2, 5, 3, 1, 1, 1]  # group 2's prefix length is out of range
    qkv, kp, vp = torch.randn(R, 3 * H * D, generator=g), *(torch.randn(B, H, Lp, D, generator=g) for _ in range(2))
    ks, vs = (torch.randn(R, H, Ls, D, generator=g) for _ in range(2))
    for c, ns in ((kp, pl), (vp, pl), (ks, sl), (vs, sl)):
        for i, n in enumerate(ns):
            c[i, :, max(n, 0):] = float("nan")
    before = [t.clone() for t in (kp, vp, ks, vs)]
    plens, slens = torch.tensor(pl, dtype=torch.int32), torch.tensor(sl, dtype=torch.int32)
    out = attention_decode_grouped(qkv, kp, vp, plens, ks, vs, slens, H, group=G)
    want, held = ref64_grouped(qkv, before[0], before[1], pl, before[2], before[3], sl, H, G)
    assert sorted(held) == [0, 1, 3, 5] and (out.double() - want).abs().max() < 1e-5 and not out[[2, 4, 6, 7, 8]].any()
    for r in held:  # the append, and nothing else
        before[2][r, :, sl[r]], before[3][r, :, sl[r]] = qkv.view(R, 3, H, D)[r, 1], qkv.view(R, 3, H, D)[r, 2]
    assert all(torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)) for a, b in zip(before, (kp, vp, ks, vs)))
    assert plens.tolist() == pl and slens.tolist() == sl
    with pytest.raises(ValueError):
        attention_decode_grouped(qkv, kp, vp, plens, ks, vs, slens, H, group=2)


def test_grouped_decode_step_logits_match_the_plain_cache(model):
    gen = torch.Generator().manual_seed(2)
    ids, cont = torch.randint(0, 300, (4, 12), generator=gen), torch.randint(0, 300, (4 * G, 6), generator=gen)
    lens = torch.tensor(PLENS)
    plain, group = model.init_cache(4 * G, 18), model.init_group_cache(4, G, 12, 6)
    a = model.prefill(ids.repeat_interleave(G, 0), lens.repeat_interleave(G), plain)
    b = model.prefill(ids, lens, group.prefix).repeat_interleave(G, 0)
    err = (a - b).abs().max().item()
    for t in range(6):
        err = max(err, (model.decode_step(cont[:, t], plain) - model.decode_step(cont[:, t], group)).abs().max().item())
    assert err <= 1e-4, err
    with pytest.raises(ValueError):
        model.init_group_cache(4, G, 12, 6, kv_dtype="fp8")


def test_greedy_generate_samples_equals_generate(model):
    ids = torch.randint(0, 300, (4, 12), generator=torch.Generator().manual_seed(2))
    toks, new_lens = model.generate(ids, torch.tensor(PLENS), 10, temperature=0)
    margin = float("inf")
    with torch.no_grad():
        for b, p in enumerate(PLENS):
            top = model(torch.cat([ids[b, :p], toks[b]])[None])[0, p - 1:p + 9].topk(2, -1).values
            margin = min(margin, (top[:, 0] - top[:, 1]).min().item())
    assert margin > 1e-3, margin  # no arg-max hangs on the rounding of either path
    got, got_lens = model.generate_samples(ids, torch.tensor(PLENS), 10, num_samples=2, temperature=0)
    assert torch.equal(got, toks[:, None].expand(4, 2, 10)) and got_lens.tolist() == [[10, 10]] * 4


def test_run_generate_num_samples(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1", WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck = tmp_path / "ck"

    def run(module, *flags):
        s = subprocess.run([sys.executable, "-m", module, *flags], cwd=str(tmp_path), env=env, capture_output=True,
                           text=True, timeout=240)
        assert s.returncode == 0, s.stdout[-3000:] + s.stderr[-3000:]

    run("run.train", "--model", "gpt2", "--config_name", "tiny", "--vocab_size", "200", "--seq_len", "32", "--dropout",
        "0.0", "--precision", "fp32", "--dataset", "synthetic", "--data_loader_workers", "0", "--batch_size", "4",
        "--microbatch", "4", "--learning_steps", "2", "--save_interval", "2", "--log_interval", "1", "--eval_interval",
        "100", "--ema_rate", "0.9", "--checkpoint_path", str(ck))

    def generate(name, cfg, *extra):
        run("run.generate", "--config_json", str(cfg), "--model_path", str(ck), "--num_batches", "2", "--prompt_len", "8",
            "--max_new_tokens", "6", "--out_path", str(tmp_path / name), *extra)
        return open(tmp_path / name, "rb").read()

    cfg = ck / "training_args.json"
    plain = generate("a.jsonl", cfg, "--batch_size", "3", "--noise", "philox")
    assert generate("b.jsonl", cfg, "--batch_size", "3", "--noise", "philox", "--num_samples", "1") == plain
    three = generate("c.jsonl", cfg, "--batch_size", "3", "--noise", "philox", "--num_samples", "3")
    rows = [json.loads(line) for line in three.splitlines()]
    assert len(rows) == 6 and all(len(row["samples"]) == 3 and row["samples"][0] == row["continuation"] for row in rows)
    assert rows[0]["continuation"] == json.loads(plain.splitlines()[0])["continuation"]  # both draw with row 0
    both = tmp_path / "both.json"  # the round trip through --config_json, at another batch size
    both.write_text(json.dumps(dict(json.load(open(cfg)), num_samples=3, noise="philox")))
    assert generate("d.jsonl", both, "--batch_size", "2", "--num_batches", "3") == three

    # rejected before a checkpoint is opened: the path does not exist, and it is the settings that raise
    for bad in ("--num_samples 0", "--num_beams 2", "--lookahead 2 --temperature 0", "--kv_dtype fp8", "--logprobs true",
                "--repetition_penalty 1.2", "--presence_penalty 0.5", "--frequency_penalty 0.5", "--no_repeat_ngram 2",
                "--min_new_tokens 2 --eos_id 5", "--temperature 0"):
        flags = ["--num_samples", "2", *bad.split()] if "num_samples" not in bad else bad.split()
        with pytest.raises(ValueError, match="num_samples"):
            main(create_parser().parse_args(["--config_json", str(cfg), "--model_path", str(tmp_path / "none"), *flags]))
