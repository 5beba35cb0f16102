"""The one-byte K/V cache on the CPU (the PyTorch path of ``ops.decode``): the quantizer bit for bit
against the independent yardstick of kv_fp8_helpers.py, ``kv_store``, ``attention_decode_fp8`` against
the float64 definition, the model's ``prefill`` / ``decode_step`` / ``generate`` on an fp8 cache against
an uncached forward over the yardstick's dequantized keys and values, and ``python -m run.generate
--kv_dtype``.

Allowed attention error per element: ``2^-8 |o_ref| + 4 e32`` (the rule of test_attn_decode_gpu.py), with
``e32`` the error of the fp32 PyTorch path on the same inputs against the same float64 reference."""
import json
import os
import subprocess
import sys

import pytest
import torch

import kv_fp8_helpers as kv
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops import decode as dec
from distributed_pipeline_amd.ops.decode import token_stats
from utils import lm_sampling as lms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cpu"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [64, 128])
def test_quantizer_bit_for_bit(D, dtype):
    kv.check_quantizer(DEV, D, dtype)


def test_a_row_worked_out_by_hand():
    """The yardstick and the op against a few values worked out by hand."""
    assert [kv.yard_exponent(a) for a in (448.0, 449.0, 224.0, 1.0, 2.0 ** -130, 2.0 ** 120)] == [0, 1, -1, -8, -127, 112]
    vals = [17.0, 19.0, -2.0 ** -10, 1.5 * 2.0 ** -10, 448.0, 2.0 ** -9]
    # 17 -> 16 (0x58, even), 19 -> 20 (0x5a, even), the tie below the smallest subnormal -> -0
    want = [0x58, 0x5A, 0x80, 0x01, 0x7E, 0x01]
    assert kv.yard_round(torch.tensor(vals).double().numpy()).tolist() == want
    row = torch.zeros(64)
    row[:6] = torch.tensor(vals)  # the maximum is 448: e = 0, every element is its own scaled value
    codes, exps = dec.kv_quantize(row)
    assert int(exps) == 0 and codes[:6].tolist() == want and not codes[6:].any()
    assert dec.kv_dequantize(codes, exps)[:6].tolist() == [16.0, 20.0, -0.0, 2.0 ** -9, 448.0, 2.0 ** -9]
    codes, exps = dec.kv_quantize(row * 2.0 ** 13)
    assert int(exps) == 13 and codes[:6].tolist() == want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_store(D, dtype):
    kv.check_kv_store(DEV, D, dtype)


@pytest.mark.parametrize("kind", ["normal", "ramp"])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_attention_matches_float64_and_appends_the_quantized_row(D, kind):
    lens_all = kv.chunk_lens(64 if D == 32 else D)[::2] + [-1, kv.LMAX, kv.LMAX + 5]
    lens_all = lens_all[:len(lens_all) // kv.B * kv.B]
    g = torch.Generator().manual_seed(1000 * D + len(kind))
    runs = [kv.attn_run(D, kind, lens_all[i:i + kv.B], g, DEV, torch.bfloat16, dec.attention_decode_fp8)
            for i in range(0, len(lens_all), kv.B)]
    e32 = max(r["e32"] for r in runs)
    worst = max(kv.within_tolerance(r, e32) for r in runs)
    print(f"attention_decode_fp8 (PyTorch) D={D} {kind}: e32={e32:.3e} worst err/tol={worst:.3f}")
    assert worst <= 1.0, (worst, e32)
    for r in runs:
        want_c, want_e = kv.expected_buffers(r, DEV)
        assert torch.equal(r["cbuf"], want_c) and torch.equal(r["ebuf"], want_e)
        assert r["lens_t"].tolist() == list(r["lens"])
        for b, m in enumerate(r["lens"]):
            if not 0 <= m < kv.LMAX:
                assert not r["out"][b].any()


def test_attention_never_reads_beyond_lens_and_repeats_bitwise():
    lens = (0, 33, 300)
    outs = []
    for tail in ((0, 0), (0x7F, 127), (0xFF, -128), (0x7F, 0)):  # zeros, NaN codes, wild exponents
        g = torch.Generator().manual_seed(7)
        outs.append(kv.attn_run(64, "normal", lens, g, DEV, torch.bfloat16, dec.attention_decode_fp8, tail=tail)["out"])
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))


def test_ops_reject_wrong_caches():
    k8 = torch.zeros(2, 2, 8, 64, dtype=torch.uint8)
    ke = torch.zeros(2, 2, 8, dtype=torch.int8)
    qkv = torch.zeros(2, 3 * 2 * 64)
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        dec.attention_decode_fp8(qkv, k8.to(torch.int8), ke, k8.clone(), ke.clone(), lens, 2)
    with pytest.raises(ValueError):
        dec.attention_decode_fp8(qkv, k8, ke[:, :, :7], k8.clone(), ke.clone(), lens, 2)
    with pytest.raises(ValueError):
        dec.kv_store(torch.zeros(2, 9, 3 * 2 * 64), lens, k8, ke, k8.clone(), ke.clone())  # 9 positions, 8 rows


# ---- the model ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(model="gpt2", config_name="tiny", hidden_size=128, num_layers=2, num_heads=2,
                       vocab_size=300, seq_len=64, dropout=0.0, precision="fp32").eval()


def test_cached_logits_match_the_uncached_forward_over_dequantized_keys(model):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 300, (4, 30), generator=g)
    plens = [1, 5, 17, 24]
    cache = model.init_cache(4, 40, kv_dtype="fp8")
    kv.fill_pattern(cache)
    got = kv.teacher_forced_on(model, ids, plens, 24, cache)
    assert len(got) == sum(30 - p + 1 for p in plens)
    err = 0.0
    for b, p in enumerate(plens):
        want = kv.uncached_fp8_logits(model, ids[b], p)
        err = max(err, max((got[(b, j)] - want[j]).abs().max().item() for j in range(p - 1, 30)))
    assert err <= 1e-4, err
    # it is not the bf16-cache model: the format's error shows
    plain = kv.teacher_forced_on(model, ids, plens, 24, model.init_cache(4, 40))
    assert max((got[key] - plain[key]).abs().max().item() for key in got) > 1e-3
    # codes and exponents beyond prompt + steps keep the pattern; what was written does not (every row
    # ran the 29 steps of the shortest one, or until its cache was full)
    for b, p in enumerate(plens):
        n = min(p + 29, 40)
        assert (cache.buf[:, :, b, :, n:] == kv.PAT).all() and (cache.ebuf[:, :, b, :, n:] == kv.PAT).all()
        assert not (cache.ebuf[:, :, b, :, :n] == kv.PAT).any()
    assert cache.k[1].dtype == torch.uint8 and cache.ke[1].shape == (4, 2, 40) and cache.fp8


def test_greedy_generate_equals_the_uncached_loop_and_the_written_out_loop(model):
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 300, (3, 10), generator=g)
    plens = [3, 7, 10]
    lens = torch.tensor(plens)
    toks, new_lens, lp = model.generate(ids, lens, 8, temperature=0, kv_dtype="fp8", return_logprobs=True)
    again = model.generate(ids, lens, 8, temperature=0, kv_dtype="fp8")
    assert toks.shape == (3, 8) and new_lens.tolist() == [8, 8, 8] and torch.equal(again[0], toks)
    # the uncached loop over the yardstick's dequantized values, every choice by a clear margin
    margin = float("inf")
    for b, p in enumerate(plens):
        seq = ids[b, :p].clone()
        for _ in range(8):
            last = kv.uncached_fp8_logits(model, seq, p)[-1]
            top = last.topk(2).values
            margin = min(margin, float(top[0] - top[1]))
            seq = torch.cat([seq, last.argmax().view(1)])
        assert toks[b].tolist() == seq[p:].tolist()
    assert margin > 1e-3, margin  # far above the fp32 rounding between the two evaluation orders
    # the loop written out around decode_step, and the log-probabilities of its logits
    cache = model.init_cache(3, 18, kv_dtype="fp8")
    logits = model.prefill(ids, lens, cache)
    for t in range(8):
        tok = lms.greedy(logits)
        assert torch.equal(tok, toks[:, t])
        assert torch.equal(lp[:, t], token_stats(logits, tok)[0])
        if t < 7:
            logits = model.decode_step(tok, cache)


def test_generate_parks_rows_on_an_fp8_cache(model):
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 300, (3, 6), generator=g)
    lens = torch.tensor([6, 4, 6])
    free, _ = model.generate(ids, lens, 6, temperature=0, kv_dtype="fp8")
    eos = int(free[0, 2])
    first = free[0].tolist().index(eos)
    cache = model.init_cache(3, 12, kv_dtype="fp8")
    kv.fill_pattern(cache)
    toks, new_lens = model.generate(ids, lens, 6, temperature=0, eos_id=eos, cache=cache, check_every=2)
    assert toks[0].tolist() == free[0, :first + 1].tolist() + [eos] * (5 - first)
    assert new_lens[0] == first + 1 and cache.lens[0] == -1
    # the parked row ran `first` decode steps behind its 6 prompt rows: nothing behind those was touched
    n = 6 + first
    assert (cache.buf[:, :, 0, :, n:] == kv.PAT).all() and (cache.ebuf[:, :, 0, :, n:] == kv.PAT).all()
    assert not (cache.ebuf[:, :, 0, :, :n] == kv.PAT).any()
    # the keywords of generate work on it: penalties, counter-based noise
    a = model.generate(ids, lens, 6, temperature=0.8, top_k=20, noise_seed=5, repetition_penalty=1.3,
                       no_repeat_ngram=2, kv_dtype="fp8")
    b = model.generate(ids, lens, 6, temperature=0.8, top_k=20, noise_seed=5, repetition_penalty=1.3,
                       no_repeat_ngram=2, kv_dtype="fp8")
    assert torch.equal(a[0], b[0])
    with pytest.raises(ValueError):
        model.generate(ids, lens, 6, kv_dtype="fp4")
    with pytest.raises(ValueError, match="contradicts"):
        model.generate(ids, lens, 6, kv_dtype="fp8", cache=model.init_cache(3, 12))
    with pytest.raises(ValueError, match="contradicts"):
        model.generate(ids, lens, 6, kv_dtype="bf16", cache=model.init_cache(3, 12, kv_dtype="fp8"))
    with pytest.raises(ValueError):
        model.init_cache(3, 12, kv_dtype="int8")


def test_beam_search_and_lookahead_refuse_an_fp8_cache(model):
    ids = torch.randint(0, 300, (2, 6), generator=torch.Generator().manual_seed(4))
    lens = torch.tensor([6, 4])
    with pytest.raises(ValueError, match="fp8"):
        model.beam_search(ids, lens, 4, num_beams=2, cache=model.init_cache(4, 10, kv_dtype="fp8"))
    with pytest.raises(ValueError, match="fp8"):
        model.generate_lookahead(ids, lens, 4, lookahead=3, cache=model.init_cache(2, 10, kv_dtype="fp8"))
    with pytest.raises(ValueError, match="fp8"):
        model.decode_block(ids[:, :2], model.init_cache(2, 10, kv_dtype="fp8"))
    with pytest.raises(ValueError, match="fp8"):
        cache = model.init_cache(2, 10, kv_dtype="fp8")
        model.decode_step(ids[:, 0], cache, table=(torch.zeros(2, 10, dtype=torch.uint8), 1))


# ---- python -m run.generate --kv_dtype ---------------------------------------------------------------

def test_run_generate_kv_dtype(tmp_path):
    """A 2-step tiny GPT-2 training run on the CPU, then ``python -m run.generate`` with and without
    ``--kv_dtype``."""
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

    plain, _ = generate(tmp_path / "a.jsonl", "--temperature", "0", "--logprobs", "true")
    same, _ = generate(tmp_path / "b.jsonl", "--temperature", "0", "--logprobs", "true", "--kv_dtype", "bf16")
    assert (tmp_path / "a.jsonl").read_bytes() == (tmp_path / "b.jsonl").read_bytes()
    fp8, log = generate(tmp_path / "c.jsonl", "--temperature", "0", "--logprobs", "true", "--kv_dtype", "fp8")
    assert "model_000002.pt" in log and len(fp8) == len(plain) == 6
    for row, ref in zip(fp8, plain):
        assert set(row) == {"prompt", "continuation", "reference", "logprobs"} and row["prompt"] == ref["prompt"]
        assert len(row["continuation"]) == 6 and all(0 <= i < 200 for i in row["continuation"])
    # another model than the bf16-cache one: at the very least its log-probabilities differ
    assert [r_["logprobs"] for r_ in fp8] != [r_["logprobs"] for r_ in plain]
    # the round trip through --config_json
    cfg = json.load(open(ck / "training_args.json"))
    cfg["kv_dtype"] = "fp8"
    (tmp_path / "fp8.json").write_text(json.dumps(cfg))
    via_json, _ = generate(tmp_path / "d.jsonl", "--temperature", "0", "--logprobs", "true", cfg=tmp_path / "fp8.json")
    assert (tmp_path / "d.jsonl").read_bytes() == (tmp_path / "c.jsonl").read_bytes() and via_json == fp8
    # rejected before any checkpoint is read: nothing is loaded, so no "### loading" line
    for extra in (("--kv_dtype", "fp8", "--num_beams", "2"), ("--kv_dtype", "fp8", "--lookahead", "3", "--temperature", "0"),
                  ("--kv_dtype", "int8")):
        _, log = generate(tmp_path / "e.jsonl", *extra, ok=False)
        assert "kv_dtype" in log and "### loading" not in log
    cfg["kv_dtype"] = "fp4"
    (tmp_path / "fp4.json").write_text(json.dumps(cfg))
    _, log = generate(tmp_path / "f.jsonl", ok=False, cfg=tmp_path / "fp4.json")
    assert "kv_dtype" in log and "### loading" not in log
