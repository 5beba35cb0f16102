"""Time the attention of one GPT-2 decode step: the fused kernel (csrc/attn_decode.hip through
``ext.attn_decode``) against the PyTorch path of ``ops.decode.attention_decode`` on the same
tensors, and against a device copy of as many bytes as the step has to read from the K/V caches
(2 * len * D * 2 bytes per (row, head)) - the bandwidth yardstick, measured in the same run.  Beside
it, in the same interleaved run and at the same shapes, the step over the one-byte cache
(csrc/attn_decode_fp8.hip through ``ext.attn_decode_fp8``) with yardsticks of its own: the bf16 kernel,
and a device copy of the bytes the fp8 step reads (2 * len * (D + 1) per (row, head): codes and one
exponent per row).

    python tools/attn_decode_bench.py [--B 64,8] [--lens 128,512,1023] [--H 12] [--D 64] [--reps 7] [--spread_mb 768]
                                        [--out FILE]

Consecutive calls of a variant take different caches (and the copy different buffers), so that
``spread_mb`` of reads pass before one repeats and nothing is served from the last-level cache.

It also times one whole ``GPT2LMModel.decode_step`` against what a user without the cache runs for
the same token: the full causal forward over all ``len`` positions (its hidden states, and the
head on the last position only), both at GPT-2 small, B = 64, len = 512 (``--no_model`` skips it).

Every variant of a shape is timed in turn inside each repetition (interleaved); a repetition is
``inner`` back-to-back calls between two device events; medians and min-max over the repetitions.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def interleaved(variants, reps, warmup=3):
    for fn, _ in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, (fn, inner) in variants.items():
            times[k].append(timed(fn, inner))
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                "max_ms": round(max(v), 5)} for k, v in times.items()}


def shape(B, H, D, Lmax, n, reps, spread_bytes):
    from distributed_pipeline_amd.ops._ext import get_ext
    from distributed_pipeline_amd.ops.decode import attention_decode_ref
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = 2 * n * D * 2 * B * H  # what the step reads from the caches
    # consecutive calls take different caches (and the copy different buffers), spread_bytes of
    # reads in all before one repeats: more than the chip's last-level cache holds, as in a real
    # step, where every layer has its own cache
    nsets = max(1, -(-spread_bytes // nbytes))
    sets = [torch.empty(2, B, H, Lmax, D, device="cuda", dtype=torch.bfloat16).normal_(generator=g)
            for _ in range(nsets)]  # k, v = views of one buffer, as in KVCache
    qkv = torch.randn(B, 3 * H * D, device="cuda", generator=g).bfloat16()
    lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
    src = [torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_() for _ in range(nsets)]
    dst = [torch.empty_like(t) for t in src]
    # the one-byte cache: finite codes of either sign (0x7f / 0xff are NaN), exponents around 2^-8
    nbytes8 = 2 * n * (D + 1) * B * H
    nsets8 = max(1, -(-spread_bytes // nbytes8))
    codes = [torch.empty(2, B, H, Lmax, D, device="cuda", dtype=torch.uint8).random_(0, 0x7F, generator=g)
             + 128 * torch.empty(2, B, H, Lmax, D, device="cuda", dtype=torch.uint8).random_(0, 2, generator=g)
             for _ in range(nsets8)]
    exps = [torch.empty(2, B, H, Lmax, device="cuda", dtype=torch.int8).random_(-10, -6, generator=g)
            for _ in range(nsets8)]
    src8 = [torch.empty(nbytes8, dtype=torch.uint8, device="cuda").random_() for _ in range(nsets8)]
    dst8 = [torch.empty_like(t) for t in src8]
    turn = {"kernel": 0, "torch": 0, "copy": 0, "kernel_fp8": 0, "copy_fp8": 0}
    count = {"kernel_fp8": nsets8, "copy_fp8": nsets8}

    def nxt(name):
        turn[name] = (turn[name] + 1) % count.get(name, nsets)
        return turn[name]

    def kernel():
        c = sets[nxt("kernel")]
        return ext.attn_decode(qkv, c[0], c[1], lens, H)

    def torch_path():
        c = sets[nxt("torch")]
        return attention_decode_ref(qkv, c[0], c[1], lens, H)

    def copy():
        i = nxt("copy")
        return dst[i].copy_(src[i])

    def kernel_fp8():
        i = nxt("kernel_fp8")
        return ext.attn_decode_fp8(qkv, codes[i][0], exps[i][0], codes[i][1], exps[i][1], lens, H)

    def copy_fp8():
        i = nxt("copy_fp8")
        return dst8[i].copy_(src8[i])

    assert kernel_fp8() is not None, "the fp8 kernel must take this shape"
    out = interleaved({"kernel": (kernel, 2000), "kernel_fp8": (kernel_fp8, 2000), "torch": (torch_path, 50),
                       "copy": (copy, 2000), "copy_fp8": (copy_fp8, 2000)}, reps)
    for name in ("kernel", "torch", "copy"):
        out[name]["GBps"] = round(nbytes / out[name]["median_ms"] / 1e6, 1)
    for name in ("kernel_fp8", "copy_fp8"):
        out[name]["GBps"] = round(nbytes8 / out[name]["median_ms"] / 1e6, 1)
    out["kernel_fp8"]["fraction_of_copy_rate"] = round(out["copy_fp8"]["median_ms"] / out["kernel_fp8"]["median_ms"], 3)
    out["kernel_fp8"]["speedup_vs_bf16_kernel"] = round(out["kernel"]["median_ms"] / out["kernel_fp8"]["median_ms"], 3)
    # the copy's rate counts each byte once, though it reads and writes it
    out["kernel"]["fraction_of_copy_rate"] = round(out["copy"]["median_ms"] / out["kernel"]["median_ms"], 3)
    out["kernel"]["speedup_vs_torch"] = round(out["torch"]["median_ms"] / out["kernel"]["median_ms"], 2)
    return {"B": B, "H": H, "D": D, "Lmax": Lmax, "len": n, "kv_bytes": nbytes, "cache_sets": nsets,
            "kv_bytes_fp8": nbytes8, "cache_sets_fp8": nsets8, **out}


def model_step(B, n, reps):
    from distributed_pipeline_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(model="gpt2", config_name="gpt2", precision="bf16", seq_len=1024, dropout=0.0).cuda().eval()
    for p in model.parameters():
        p._dpa_shadow = p.detach().to(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(0, model.cfg["vocab_size"], (B, n), device="cuda", generator=g)
    cache = model.init_cache(B, 1024)
    with torch.no_grad():
        model.prefill(ids[:, :n - 1], torch.full((B,), n - 1, dtype=torch.int32, device="cuda"), cache)

    def step():
        cache.lens.fill_(n - 1)  # the same position every call
        return model.decode_step(ids[:, n - 1], cache)

    def uncached():
        with torch.no_grad():
            h = model.hidden_states(ids)
            return torch.nn.functional.linear(h[:, -1], model.wte.weight._dpa_shadow)

    out = interleaved({"decode_step": (step, 20), "uncached_forward": (uncached, 5)}, reps, warmup=2)
    out["decode_step"]["speedup_vs_uncached"] = round(
        out["uncached_forward"]["median_ms"] / out["decode_step"]["median_ms"], 1)
    return {"model": "gpt2", "B": B, "len": n, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="64,8")
    ap.add_argument("--lens", default="128,512,1023")
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--Lmax", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spread_mb", type=int, default=768, help="bytes read before a cache is reused, MB")
    ap.add_argument("--no_model", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for B in (int(x) for x in a.B.split(",")):
        for n in (int(x) for x in a.lens.split(",")):
            lines.append(json.dumps(shape(B, a.H, a.D, a.Lmax, n, a.reps, a.spread_mb << 20)))
            print(lines[-1], flush=True)
    if not a.no_model:
        lines.append(json.dumps(model_step(64, 512, a.reps)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
