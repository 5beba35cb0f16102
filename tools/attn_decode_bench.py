"""Time the attention of one GPT-2 decode step: the fused kernel (csrc/attn_decode.hip through
``ext.attn_decode``) against the PyTorch path of ``ops.decode.attention_decode`` on the same
tensors, and against a device copy of as many bytes as the step has to read from the K/V caches
(2 * len * D * 2 bytes per (row, head)) - the bandwidth yardstick, measured in the same run.  Beside
it, in the same interleaved run and at the same shapes, the step over the one-byte cache
(csrc/attn_decode_fp8.hip through ``ext.attn_decode_fp8``) with yardsticks of its own: the bf16 kernel,
and a device copy of the bytes the fp8 step reads (2 * len * (D + 1) per (row, head): codes and one
exponent per row).

    python tools/attn_decode_bench.py [--B 64,8] [--lens 128,512,1023] [--H 12] [--D 64] [--reps 7] [--spread_mb 768]
                                        [--out FILE] [--extend [--extend_shapes 0:128,512:32,896:128]] [--grouped]

``--extend`` times the cache-extending kernel (csrc/attn_extend.hip) instead: see ``extend_shape``.
``--grouped`` times the grouped decode kernel (csrc/attn_decode_grouped.hip) instead: see ``grouped_shape``.

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


def extend_shape(B, H, D, Lmax, n, T, reps, spread_bytes):
    """K-M27 (csrc/attn_extend.hip): T new tokens per row against ``n`` cached ones, beside three
    yardsticks in the same interleaved run - ``ops.nn.attention`` on the equivalent full causal sequence
    of n + T tokens (padded to a multiple of 64: what a prefill from scratch runs), ceil(T / 8) calls of
    the block kernel (what the tree could append with before), and a device copy of the K/V bytes the
    call has to read: the n cached rows and the T new ones, K and V, once per (row, head)."""
    from distributed_pipeline_amd.ops import nn as ops
    from distributed_pipeline_amd.ops._ext import get_ext
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = 2 * (n + T) * D * 2 * B * H
    nsets = max(2, -(-spread_bytes // nbytes))
    sets = [torch.empty(2, B, H, Lmax, D, device="cuda", dtype=torch.bfloat16).normal_(generator=g)
            for _ in range(nsets)]
    qkv = torch.randn(B, T, 3 * H * D, device="cuda", generator=g).bfloat16()
    L = -(-(n + T) // 64) * 64
    full = [torch.randn(B, L, 3 * H * D, device="cuda", generator=g).bfloat16() for _ in range(min(nsets, 8))]
    lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
    blens = [torch.full((B,), n + j, dtype=torch.int32, device="cuda") for j in range(0, T, 8)]
    src = [torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_() for _ in range(nsets)]
    dst = [torch.empty_like(t) for t in src]
    turn = {"extend": 0, "attention": 0, "block": 0, "copy": 0}

    def nxt(name, count=nsets):
        turn[name] = (turn[name] + 1) % count
        return turn[name]

    def extend():
        c = sets[nxt("extend")]
        return ext.attn_extend(qkv, c[0], c[1], lens, H)

    def attention():
        return ops.attention(full[nxt("attention", len(full))], H, 0.0, True, False)

    def block():
        c = sets[nxt("block")]
        for i, j in enumerate(range(0, T, 8)):
            ext.attn_decode_block(qkv[:, j:j + 8], c[0], c[1], blens[i], H)

    def copy():
        i = nxt("copy")
        return dst[i].copy_(src[i])

    assert extend() is not None, "the extend kernel must take this shape"
    out = interleaved({"extend": (extend, 200), "attention": (attention, 200), "block": (block, 50),
                       "copy": (copy, 200)}, reps)
    for name in ("attention", "block", "copy"):
        out["extend"]["time_vs_" + name] = round(out["extend"]["median_ms"] / out[name]["median_ms"], 3)
    # 4 (n + (T + 1) / 2) T D multiply-adds' worth of flops per (row, head): Q K^T and P V under the causal edge
    out["extend"]["TFLOPs"] = round(4 * (n + (T + 1) / 2) * T * D * B * H / out["extend"]["median_ms"] / 1e9, 2)
    return {"kernel": "attn_extend", "B": B, "H": H, "D": D, "Lmax": Lmax, "len": n, "T": T, "kv_bytes": nbytes,
            "cache_sets": nsets, **out}


def grouped_shape(R, G, H, D, prefix, suffix, reps, spread_bytes):
    """K-M28 (csrc/attn_decode_grouped.hip): R = B G rows, ``prefix`` shared keys per group and ``suffix`` own keys per
    row, beside two yardsticks in the same interleaved run - K-M18 (csrc/attn_decode.hip) on R rows that each hold
    a full copy of prefix + suffix (what G samples of a prompt cost without the kernel), and a device copy of the
    K/V bytes K-M28 has to read: the prefix once per group, the suffix once per row."""
    from distributed_pipeline_amd.ops._ext import get_ext
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    B = R // G
    nbytes = 2 * D * 2 * H * (B * prefix + R * suffix)   # K-M28's reads
    nbytes_rows = 2 * D * 2 * H * R * (prefix + suffix)  # K-M18's
    nsets, nsets_rows = max(2, -(-spread_bytes // nbytes)), max(2, -(-spread_bytes // nbytes_rows))
    new = lambda *shape: torch.empty(*shape, device="cuda", dtype=torch.bfloat16).normal_(generator=g)  # noqa: E731
    pre, suf = [new(2, B, H, prefix, D) for _ in range(nsets)], [new(2, R, H, suffix + 1, D) for _ in range(nsets)]
    full = [new(2, R, H, prefix + suffix + 1, D) for _ in range(nsets_rows)]
    qkv = torch.randn(R, 3 * H * D, device="cuda", generator=g).bfloat16()
    plens = torch.full((B,), prefix, dtype=torch.int32, device="cuda")
    slens = torch.full((R,), suffix, dtype=torch.int32, device="cuda")
    lens = torch.full((R,), prefix + suffix, dtype=torch.int32, device="cuda")
    src = [torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_() for _ in range(nsets)]
    dst = [torch.empty_like(t) for t in src]
    turn = {"grouped": 0, "rows": 0, "copy": 0}

    def nxt(name, count):
        turn[name] = (turn[name] + 1) % count
        return turn[name]

    def grouped():
        i = nxt("grouped", nsets)
        return ext.attn_decode_grouped(qkv, pre[i][0], pre[i][1], plens, suf[i][0], suf[i][1], slens, H, G)

    def rows():
        c = full[nxt("rows", nsets_rows)]
        return ext.attn_decode(qkv, c[0], c[1], lens, H)

    def copy():
        i = nxt("copy", nsets)
        return dst[i].copy_(src[i])

    assert grouped() is not None, "the grouped kernel must take this shape"
    out = interleaved({"grouped": (grouped, 300), "rows": (rows, 300), "copy": (copy, 300)}, reps)
    out["grouped"]["time_vs_rows"] = round(out["grouped"]["median_ms"] / out["rows"]["median_ms"], 3)
    out["grouped"]["time_vs_copy"] = round(out["grouped"]["median_ms"] / out["copy"]["median_ms"], 3)
    qs = ext.attn_decode_grouped_qs(B * H, G, torch.cuda.get_device_properties(0).multi_processor_count)
    return {"kernel": "attn_decode_grouped", "R": R, "G": G, "H": H, "D": D, "prefix": prefix, "suffix": suffix,
            "qs": qs, "kv_bytes": nbytes, "kv_bytes_rows": nbytes_rows, "cache_sets": nsets, **out}


def grouped_model_step(R, G, prefix, suffix, reps):
    """One whole ``decode_step(decode_linears="rows")`` of GPT-2 small per cache kind: R rows over a plain cache
    that holds prefix + suffix keys each, and over a ``GroupKVCache`` of R / G prompts."""
    from distributed_pipeline_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(model="gpt2", config_name="gpt2", precision="bf16", seq_len=1024, dropout=0.0).cuda().eval()
    for p in model.parameters():
        p._dpa_shadow = p.detach().to(torch.bfloat16)
    tok = torch.randint(0, model.cfg["vocab_size"], (R,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    plain, group = model.init_cache(R, 1024), model.init_group_cache(R // G, G, prefix, 1024 - prefix)
    for buf in (plain.buf, group.prefix.buf, group.suffix.buf):
        buf.normal_()

    def step_plain():
        plain.lens.fill_(prefix + suffix)  # the same position every call
        return model.decode_step(tok, plain, decode_linears="rows")

    def step_group():
        group.prefix.lens.fill_(prefix)
        group.suffix.lens.fill_(suffix)
        return model.decode_step(tok, group, decode_linears="rows")

    out = interleaved({"plain_cache": (step_plain, 20), "group_cache": (step_group, 20)}, reps, warmup=2)
    out["group_cache"]["time_vs_plain"] = round(out["group_cache"]["median_ms"] / out["plain_cache"]["median_ms"], 3)
    return {"model": "gpt2", "decode_linears": "rows", "R": R, "G": G, "prefix": prefix, "suffix": suffix, **out}


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
    ap.add_argument("--extend", action="store_true",
                    help="the rows of the cache-extending kernel instead: B in 1,8,64 x (len, T) in --extend_shapes")
    ap.add_argument("--extend_shapes", default="0:128,512:32,896:128")
    ap.add_argument("--grouped", action="store_true",
                    help="the cells of the grouped decode kernel instead: B*G in --B x G in 2..32 x prefix x suffix")
    ap.add_argument("--prefixes", default="128,512,896")
    ap.add_argument("--suffixes", default="1,64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    if a.extend:
        for B in (1, 8, 64):
            for n, T in (tuple(int(x) for x in sh.split(":")) for sh in a.extend_shapes.split(",")):
                lines.append(json.dumps(extend_shape(B, a.H, a.D, a.Lmax, n, T, a.reps, a.spread_mb << 20)))
                print(lines[-1], flush=True)
        a.B, a.no_model = "", True
    if a.grouped:
        for R in (int(x) for x in a.B.split(",")):
            for G in (g for g in (2, 4, 8, 16, 32) if g <= R):
                for pfx in (int(x) for x in a.prefixes.split(",")):
                    for sfx in (int(x) for x in a.suffixes.split(",")):
                        lines.append(json.dumps(grouped_shape(R, G, a.H, a.D, pfx, sfx, a.reps, a.spread_mb << 20)))
                        print(lines[-1], flush=True)
        if not a.no_model:
            lines.append(json.dumps(grouped_model_step(64, 8, 512, 16, a.reps)))
            print(lines[-1], flush=True)
        a.B, a.no_model = "", True
    for B in (int(x) for x in a.B.split(",") if x):
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
