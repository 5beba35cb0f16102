"""Time the Linears of one GPT-2 decode step: the row kernel (csrc/linear_rows.hip through
``ext.linear_rows``) against today's ``ops.nn.linear`` on the same tensors (the rows padded into the
training GEMM's tiles; hipBLASLt for the head) and against a device copy of the weight's bytes - the
bandwidth yardstick - all in one process and interleaved.  Beside them the same Linear on one-byte weights
(csrc/linear_rows_fp8.hip through ``ext.linear_rows_fp8``, the weights quantized with ``kv_quantize_ref``) and a
device copy of the fp8 weight's bytes, on weight copies of their own spread over the same number of bytes.

    python tools/decode_linear_bench.py [--M 1,8,64,128] [--reps 7] [--spread_mb 768] [--no_linears] [--no_model]
                                        [--out FILE]

Shapes: GPT-2 small's five Linears, (N, K) = qkv (2304, 768), attn_proj (768, 768), mlp_fc (3072, 768, GELU),
mlp_proj (768, 3072) and the tied head (50257, 768, no bias).  Consecutive calls of a variant take
different copies of the weight, so that ``spread_mb`` of reads pass before one repeats and nothing is
served from the last-level cache.

The fused sublayers (csrc/linear_rows_fused.hip, ``ext.linear_rows`` with ``ln_*`` / ``residual``) are timed as the
two chains of a block, "rows" against "rows_fused" on the same rotating weights: ``ln_qkv`` (rows: the
``residual_layernorm`` launch and the qkv launch; fused: one launch) and ``proj_ln_fc`` (rows: attn_proj,
``residual_layernorm``, mlp_fc; fused: attn_proj + residual, LN + mlp_fc).  ``--no_linears`` skips the single Linears.

It also times one whole ``GPT2LMModel.decode_step`` at (B, len) = (64, 512) and (8, 512) with
``decode_linears="tile"``, ``"rows"``, ``"rows_fp8"`` and ``"rows_fused"``, interleaved in the same run (``--no_model``
skips it).

Every variant of a shape is timed in turn inside each repetition; a repetition is ``inner`` back-to-back
calls between two device events; medians and min-max over the repetitions.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.attn_decode_bench import interleaved  # noqa: E402

LINEARS = [("qkv", 2304, 768, "none", True), ("attn_proj", 768, 768, "none", True), ("mlp_fc", 3072, 768, "gelu", True),
           ("mlp_proj", 768, 3072, "none", True), ("head", 50257, 768, "none", False)]
ACT_CODES = {"none": 0, "gelu": 1}


def shape(name, N, K, act, has_bias, M, reps, spread_bytes):
    from distributed_pipeline_amd.ops import nn
    from distributed_pipeline_amd.ops._ext import get_ext
    from distributed_pipeline_amd.ops.decode import kv_quantize_ref
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = N * K * 2
    nsets = max(1, -(-spread_bytes // nbytes))
    ws = [torch.empty(N, K, device="cuda", dtype=torch.bfloat16).normal_(0.0, K ** -0.5, generator=g)
          for _ in range(nsets)]
    dst = [torch.empty_like(ws[0]) for _ in range(min(nsets, 8))]
    # the one-byte weights: twice as many copies, so that as many bytes pass before one repeats
    nsets8 = 2 * nsets
    q = [kv_quantize_ref(w) for w in ws]
    w8 = [q[i % nsets][0].clone() for i in range(nsets8)]
    e8 = [q[i % nsets][1] for i in range(nsets8)]
    del q
    dst8 = [torch.empty_like(w8[0]) for _ in range(min(nsets8, 8))]
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    b = torch.randn(N, device="cuda", generator=g).bfloat16() if has_bias else None
    turn = {"rows": 0, "tile": 0, "copy": 0, "rows_fp8": 0, "copy_fp8": 0}

    def nxt(key, n=nsets):
        turn[key] = (turn[key] + 1) % n
        return turn[key]

    def rows_fp8():
        i = nxt("rows_fp8", nsets8)
        return ext.linear_rows_fp8(x, w8[i], e8[i], b, ACT_CODES[act])

    def copy_fp8():
        i = nxt("copy_fp8", nsets8)
        return dst8[i % len(dst8)].copy_(w8[i])

    def rows():
        return ext.linear_rows(x, ws[nxt("rows")], b, ACT_CODES[act])

    def tile():
        with torch.no_grad():
            return nn.linear(x, ws[nxt("tile")], b, act)

    def copy():
        i = nxt("copy")
        return dst[i % len(dst)].copy_(ws[i])

    assert rows() is not None and rows_fp8() is not None, "the row kernels must take this shape"
    out = interleaved({"rows": (rows, 500), "rows_fp8": (rows_fp8, 500), "tile": (tile, 200), "copy": (copy, 500),
                       "copy_fp8": (copy_fp8, 500)}, reps)
    for key in out:
        out[key]["GBps"] = round((nbytes // 2 if key.endswith("fp8") else nbytes) / out[key]["median_ms"] / 1e6, 1)
    out["rows_fp8"]["fraction_of_fp8_copy_rate"] = round(out["copy_fp8"]["median_ms"] / out["rows_fp8"]["median_ms"], 3)
    out["rows_fp8"]["speedup_vs_rows"] = round(out["rows"]["median_ms"] / out["rows_fp8"]["median_ms"], 2)
    out["rows_fp8"]["ranges_apart_from_rows"] = bool(out["rows_fp8"]["max_ms"] < out["rows"]["min_ms"])
    # the copy's rate counts each byte once, though it reads and writes it
    out["rows"]["fraction_of_copy_rate"] = round(out["copy"]["median_ms"] / out["rows"]["median_ms"], 3)
    out["rows"]["speedup_vs_tile"] = round(out["tile"]["median_ms"] / out["rows"]["median_ms"], 2)
    return {"linear": name, "M": M, "N": N, "K": K, "act": act, "weight_bytes": nbytes, "weight_copies": nsets, **out}


def sublayers(M, reps, spread_bytes, H=768):
    """The two chains of a GPT-2 small block at M rows, "rows" against "rows_fused", interleaved."""
    from distributed_pipeline_amd.ops import nn
    from distributed_pipeline_amd.ops._ext import get_ext
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *sh: torch.randn(*sh, device="cuda", generator=g).bfloat16()  # noqa: E731
    sets = lambda N, K: [torch.empty(N, K, device="cuda", dtype=torch.bfloat16).normal_(0.0, K ** -0.5, generator=g)  # noqa: E731
                         for _ in range(max(1, -(-spread_bytes // (N * K * 2))))]
    wq, wp, wf = sets(3 * H, H), sets(H, H), sets(4 * H, H)
    bq, bp, bf = rnd(3 * H), rnd(H), rnd(4 * H)
    x, h, gm, bt = rnd(M, H), rnd(M, H), rnd(H), rnd(H)
    turn = {}

    def nxt(key, ws):
        turn[key] = (turn.get(key, -1) + 1) % len(ws)
        return ws[turn[key]]

    def ln_qkv_rows():
        _, a = nn.residual_layernorm(h.view(1, M, H), x.view(1, M, H), gm, bt, 0.0, 1e-5, False)
        return ext.linear_rows(a.view(M, H), nxt("q0", wq), bq, 0)

    def ln_qkv_fused():
        return ext.linear_rows(x, nxt("q1", wq), bq, 0, ln_gamma=gm, ln_beta=bt, ln_eps=1e-5)

    def proj_ln_fc_rows():
        y = ext.linear_rows(h, nxt("p0", wp), bp, 0)
        _, a = nn.residual_layernorm(y.view(1, M, H), x.view(1, M, H), gm, bt, 0.0, 1e-5, False)
        return ext.linear_rows(a.view(M, H), nxt("f0", wf), bf, 1)

    def proj_ln_fc_fused():
        x2 = ext.linear_rows(h, nxt("p1", wp), bp, 0, residual=x)
        return ext.linear_rows(x2, nxt("f1", wf), bf, 1, ln_gamma=gm, ln_beta=bt, ln_eps=1e-5)

    with torch.no_grad():
        assert ln_qkv_fused() is not None and proj_ln_fc_fused() is not None, "the fused kernel must take this shape"
        out = interleaved({"ln_qkv_rows": (ln_qkv_rows, 300), "ln_qkv_fused": (ln_qkv_fused, 300),
                           "proj_ln_fc_rows": (proj_ln_fc_rows, 200), "proj_ln_fc_fused": (proj_ln_fc_fused, 200)}, reps)
    for chain in ("ln_qkv", "proj_ln_fc"):
        r, f = out[chain + "_rows"], out[chain + "_fused"]
        f["speedup_vs_rows"] = round(r["median_ms"] / f["median_ms"], 2)
        f["ranges_overlap_rows"] = bool(f["max_ms"] >= r["min_ms"] and r["max_ms"] >= f["min_ms"])
    return {"sublayers": "gpt2", "M": M, **out}


def model_steps(shapes, reps):
    from distributed_pipeline_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(model="gpt2", config_name="gpt2", precision="bf16", seq_len=1024, dropout=0.0).cuda().eval()
    for p in model.parameters():
        p._dpa_shadow = p.detach().to(torch.bfloat16)
    res = []
    for B, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        ids = torch.randint(0, model.cfg["vocab_size"], (B, n), device="cuda", generator=g)
        cache = model.init_cache(B, 1024)
        with torch.no_grad():
            model.prefill(ids[:, :n - 1], torch.full((B,), n - 1, dtype=torch.int32, device="cuda"), cache)

        def step(mode):
            cache.lens.fill_(n - 1)  # the same position every call
            return model.decode_step(ids[:, n - 1], cache, decode_linears=mode)

        # one row alone against the same row inside the batch: an observation, not a promise
        one = model.init_cache(1, 1024)
        with torch.no_grad():
            model.prefill(ids[:1, :n - 1], torch.full((1,), n - 1, dtype=torch.int32, device="cuda"), one)
        alone = model.decode_step(ids[:1, n - 1], one, decode_linears="rows")
        same = bool(torch.equal(alone.view(torch.int16), step("rows")[:1].view(torch.int16)))
        out = interleaved({"tile": (lambda: step("tile"), 20), "rows": (lambda: step("rows"), 20),
                           "rows_fp8": (lambda: step("rows_fp8"), 20),
                           "rows_fused": (lambda: step("rows_fused"), 20)}, reps, warmup=2)
        out["rows"]["speedup_vs_tile"] = round(out["tile"]["median_ms"] / out["rows"]["median_ms"], 2)
        out["rows_fp8"]["speedup_vs_rows"] = round(out["rows"]["median_ms"] / out["rows_fp8"]["median_ms"], 2)
        r, f = out["rows"], out["rows_fused"]
        f["speedup_vs_rows"] = round(r["median_ms"] / f["median_ms"], 2)
        f["ranges_overlap_rows"] = bool(f["max_ms"] >= r["min_ms"] and r["max_ms"] >= f["min_ms"])
        res.append({"model": "gpt2", "B": B, "len": n, "row_0_alone_bit_equal_rows_mode": same, **out})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", default="1,8,64,128")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spread_mb", type=int, default=768, help="weight bytes read before a copy is reused, MB")
    ap.add_argument("--no_linears", action="store_true", help="skip the single Linears (the fused chains still run)")
    ap.add_argument("--no_model", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for M in (int(v) for v in a.M.split(",")):
        lines.append(json.dumps(sublayers(M, a.reps, a.spread_mb << 20)))
        print(lines[-1], flush=True)
    for name, N, K, act, has_bias in ([] if a.no_linears else LINEARS):
        for M in (int(v) for v in a.M.split(",")):
            lines.append(json.dumps(shape(name, N, K, act, has_bias, M, a.reps, a.spread_mb << 20)))
            print(lines[-1], flush=True)
    if not a.no_model:
        for r in model_steps([(64, 512), (8, 512)], a.reps):
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
