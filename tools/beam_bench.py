"""Time what one beam-search step adds to a GPT-2 decode step, at GPT-2 small shapes (H = 12, D = 64,
V = 50257, W = 4 beams), all variants of a shape in one run:

* the decode attention through the cache indirection table (``ext.attn_decode_beam``) against the
  plain kernel (``ext.attn_decode``) on the same caches - with an identity table, where both read
  the same rows, and with a random table, where every key row comes from a random slot of its group;
* the table gather (the ``[B, W, Lmax]`` uint8 gather + scatter a step does once for all layers)
  and the copy it replaces: ``index_select`` of the live cache rows ``[2, B W, H, len, D]`` of one
  layer into a second buffer;
* ``ext.beam_step`` against ``log_softmax`` + add + ``topk`` over ``W V`` in stock ops.

    python tools/beam_bench.py [--rows 64,8] [--lens 128,512,1023] [--W 4] [--reps 7] [--spread_mb 768] [--out FILE]

As in tools/attn_decode_bench.py (whose ``interleaved`` this uses), consecutive calls of a variant
take different buffers, ``spread_mb`` of reads in all before one repeats, so nothing is served from
the last-level cache; every variant of a shape is timed in turn inside each repetition; medians and
min-max over the repetitions.  The derived figures per shape: the table variant relative to the plain
kernel, and per layer ``table variant + table gather / layers`` against ``plain kernel + cache copy``.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attn_decode_bench import interleaved  # noqa: E402

LAYERS = 12  # GPT-2 small: the table is built once per step and read by every layer


def attention(R, W, H, D, Lmax, n, reps, spread_bytes):
    from distributed_pipeline_amd.ops._ext import get_ext
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = 2 * n * D * 2 * R * H  # what the step reads from the caches
    nsets = max(2, -(-spread_bytes // nbytes))
    sets = [torch.empty(2, R, H, Lmax, D, device="cuda", dtype=torch.bfloat16).normal_(generator=g)
            for _ in range(nsets)]
    spare = torch.empty(2, R, H, n, D, device="cuda", dtype=torch.bfloat16)  # the second buffer of the copy
    qkv = torch.randn(R, 3 * H * D, device="cuda", generator=g).bfloat16()
    lens = torch.full((R,), n, dtype=torch.int32, device="cuda")
    ident = (torch.arange(R, device="cuda") % W).to(torch.uint8).view(R, 1).expand(R, Lmax).contiguous()
    rand = torch.randint(0, W, (R, Lmax), device="cuda", generator=g).to(torch.uint8)
    B = R // W
    parent = torch.randint(0, W, (B, W), device="cuda", generator=g)
    tables = [rand.view(B, W, Lmax).clone(), torch.empty(B, W, Lmax, dtype=torch.uint8, device="cuda")]
    rows = (torch.arange(B, device="cuda").view(B, 1) * W + parent).view(-1)
    at = torch.full((B, W, 1), n - 1, device="cuda")
    turn = {}

    def nxt(name):
        turn[name] = (turn.get(name, 0) + 1) % nsets
        return sets[turn[name]]

    def plain():
        c = nxt("plain")
        return ext.attn_decode(qkv, c[0], c[1], lens, H)

    def table(src, name):
        def run():
            c = nxt(name)
            return ext.attn_decode_beam(qkv, c[0], c[1], lens, H, src, W)
        return run

    def gather():  # the next table from this one: what beam_search does once per step
        torch.gather(tables[0], 1, parent.view(B, W, 1).expand(B, W, Lmax), out=tables[1])
        return tables[1].scatter_(2, at, parent.to(torch.uint8).view(B, W, 1))

    def copy():  # one layer's live K and V rows re-ordered into the second buffer
        c = nxt("copy")
        return torch.index_select(c[:, :, :, :n], 1, rows, out=spare)

    out = interleaved({"plain": (plain, 1000), "table_identity": (table(ident, "ti"), 1000),
                       "table_random": (table(rand, "tr"), 1000), "table_gather": (gather, 500),
                       "cache_copy": (copy, 200)}, reps)
    p = out["plain"]["median_ms"]
    for name in ("table_identity", "table_random"):
        out[name]["vs_plain"] = round(out[name]["median_ms"] / p, 3)
    out["plain"]["GBps"] = round(nbytes / p / 1e6, 1)
    with_table = out["table_random"]["median_ms"] + out["table_gather"]["median_ms"] / LAYERS
    with_copy = p + out["cache_copy"]["median_ms"]
    out["per_layer_ms"] = {"table_random_plus_gather": round(with_table, 5), "plain_plus_copy": round(with_copy, 5),
                           "ratio": round(with_table / with_copy, 3)}
    return {"op": "attention", "rows": R, "W": W, "H": H, "D": D, "Lmax": Lmax, "len": n, "kv_bytes": nbytes,
            "cache_sets": nsets, **out}


def step(R, W, V, reps, spread_bytes):
    from distributed_pipeline_amd.ops._ext import get_ext
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    B = R // W
    res = {"op": "beam_step", "rows": R, "W": W, "V": V}
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        nbytes = R * V * (2 if dtype == torch.bfloat16 else 4)
        nsets = max(2, -(-spread_bytes // nbytes))
        sets = [(2 * torch.randn(B, W, V, device="cuda", generator=g)).to(dtype) for _ in range(nsets)]
        scores = 1.5 * torch.randn(B, W, device="cuda", generator=g)
        fin = torch.zeros(B, W, dtype=torch.bool, device="cuda")
        turn = {}

        def nxt(name):
            turn[name] = (turn.get(name, 0) + 1) % nsets
            return sets[turn[name]]

        def kernel():
            return ext.beam_step(nxt("k"), scores, fin, -1, 0)

        def stock():
            lp = torch.log_softmax(nxt("s").float(), -1) + scores.unsqueeze(-1)
            top = torch.topk(lp.view(B, W * V), W, dim=-1)
            return top.values, top.indices // V, top.indices % V

        out = interleaved({"kernel": (kernel, 500), "stock": (stock, 100)}, reps)
        out["kernel"]["speedup_vs_stock"] = round(out["stock"]["median_ms"] / out["kernel"]["median_ms"], 2)
        res[tag] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,8", help="cache rows B * W")
    ap.add_argument("--lens", default="128,512,1023")
    ap.add_argument("--W", type=int, default=4)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--V", type=int, default=50257)
    ap.add_argument("--Lmax", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spread_mb", type=int, default=768, help="bytes read before a buffer is reused, MB")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__,
                         "layers_sharing_a_table": LAYERS})]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for R in (int(x) for x in a.rows.split(",")):
        for n in (int(x) for x in a.lens.split(",")):
            emit(attention(R, a.W, a.H, a.D, a.Lmax, n, a.reps, a.spread_mb << 20))
        emit(step(R, a.W, a.V, a.reps, a.spread_mb << 20))


if __name__ == "__main__":
    main()
