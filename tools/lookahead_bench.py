"""Time what lookahead decoding stands on: the block decode attention (csrc/attn_decode_block.hip
through ``ext.attn_decode_block``) against the T sequential calls of the plain kernel it equals, and
one ``GPT2LMModel.decode_block`` of the whole model against one ``decode_step``.

    python tools/lookahead_bench.py [--B 64,8] [--lens 128,512,1023] [--T 2,4,8] [--H 12] [--D 64] [--reps 7]
                                    [--spread_mb 768] [--no_model] [--out FILE]

Per (B, len, T), on the same caches and projections: ``block`` - one block call whose last query
attends over ``len`` cached keys and its own (``lens = len - T + 1``); ``sequential`` - the T plain
calls that define it (``lens = len - T + 1 .. len``); ``plain`` - one plain call at ``len``.  The
yardstick for the kernel is ``sequential`` in the same run; no time is fixed in advance.

The method is tools/attn_decode_bench.py's (whose ``interleaved`` this uses): every variant of a
shape is timed in turn inside each repetition; a repetition is ``inner`` back-to-back calls between
two device events; medians and min-max over the repetitions; consecutive calls of a variant take
different caches, so that ``spread_mb`` of reads pass before one repeats.

The model part is GPT-2 small at len 512, B = 64 and B = 8: one ``decode_block`` of T tokens per row
(the last one at position 511) against one ``decode_step`` at position 511.  ``break_even_accept`` is
the mean number of accepted guesses per call from which lookahead decoding is the faster loop:
``t_block / t_step - 1`` (a call emits 1 + accepted tokens), without the draft and bookkeeping ops of
``generate_lookahead``, which are not timed here.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attn_decode_bench import interleaved  # noqa: E402


def shape(B, H, D, Lmax, n, Ts, reps, spread_bytes):
    from distributed_pipeline_amd.ops._ext import get_ext
    ext = get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = 2 * n * D * 2 * B * H  # what one pass reads from the caches
    nsets = max(1, -(-spread_bytes // nbytes))
    sets = [torch.empty(2, B, H, Lmax, D, device="cuda", dtype=torch.bfloat16).normal_(generator=g)
            for _ in range(nsets)]  # k, v = views of one buffer, as in KVCache
    turn = {}

    def nxt(name):
        turn[name] = (turn.get(name, 0) + 1) % nsets
        return sets[turn[name]]

    out = {"B": B, "H": H, "D": D, "Lmax": Lmax, "len": n, "kv_bytes": nbytes, "cache_sets": nsets}
    for T in Ts:
        qkv = torch.randn(B, T, 3 * H * D, device="cuda", generator=g).bfloat16()
        first = n - T + 1
        assert first >= 0 and n < Lmax
        lens = [torch.full((B,), first + j, dtype=torch.int32, device="cuda") for j in range(T)]
        rows = [qkv[:, j] for j in range(T)]

        def block():
            c = nxt("block")
            return ext.attn_decode_block(qkv, c[0], c[1], lens[0], H)

        def sequential():
            c = nxt("sequential")
            for j in range(T):
                o = ext.attn_decode(rows[j], c[0], c[1], lens[j], H)
            return o

        def plain():
            c = nxt("plain")
            return ext.attn_decode(rows[T - 1], c[0], c[1], lens[T - 1], H)

        assert block() is not None and sequential() is not None
        r = interleaved({"block": (block, 1000), "sequential": (sequential, 250), "plain": (plain, 1000)}, reps)
        r["block"]["speedup_vs_sequential"] = round(r["sequential"]["median_ms"] / r["block"]["median_ms"], 2)
        r["block"]["plain_calls_worth"] = round(r["block"]["median_ms"] / r["plain"]["median_ms"], 2)
        out[f"T={T}"] = r
    return out


def model_calls(B, n, Ts, reps):
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

    variants = {"decode_step": (step, 20)}
    for T in Ts:
        def block(T=T):
            cache.lens.fill_(n - T)  # the block's last token at position n - 1
            return model.decode_block(ids[:, n - T:], cache)
        variants[f"decode_block_T{T}"] = (block, 20)
    out = interleaved(variants, reps, warmup=2)
    for T in Ts:
        ratio = out[f"decode_block_T{T}"]["median_ms"] / out["decode_step"]["median_ms"]
        out[f"decode_block_T{T}"]["steps_worth"] = round(ratio, 3)
        out[f"decode_block_T{T}"]["break_even_accept"] = round(ratio - 1, 3)
    return {"model": "gpt2", "B": B, "len": n, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="64,8")
    ap.add_argument("--lens", default="128,512,1023")
    ap.add_argument("--T", default="2,4,8")
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--Lmax", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spread_mb", type=int, default=768, help="bytes read before a cache is reused, MB")
    ap.add_argument("--no_model", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    Ts = [int(x) for x in a.T.split(",")]
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for B in (int(x) for x in a.B.split(",")):
        for n in (int(x) for x in a.lens.split(",")):
            lines.append(json.dumps(shape(B, a.H, a.D, a.Lmax, n, Ts, a.reps, a.spread_mb << 20)))
            print(lines[-1], flush=True)
    if not a.no_model:
        for B in (64, 8):
            lines.append(json.dumps(model_calls(B, 512, Ts, a.reps)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
