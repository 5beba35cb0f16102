"""Time one DiffuSeq reverse-step update outside the model: the fused kernel
(csrc/reverse_step.hip through ``ops.diffusion.reverse_step``) against the PyTorch chain that
``GaussianDiffusion.p_sample`` (+ the gather of ``round_to_embeds``) runs.

    python tools/reverse_step_bench.py [--N 262144,8192] [--E 128] [--V 30522] [--reps 7] [--out FILE]

Both sides start from the same bf16 model output (and, on the rounded steps, the same token ids:
the arg-max of the rounding is common to both and left out) and end with the fp32 x_{t-1} and
its bf16 copy, the next forward's input.  The chain is the real ``p_sample`` around a stub model
that does the input cast of ``TransformerNetModel.forward`` and returns the fixed prediction.
The four-term update of the multistep samplers (``a_prev`` times the previous step's prediction,
``fused4_*``) is timed next to the three-term one and next to a composition of the three-term
kernel and a PyTorch ``add_`` (``fused3_plus_add_*``).
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
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "max_ms": round(max(v), 4)} for k, v in times.items()}


def shape(N, L, E, V, reps):
    from distributed_pipeline_amd.models import create_gaussian_diffusion
    from distributed_pipeline_amd.ops import diffusion as dops
    B = N // L
    g = torch.Generator(device="cuda").manual_seed(0)
    W = torch.randn(V, E, device="cuda", generator=g)
    ids = torch.randint(0, V, (B, L), device="cuda", generator=g)
    x_start = W[ids]
    x = torch.randn(B, L, E, device="cuda", generator=g)
    pred16 = torch.randn(B, L, E, device="cuda", generator=g).bfloat16()
    idx = torch.randint(0, V, (B, L), device="cuda", generator=g)
    mask = torch.zeros(B, L, dtype=torch.long, device="cuda")
    mask[:, L // 2:] = 1
    diff = create_gaussian_diffusion(steps=2000)
    t = torch.full((B,), 1000, dtype=torch.long, device="cuda")
    _, a, b, s = diff.reverse_schedule()[2000 - 1 - 1000]

    def stub(xin, ts):
        xin.to(torch.bfloat16)  # the forward's input cast; the fused op writes that copy itself
        return pred16

    def gather(p, tt):  # round_to_embeds without its arg-max: the cast it feeds the arg-max, the gather
        p.to(torch.bfloat16)
        return torch.nn.functional.embedding(idx, W)

    def chain(fn):
        def run():
            with torch.no_grad():
                return diff.p_sample(stub, x, t, mask, x_start, denoised_fn=fn)
        return run

    def fused(top_p, rounded):
        src = dict(idx=idx, weight=W) if rounded else dict(pred=pred16)
        return lambda: dops.reverse_step(x, x_start=x_start, mask=mask, a=a, b=b, s=s, seed=1, step=1000,
                                         top_p=top_p, want_bf16=True, **src)

    # the multistep (DPM-Solver++ 2M) update: the previous step's prediction as a fourth term, in the
    # same kernel, or added by a PyTorch add_ to the three-term kernel's output (two launches, after
    # a gather on the rounded steps).  The composition is timed as a lower bound of what it would
    # cost: it neither keeps the source rows at x_start nor refreshes the bf16 copy.
    prev16 = torch.randn(B, L, E, device="cuda", generator=g).bfloat16()
    idx_prev = torch.randint(0, V, (B, L), device="cuda", generator=g)
    _, a4, b4, s4, a_prev = diff.reverse_schedule(4, "dpmpp_2m_sde")[1]

    def four(rounded):
        src = dict(idx=idx, idx_prev=idx_prev, weight=W) if rounded else dict(pred=pred16, pred_prev=prev16)
        return lambda: dops.reverse_step(x, x_start=x_start, mask=mask, a=a4, b=b4, s=s4, a_prev=a_prev, seed=1,
                                         step=1000, want_bf16=True, **src)

    def two_launch(rounded):
        three = fused(0.0, rounded)

        def run():
            y, _ = three()
            return y.add_(torch.nn.functional.embedding(idx_prev, W) if rounded else prev16, alpha=a_prev)
        return run

    inner = 200 if N >= 65536 else 1000  # every window is tens of milliseconds of device work
    out = interleaved({
        "chain_unrounded": (chain(None), inner),
        "fused_unrounded": (fused(0.0, False), inner),
        "fused_unrounded_top_p0.9": (fused(0.9, False), inner),
        "fused4_unrounded": (four(False), inner),
        "fused3_plus_add_unrounded": (two_launch(False), inner),
        "chain_rounded": (chain(gather), inner),
        "fused_rounded": (fused(0.0, True), inner),
        "fused_rounded_top_p0.9": (fused(0.9, True), inner),
        "fused4_rounded": (four(True), inner),
        "fused3_plus_add_rounded": (two_launch(True), inner),
    }, reps)
    for kind in ("unrounded", "rounded"):
        out[f"fused4_{kind}"]["vs_three_term"] = round(
            out[f"fused4_{kind}"]["median_ms"] / out[f"fused_{kind}"]["median_ms"], 3)
        out[f"fused3_plus_add_{kind}"]["vs_four_term"] = round(
            out[f"fused3_plus_add_{kind}"]["median_ms"] / out[f"fused4_{kind}"]["median_ms"], 3)
    # bytes the update needs: x_t, x_start on the source half, the prediction (bf16) or the
    # gathered rows (fp32) on the target half, both outputs
    tgt = float((mask != 0).float().mean())
    need = {"unrounded": N * E * (4 * tgt + 4 * (1 - tgt) + 2 * tgt + 4 + 2),
            "rounded": N * E * (4 * tgt + 4 * (1 - tgt) + 4 * tgt + 4 + 2)}
    for kind in need:
        for name in (f"fused_{kind}", f"fused_{kind}_top_p0.9"):
            out[name]["needed_GBps"] = round(need[kind] / out[name]["median_ms"] / 1e6, 1)
            out[name]["speedup_vs_chain"] = round(out[f"chain_{kind}"]["median_ms"] / out[name]["median_ms"], 2)
    # the fourth term reads one more source on the target half: bf16, or gathered fp32 rows
    need4 = {"unrounded": need["unrounded"] + N * E * 2 * tgt, "rounded": need["rounded"] + N * E * 4 * tgt}
    for kind in need4:
        out[f"fused4_{kind}"]["needed_GBps"] = round(need4[kind] / out[f"fused4_{kind}"]["median_ms"] / 1e6, 1)
        out[f"fused4_{kind}"]["needed_bytes_vs_three_term"] = round(need4[kind] / need[kind], 3)
    return {"N": N, "L": L, "E": E, "V": V, "target_fraction": tgt, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="262144,8192")
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--E", type=int, default=128)
    ap.add_argument("--V", type=int, default=30522)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from distributed_pipeline_amd.ops._ext import get_ext
    get_ext(required=True)
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for n in (int(v) for v in a.N.split(",")):
        lines.append(json.dumps(shape(n, a.L, a.E, a.V, a.reps)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
