"""Time the fused linear + arg-max (csrc/linear_argmax.hip) against lxent_fwd and the chunked
PyTorch path, and the rounding's share of a DiffuSeq reverse step.

    python tools/linear_argmax_bench.py [--N 262144,8192] [--V 30522] [--E 128] [--reps 7]
                                        [--step-batch 2048] [--out FILE]

Every variant of one shape is timed in turn inside each repetition (interleaved), a repetition
is ``inner`` back-to-back calls between two device events, and the median and the min-max spread
over the repetitions are reported.  ``argmax_3calls`` is the same work as three calls of at most
130944 tokens, i.e. on the 8-split (one per XCD) grid instead of the single sweep that
N > 130944 takes: the A/B of the two large-N schedules.
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


def interleaved(variants, reps, warmup=2):
    """variants: {name: (fn, inner)} -> {name: {"median_ms", "min_ms", "max_ms"}}"""
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


def kernel_shape(ext, ops, N, V, E, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(N, E, device="cuda", generator=g).bfloat16()
    W = (0.5 * torch.randn(V, E, device="cuda", generator=g)).bfloat16()
    bias = 0.1 * torch.randn(V, device="cuda", generator=g)
    b16 = bias.bfloat16()
    tgt = torch.randint(0, V, (N,), device="cuda", generator=g)
    c = ext.row_half_sqnorm(W)
    xf, Wf = x.float(), W.float()
    inner = 10 if N >= 65536 else 50
    variants = {
        "argmax_logits": (lambda: ext.linear_argmax(x, W, bias), inner),
        "argmax_nearest": (lambda: ext.linear_argmax(x, W, c), inner),
        "lxent_fwd": (lambda: ext.lxent_fwd(x, W, b16, tgt), inner),
        "row_half_sqnorm": (lambda: ext.row_half_sqnorm(W), 50),
        "fallback_nearest": (lambda: ops._linear_argmax_ref(xf, Wf, c), 1 if N >= 65536 else 5),
    }
    if N > 130944:
        parts = [x[i:i + 130944] for i in range(0, N, 130944)]
        variants["argmax_3calls"] = (lambda: [ext.linear_argmax(p, W, c) for p in parts], inner)
    out = interleaved(variants, reps)
    flop = 2.0 * N * V * E
    for k in ("argmax_logits", "argmax_nearest", "lxent_fwd"):
        out[k]["logit_TFLOPs"] = round(flop / out[k]["median_ms"] / 1e9, 1)
    # same answers from both paths on the rows whose top-2 gap is clear in fp32
    i_k, _ = ext.linear_argmax(x[:4096], W, c)
    i_f, _ = ops._linear_argmax_ref(xf[:4096], Wf, c)
    out["kernel_vs_fallback_index_mismatch_rows_of_4096"] = int((i_k != i_f).sum())
    return {"N": N, "V": V, "E": E, **out}


def reverse_step(ops, B, L, V, E, reps):
    """One DiffuSeq-base reverse step at batch B (bf16, eval, no_grad): the model forward, the
    rounding (kernel / PyTorch path) and the posterior update in PyTorch."""
    from distributed_pipeline_amd.models import TransformerNetModel, create_gaussian_diffusion
    torch.manual_seed(0)
    net = TransformerNetModel(vocab_size=V, input_dims=E, seq_len=L, config_name="bert-base-uncased",
                              compute_dtype=torch.bfloat16).cuda().eval()
    for p in net.parameters():
        p._dpa_shadow = p.detach().to(torch.bfloat16)
    diff = create_gaussian_diffusion(steps=2000)
    ids = torch.randint(1000, V, (B, L), device="cuda")
    mask = torch.zeros(B, L, dtype=torch.long, device="cuda")
    mask[:, L // 2:] = 1
    t = torch.full((B,), 1000, dtype=torch.long, device="cuda")
    with torch.no_grad():
        x_start = net.get_embeds(ids)
        x = torch.randn_like(x_start)
        c = net.rounding_offsets()
        W32 = net.word_embedding.weight.detach()
        W16f = ops.shadow(net.word_embedding.weight, torch.bfloat16).float()
        x0 = net(x, diff.scale_timesteps(t)).float()
        x2 = x0.reshape(-1, E)

        def fallback_round():
            idx, _ = ops._linear_argmax_ref(x2.bfloat16().float(), W16f, c)
            return torch.nn.functional.embedding(idx, W32)

        def nograd(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        variants = {
            "model_forward": (nograd(lambda: net(x, diff.scale_timesteps(t))), 2),
            "round_kernel": (nograd(lambda: net.round_to_embeds(x0, c)), 5),
            "round_fallback": (nograd(fallback_round), 1),
            "step_no_rounding": (nograd(lambda: diff.p_sample(net, x, t, mask, x_start)), 2),
            "step_round_kernel": (nograd(lambda: diff.p_sample(net, x, t, mask, x_start,
                                                               denoised_fn=lambda v, tt: net.round_to_embeds(v, c))), 2),
        }
        out = interleaved(variants, reps)
    step_k = out["step_round_kernel"]["median_ms"]
    step_f = out["step_no_rounding"]["median_ms"] + out["round_fallback"]["median_ms"]
    out["rounding_share_of_step_kernel"] = round(out["round_kernel"]["median_ms"] / step_k, 4)
    out["rounding_share_of_step_fallback"] = round(out["round_fallback"]["median_ms"] / step_f, 4)
    return {"batch": B, "seq_len": L, "tokens": B * L, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="262144,8192")
    ap.add_argument("--V", type=int, default=30522)
    ap.add_argument("--E", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-batch", type=int, default=2048, help="0: skip the reverse-step part")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from distributed_pipeline_amd.ops import nn as ops
    from distributed_pipeline_amd.ops._ext import get_ext
    ext = get_ext(required=True)
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for n in (int(s) for s in a.N.split(",")):
        lines.append(json.dumps(kernel_shape(ext, ops, n, a.V, a.E, a.reps)))
        print(lines[-1], flush=True)
    if a.step_batch:
        lines.append(json.dumps(reverse_step(ops, a.step_batch, 128, a.V, a.E, a.reps)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
