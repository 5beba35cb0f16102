"""Time the choice of the next token on GPT-2's ``[B, 50257]`` bf16 logits: the fused kernel
(csrc/sample.hip through ``ops.decode.sample_tokens``) against ``utils.lm_sampling.sample_next`` with
a device generator on the same tensors - the yardstick, measured in the same run - and against a
device copy of the logits' bytes (B * V * 2).

    python tools/sample_bench.py [--B 8,64] [--V 50257] [--reps 7] [--spread_mb 768] [--out FILE]

Three settings: plain temperature, ``top_k = 50``, ``top_p = 0.9`` (temperature 0.8 throughout).
Consecutive calls of a variant take different logit tensors (and the copy different buffers), so
that ``spread_mb`` of reads pass before one repeats and nothing is served from the last-level cache.

Every variant of a shape is timed in turn inside each repetition (interleaved); a repetition is
``inner`` back-to-back calls between two device events; medians and min-max over the repetitions.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.attn_decode_bench import interleaved  # noqa: E402

SETTINGS = {"temperature": dict(top_k=0, top_p=0.0), "top_k=50": dict(top_k=50, top_p=0.0),
            "top_p=0.9": dict(top_k=0, top_p=0.9)}
TEMPERATURE = 0.8


def shape(B, V, reps, spread_bytes):
    from distributed_pipeline_amd.ops._ext import get_ext
    from distributed_pipeline_amd.ops.decode import sample_tokens
    from utils.lm_sampling import sample_next
    get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = B * V * 2
    nsets = max(2, -(-spread_bytes // nbytes))
    logits = [(torch.randn(B, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(nsets)]
    dst = [torch.empty_like(t) for t in logits]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for name, kw in SETTINGS.items():
        turn = {"kernel": 0, "sample_next": 0, "copy": 0}

        def nxt(which):
            turn[which] = (turn[which] + 1) % nsets
            return turn[which]

        def kernel():
            i = nxt("kernel")
            return sample_tokens(logits[i], temperature=TEMPERATURE, seed=102, step=turn["kernel"], **kw)

        def torch_path():
            return sample_next(logits[nxt("sample_next")], TEMPERATURE, generator=gen, **kw)

        def copy():
            i = nxt("copy")
            return dst[i].copy_(logits[i])

        out = interleaved({"kernel": (kernel, 200), "sample_next": (torch_path, 20), "copy": (copy, 200)}, reps)
        out["kernel"]["speedup_vs_sample_next"] = round(out["sample_next"]["median_ms"] / out["kernel"]["median_ms"], 2)
        out["kernel"]["times_the_copy"] = round(out["kernel"]["median_ms"] / out["copy"]["median_ms"], 2)
        rows.append({"B": B, "V": V, "setting": name, "temperature": TEMPERATURE, "logit_bytes": nbytes,
                     "logit_sets": nsets, **out})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="8,64")
    ap.add_argument("--V", type=int, default=50257)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spread_mb", type=int, default=768, help="bytes read before a logits tensor is reused, MB")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for B in (int(x) for x in a.B.split(",")):
        for row in shape(B, a.V, a.reps, a.spread_mb << 20):
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
