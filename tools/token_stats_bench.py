"""Time teacher-forced token statistics on GPT-2's ``[B, 50257]`` bf16 logits: the fused kernel
(csrc/token_stats.hip through ``ops.decode.token_stats``) against the PyTorch chain on the same
tensors - ``log_softmax``, ``gather``, a compare-and-count for the rank, ``argmax`` and the
``exp * log`` sum of the entropy, in fp32; the yardstick, measured in the same run - and against a
device copy of the logits' bytes (B * V * 2).

    python tools/token_stats_bench.py [--B 8,64,4096] [--V 50257] [--reps 7] [--spread_mb 768] [--out FILE]

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


def torch_chain(logits, targets):
    """logp, rank, entropy and top1 as one would write them without the op (no NaN handling)."""
    s = logits.float()
    t = targets.view(-1, 1)
    lsm = torch.log_softmax(s, -1)
    logp = lsm.gather(1, t).squeeze(1)
    st = s.gather(1, t)
    ids = torch.arange(s.shape[1], device=s.device).view(1, -1)
    rank = (s > st).sum(-1) + ((s == st) & (ids < t)).sum(-1)
    entropy = -(torch.exp(lsm) * lsm).sum(-1)
    return logp, rank, entropy, s.argmax(-1)


def shape(B, V, reps, spread_bytes):
    from distributed_pipeline_amd.ops._ext import get_ext
    from distributed_pipeline_amd.ops.decode import token_stats
    get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = B * V * 2
    nsets = max(2, -(-spread_bytes // nbytes))
    logits = [(torch.randn(B, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(nsets)]
    targets = [torch.randint(0, V, (B,), device="cuda", generator=g) for _ in range(nsets)]
    dst = [torch.empty_like(t) for t in logits]
    turn = {"kernel": 0, "torch_chain": 0, "copy": 0}

    def nxt(which):
        turn[which] = (turn[which] + 1) % nsets
        return turn[which]

    def kernel():
        i = nxt("kernel")
        return token_stats(logits[i], targets[i])

    def chain():
        i = nxt("torch_chain")
        return torch_chain(logits[i], targets[i])

    def copy():
        i = nxt("copy")
        return dst[i].copy_(logits[i])

    # the two paths agree on what they time
    a, b = kernel(), chain()
    assert torch.equal(a[1].long(), b[1]) and torch.equal(a[3].long(), b[3])
    assert torch.allclose(a[0], b[0], rtol=0, atol=1e-4) and torch.allclose(a[2], b[2], rtol=0, atol=1e-4)

    few = B >= 1024  # a call takes long enough for few of them to fill a repetition
    out = interleaved({"kernel": (kernel, 20 if few else 200), "torch_chain": (chain, 3 if few else 20),
                       "copy": (copy, 20 if few else 200)}, reps)
    out["kernel"]["speedup_vs_torch_chain"] = round(out["torch_chain"]["median_ms"] / out["kernel"]["median_ms"], 2)
    out["kernel"]["times_the_copy"] = round(out["kernel"]["median_ms"] / out["copy"]["median_ms"], 2)
    return {"B": B, "V": V, "logit_bytes": nbytes, "logit_sets": nsets, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="8,64,4096")
    ap.add_argument("--V", type=int, default=50257)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spread_mb", type=int, default=768, help="bytes read before a logits tensor is reused, MB")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for B in (int(x) for x in a.B.split(",")):
        lines.append(json.dumps(shape(B, a.V, a.reps, a.spread_mb << 20)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
