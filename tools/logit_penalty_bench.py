"""Time the logit processors of one GPT-2 decode step on ``[B, 50257]`` bf16 logits: the fused kernel
(csrc/logit_penalty.hip through ``ops.decode.penalize_logits_``) against the PyTorch path of the same op
(``penalize_logits_ref``, the yardstick, measured in the same run) and against the usual gather / where
/ scatter formulation in plain tensor ops, all on the same tensors.

    python tools/logit_penalty_bench.py [--B 8,64] [--n 128,1023] [--V 50257] [--Lh 1024] [--reps 7]
                                        [--spread_mb 768] [--out FILE]

Two settings: the repetition penalty alone, and all four processors (repetition 1.3, presence 0.5,
frequency 0.1, no-repeat 3-gram).  The histories are uniform random ids, ``n`` of ``Lh`` columns in use.
Consecutive calls of a variant take different logits and histories, so that ``spread_mb`` of logits lie
between two uses of one tensor.  The op works in place, so a tensor's values drift from call to call;
no variant's work depends on them.

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

SETTINGS = {"repetition": dict(repetition_penalty=1.3),
            "all four": dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.1, no_repeat_ngram=3)}


def usual(logits, hist, n, *, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0):
    """What one writes without the op: gather / where / scatter for the repetition penalty, a ``[B, V]``
    count for presence and frequency, an ``unfold`` compare for the n-gram ban.  fp32 arithmetic on the
    gathered values; not bit-equal to the op (padding is handled by pointing it at the row's first id)."""
    B, Lh = hist.shape
    V = logits.shape[1]
    inside = torch.arange(Lh, device=hist.device).view(1, Lh) < n.view(B, 1)
    ids = torch.where(inside, hist, hist[:, :1]).long()
    s = logits.gather(1, ids).float()
    s = torch.where(s < 0, s * repetition_penalty, s / repetition_penalty)
    if presence_penalty or frequency_penalty:
        count = torch.zeros(B, V, dtype=torch.float32, device=hist.device)
        count.scatter_add_(1, ids, inside.float())
        c = count.gather(1, ids)
        s = s - (presence_penalty + frequency_penalty * c)
    logits.scatter_(1, ids, s.to(logits.dtype))
    g = int(no_repeat_ngram)
    if g >= 1 and Lh >= g:
        win = hist.unfold(1, g, 1)  # [B, Lh - g + 1, g]
        nw = Lh - g + 1
        tail = n.long().view(B, 1) - (g - 1) + torch.arange(g - 1, device=hist.device).view(1, g - 1)
        last = hist.gather(1, tail.clamp(0, Lh - 1))  # the window's last g - 1 ids
        at = torch.arange(nw, device=hist.device).view(1, nw)
        hit = (win[:, :, :g - 1] == last.unsqueeze(1)).all(-1) & (at + g <= n.view(B, 1))
        mask = torch.zeros(B, V + 1, dtype=torch.bool, device=hist.device)  # column V takes the misses
        mask.scatter_(1, torch.where(hit, win[:, :, g - 1], V).long(), True)
        logits.masked_fill_(mask[:, :V], float("-inf"))
    return logits


def shape(B, V, Lh, n_used, reps, spread_bytes):
    from distributed_pipeline_amd.ops._ext import get_ext
    from distributed_pipeline_amd.ops.decode import penalize_logits_, penalize_logits_ref
    get_ext(required=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    nbytes = B * V * 2
    nsets = max(2, -(-spread_bytes // nbytes))
    logits = [(torch.randn(B, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(nsets)]
    hists = [torch.randint(0, V, (B, Lh), device="cuda", generator=g, dtype=torch.int32) for _ in range(nsets)]
    n = torch.full((B,), n_used, dtype=torch.int32, device="cuda")
    rows = []
    for name, kw in SETTINGS.items():
        turn = {"kernel": 0, "pytorch_path": 0, "usual": 0}

        def nxt(which):
            turn[which] = (turn[which] + 1) % nsets
            return turn[which]

        def kernel():
            i = nxt("kernel")
            return penalize_logits_(logits[i], hists[i], n, **kw)

        def torch_path():
            i = nxt("pytorch_path")
            return penalize_logits_ref(logits[i], hists[i], n, **kw)

        def plain():
            i = nxt("usual")
            return usual(logits[i], hists[i], n, **kw)

        out = interleaved({"kernel": (kernel, 200), "pytorch_path": (torch_path, 10), "usual": (plain, 50)}, reps)
        out["kernel"]["speedup_vs_pytorch_path"] = round(out["pytorch_path"]["median_ms"] / out["kernel"]["median_ms"], 1)
        out["kernel"]["speedup_vs_usual"] = round(out["usual"]["median_ms"] / out["kernel"]["median_ms"], 1)
        rows.append({"B": B, "V": V, "Lh": Lh, "n": n_used, "setting": name, "logit_sets": nsets, **out})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="8,64")
    ap.add_argument("--n", default="128,1023")
    ap.add_argument("--V", type=int, default=50257)
    ap.add_argument("--Lh", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spread_mb", type=int, default=768, help="logits between two uses of one tensor, MB")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for B in (int(x) for x in a.B.split(",")):
        for n in (int(x) for x in a.n.split(",")):
            for row in shape(B, a.V, a.Lh, n, a.reps, a.spread_mb << 20):
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
