"""Time ROUGE-L minimum-Bayes-risk selection among decoded candidates: the pure-Python
``mbr_select(metric="rouge_l")`` (utils/mbr.py, utils/rouge.py) against
``mbr_select_batch(metric="rouge_l")`` (one LCS kernel, csrc/lcs.hip, one copy of the lengths, the
closed-form ROUGE-L on the host), the LCS kernel alone and, as the yardstick, the n-gram match
kernel (csrc/ngram_match.hip) alone on the same tensors.

    python tools/lcs_bench.py [--B 2048,64] [--K 10] [--L 64] [--min_len 30] [--py_groups 64] [--reps 7] [--out FILE]

A shape is B sources with K candidates of min_len..L tokens each, the candidates of
tools/mbr_bench.py.  The four variants are timed in turn inside each repetition (interleaved);
medians and min-max over the repetitions.  ``python_mbr_select`` runs on the first ``py_groups``
sources only, one source at a time (wall clock), and ``python_mbr_select_scaled_to_B`` scales its
median linearly to B - it is not measured at B; ``batch_end_to_end`` is the wall clock of one
``mbr_select_batch`` call on device tensors, device work, copy and host finish included;
``lcs_kernel`` and ``ngram_kernel`` are ``lcs_lengths`` / ``ngram_matches`` between two device
events.  The picks of both paths are compared on the timed subset.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.mbr_bench import candidates, events, stats, wall  # noqa: E402


def shape(B, K, L, min_len, py_groups, reps):
    from distributed_pipeline_amd.ops.text import lcs_lengths, ngram_matches
    from utils.mbr import mbr_select, mbr_select_batch
    tokens, lens = candidates(B, K, L, min_len)
    n_py = min(py_groups, B)
    lists = [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(n_py)]
    tok_d, len_d = tokens.cuda(), lens.cuda()
    picks = mbr_select_batch(tok_d, len_d, metric="rouge_l")
    assert picks[:n_py] == [mbr_select(c, metric="rouge_l") for c in lists], "the batch picks differ from mbr_select"
    for _ in range(3):
        lcs_lengths(tok_d, len_d)
        ngram_matches(tok_d, len_d)
    times = {"python_mbr_select": [], "batch_end_to_end": [], "lcs_kernel": [], "ngram_kernel": []}
    for _ in range(reps):
        times["python_mbr_select"].append(wall(lambda: [mbr_select(c, metric="rouge_l") for c in lists]))
        times["batch_end_to_end"].append(wall(lambda: mbr_select_batch(tok_d, len_d, metric="rouge_l")))
        times["lcs_kernel"].append(events(lambda: lcs_lengths(tok_d, len_d), 20))
        times["ngram_kernel"].append(events(lambda: ngram_matches(tok_d, len_d), 20))
    out = {k: stats(v) for k, v in times.items()}
    out["python_mbr_select"]["groups"] = n_py
    scaled = out["python_mbr_select"]["median_ms"] * B / n_py
    out["python_mbr_select_scaled_to_B"] = {"median_ms": round(scaled, 2)}
    out["batch_end_to_end"]["speedup_vs_python"] = round(scaled / out["batch_end_to_end"]["median_ms"], 2)
    out["lcs_kernel"]["ratio_to_ngram_kernel"] = round(
        out["lcs_kernel"]["median_ms"] / out["ngram_kernel"]["median_ms"], 2)
    return {"B": B, "K": K, "L": L, "min_len": min_len, "metric": "rouge_l", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="2048,64")
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--min_len", type=int, default=30)
    ap.add_argument("--py_groups", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from distributed_pipeline_amd.ops._ext import get_ext
    get_ext(required=True)
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "torch": torch.__version__})]
    for b in (int(v) for v in a.B.split(",")):
        lines.append(json.dumps(shape(b, a.K, a.L, a.min_len, a.py_groups, a.reps)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
