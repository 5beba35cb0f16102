"""Time the diversity metrics of run.eval: the pure-Python set versions ``div_n`` / ``dist_n``
(utils/diversity.py) against ``div_n_batch`` / ``dist_n_batch`` (one distinct n-gram kernel,
csrc/ngram_distinct.hip, one copy of the counts, the divisions on the host), the kernel alone and,
as the yardstick, the n-gram match kernel (csrc/ngram_match.hip) alone on the same tensors.

    python tools/diversity_bench.py [--B 2048,64] [--K 10,1] [--L 64] [--min_len 30] [--py_groups 64] [--reps 7] [--out FILE]

A shape is B sources with K candidates of min_len..L tokens each, the candidates of
tools/mbr_bench.py; K = 1 is the ``recover`` case of run.eval (one sequence per source, as groups
of one).  For K > 1 the metric is div-n, n = 1..4, of every source (``div_n`` in a loop
against one ``div_n_batch`` call), for K = 1 it is dist-n, n = 1..4, of every sequence (``dist_n``
against ``dist_n_batch``).  The four variants are timed in turn inside each repetition
(interleaved); medians and min-max over the repetitions.  ``python_sets`` runs on the first
``py_groups`` sources only, one source at a time (wall clock), and ``python_sets_scaled_to_B``
scales its median linearly to B - it is not measured at B; ``batch_end_to_end`` is the wall clock of
one batch call on device tensors, device work, copy and host finish included; ``distinct_kernel``
and ``ngram_kernel`` are ``ngram_distinct`` / ``ngram_matches`` between two device events.  The
batch results are compared with the list versions, exactly, on the timed sources.  Nothing here is
a target: the set version is cheap, and a ratio below 1 is a result like any other.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.mbr_bench import candidates, events, stats, wall  # noqa: E402


def shape(B, K, L, min_len, py_groups, reps):
    from distributed_pipeline_amd.ops.text import ngram_distinct, ngram_matches
    from utils.diversity import dist_n, dist_n_batch, div_n, div_n_batch
    tokens, lens = candidates(B, K, L, min_len)
    n_py = min(py_groups, B)
    lists = [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(n_py)]
    tok_d, len_d = tokens.cuda(), lens.cuda()
    if K > 1:
        metric = "div_n"
        python = lambda: [[div_n(c, n) for n in range(1, 5)] for c in lists]  # noqa: E731
        batch = lambda: div_n_batch(tok_d, len_d)  # noqa: E731
    else:
        metric = "dist_n"
        python = lambda: [[[dist_n(c[0], n) for n in range(1, 5)]] for c in lists]  # noqa: E731
        batch = lambda: dist_n_batch(tok_d, len_d)  # noqa: E731
    assert torch.equal(batch()[:n_py], torch.tensor(python(), dtype=torch.float64)), \
        "the batch values differ from the list versions"
    for _ in range(3):
        ngram_distinct(tok_d, len_d)
        ngram_matches(tok_d, len_d)
    times = {"python_sets": [], "batch_end_to_end": [], "distinct_kernel": [], "ngram_kernel": []}
    for _ in range(reps):
        times["python_sets"].append(wall(python))
        times["batch_end_to_end"].append(wall(batch))
        times["distinct_kernel"].append(events(lambda: ngram_distinct(tok_d, len_d), 20))
        times["ngram_kernel"].append(events(lambda: ngram_matches(tok_d, len_d), 20))
    out = {k: stats(v) for k, v in times.items()}
    out["python_sets"]["groups"] = n_py
    scaled = out["python_sets"]["median_ms"] * B / n_py
    out["python_sets_scaled_to_B"] = {"median_ms": round(scaled, 2)}
    out["batch_end_to_end"]["speedup_vs_python"] = round(scaled / out["batch_end_to_end"]["median_ms"], 2)
    out["distinct_kernel"]["ratio_to_ngram_kernel"] = round(
        out["distinct_kernel"]["median_ms"] / out["ngram_kernel"]["median_ms"], 2)
    return {"B": B, "K": K, "L": L, "min_len": min_len, "metric": metric, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="2048,64")
    ap.add_argument("--K", default="10,1")
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
    for k in (int(v) for v in a.K.split(",")):
        for b in (int(v) for v in a.B.split(",")):
            lines.append(json.dumps(shape(b, k, a.L, a.min_len, a.py_groups, a.reps)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
