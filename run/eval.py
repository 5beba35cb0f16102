"""
Entry point: ``python -m run.eval --path out.jsonl``

Scores a file written by ``run.sample`` and prints one JSON line:

* ``n``: rows; ``bleu``: mean ``sentence_bleu(recover, reference)`` (utils/mbr.py); ``len``: mean
  length of ``recover``; ``dist1``: mean over rows of distinct unigrams / length (0 for an empty
  row);
* ``self_bleu`` (rows written with ``--keep_candidates true``): mean over rows of the mean BLEU
  of a row's candidates against each other (every ordered pair i != j) - lower is more diverse;
* with ``--rouge_l true`` also ``rouge_l``: mean ``rouge_l(recover, reference)`` (utils/rouge.py),
  and ``self_rouge_l``: as ``self_bleu`` with ROUGE-L;
* with ``--diversity true`` also ``dist2``, ``dist3``, ``dist4``: mean over rows of
  ``dist_n(recover, n)``, distinct n-grams / n-grams (0 for a row without an n-gram), and, for rows
  with more than one candidate, ``div4``: mean over those rows of ``div_n(candidates, 4)``, the
  distinct 4-grams of a row's candidates / the sum of their 4-gram totals (utils/diversity.py) -
  higher is more diverse.

The BLEU numbers come from ``ops.text.ngram_matches`` on the ``[recover, reference]`` pairs and on
the candidate groups (one kernel per batch of rows on a GPU, the same integers on the CPU), the
ROUGE-L numbers from ``ops.text.lcs_lengths`` on the same padded batches, the diversity numbers
from ``ops.text.ngram_distinct`` on the ``recover`` rows as groups of one and on the candidate groups.
"""
import json

from config.eval import EvalSettings


def create_parser():
    return EvalSettings.to_argparse()


def _padded(groups, device):
    """Equal-sized groups of id lists -> (tokens [G, K, L], lens [G, K]) on ``device``."""
    import torch

    L = max(1, max(len(seq) for grp in groups for seq in grp))
    tokens = torch.tensor([[seq + [0] * (L - len(seq)) for seq in grp] for grp in groups], dtype=torch.long)
    lens = torch.tensor([[len(seq) for seq in grp] for grp in groups], dtype=torch.long)
    return tokens.to(device), lens.to(device)


def evaluate(rows, device, batch_size=4096, rouge_l=False, diversity=False):
    """The metrics of ``rows`` (dicts with ``recover``, ``reference`` and optionally ``candidates``);
    ``rouge_l``: also ``rouge_l`` and, for rows with candidates, ``self_rouge_l``; ``diversity``:
    also ``dist2``, ``dist3``, ``dist4`` and, for rows with candidates, ``div4``."""
    from utils.diversity import dist_n_batch, div_n_batch
    from utils.mbr import pairwise_bleu
    from utils.rouge import pairwise_rouge_l

    bleu, self_bleu, rouge, self_rouge, dist, div4 = [], [], [], [], [], []

    def off_diagonal(pw, k):  # mean over the ordered pairs i != j
        return sum(pw[i][j] for i in range(k) for j in range(k) if i != j) / (k * (k - 1))

    for r0 in range(0, len(rows), batch_size):
        part = rows[r0:r0 + batch_size]
        pairs = _padded([[r["recover"], r["reference"]] for r in part], device)
        bleu += pairwise_bleu(*pairs)[:, 0, 1].tolist()
        if rouge_l:
            rouge += pairwise_rouge_l(*pairs)[:, 0, 1].tolist()
        if diversity:
            dist += dist_n_batch(*_padded([[r["recover"]] for r in part], device))[:, 0].tolist()
        by_k = {}
        for r in part:
            if len(r.get("candidates", ())) > 1:
                by_k.setdefault(len(r["candidates"]), []).append(r["candidates"])
        for k, groups in by_k.items():
            cands = _padded(groups, device)
            for pb in pairwise_bleu(*cands).tolist():
                self_bleu.append(off_diagonal(pb, k))
            if rouge_l:
                for pr in pairwise_rouge_l(*cands).tolist():
                    self_rouge.append(off_diagonal(pr, k))
            if diversity:
                div4 += div_n_batch(*cands)[:, 3].tolist()
    n = len(rows)
    mean = lambda xs: sum(xs) / len(xs) if xs else 0.0  # noqa: E731
    out = {"n": n, "bleu": mean(bleu), "len": mean([len(r["recover"]) for r in rows]),
           "dist1": mean([len(set(r["recover"])) / len(r["recover"]) if r["recover"] else 0.0 for r in rows])}
    if self_bleu:
        out["self_bleu"] = mean(self_bleu)
    if rouge_l:
        out["rouge_l"] = mean(rouge)
        if self_rouge:
            out["self_rouge_l"] = mean(self_rouge)
    if diversity:
        for o in (2, 3, 4):
            out[f"dist{o}"] = mean([d[o - 1] for d in dist])
        if div4:
            out["div4"] = mean(div4)
    return out


def main(namespace):
    args: EvalSettings = EvalSettings.from_argparse(namespace)

    import torch

    with open(args.path) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    dev = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    out = evaluate(rows, dev, args.batch_size, rouge_l=args.rouge_l, diversity=args.diversity)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main(create_parser().parse_args())
