"""
Entry point: ``python -m run.eval --path out.jsonl``

Scores a file written by ``run.sample`` and prints one JSON line:

* ``n``: rows; ``bleu``: mean ``sentence_bleu(recover, reference)`` (utils/mbr.py); ``len``: mean
  length of ``recover``; ``dist1``: mean over rows of distinct unigrams / length (0 for an empty
  row);
* ``self_bleu`` (rows written with ``--keep_candidates true``): mean over rows of the mean BLEU
  of a row's candidates against each other (every ordered pair i != j) - lower is more diverse.

The BLEU numbers come from ``ops.text.ngram_matches`` on the ``[recover, reference]`` pairs and on
the candidate groups (one kernel per batch of rows on a GPU, the same integers on the CPU).
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


def evaluate(rows, device, batch_size=4096):
    """The metrics of ``rows`` (dicts with ``recover``, ``reference`` and optionally ``candidates``)."""
    from utils.mbr import pairwise_bleu

    bleu, self_bleu = [], []
    for r0 in range(0, len(rows), batch_size):
        part = rows[r0:r0 + batch_size]
        bleu += pairwise_bleu(*_padded([[r["recover"], r["reference"]] for r in part], device))[:, 0, 1].tolist()
        by_k = {}
        for r in part:
            if len(r.get("candidates", ())) > 1:
                by_k.setdefault(len(r["candidates"]), []).append(r["candidates"])
        for k, groups in by_k.items():
            for pb in pairwise_bleu(*_padded(groups, device)).tolist():
                self_bleu.append(sum(pb[i][j] for i in range(k) for j in range(k) if i != j) / (k * (k - 1)))
    n = len(rows)
    mean = lambda xs: sum(xs) / len(xs) if xs else 0.0  # noqa: E731
    out = {"n": n, "bleu": mean(bleu), "len": mean([len(r["recover"]) for r in rows]),
           "dist1": mean([len(set(r["recover"])) / len(r["recover"]) if r["recover"] else 0.0 for r in rows])}
    if self_bleu:
        out["self_bleu"] = mean(self_bleu)
    return out


def main(namespace):
    args: EvalSettings = EvalSettings.from_argparse(namespace)

    import torch

    with open(args.path) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    dev = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    out = evaluate(rows, dev, args.batch_size)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main(create_parser().parse_args())
