"""
Entry point: ``python -m run.score --config_json cfg.json --model_path DIR [--path out.jsonl]``

Teacher-forced scoring with a trained GPT-2 checkpoint (one process; one GPU, or the CPU): settings
-> model -> state dict -> ``eval()`` -> ``GPT2LMModel.score`` on batches of token rows -> perplexity,
top-k accuracy, entropy and, on request, every token's log-probability and rank.

Without ``--path`` the rows are the ``input_ids`` of ``--split`` (``--num_batches`` batches of
``--batch_size``), each scored from position ``--prompt_len`` on: the tokens in front are context
only.  With ``--path`` the rows come from a ``run.generate`` file: each line is ``prompt + <field>``
(``--field continuation`` or ``reference``), right-padded within its batch and scored from
``len(prompt)`` on, so the numbers speak of the continuation alone; the whole file is scored.

stdout gets one JSON line: ``n_rows``, ``n_tokens``, ``nll`` (mean per token, nats), ``ppl``,
``bits_per_token``, ``top1``, ``top5`` (the share of tokens with rank < 5) and ``entropy`` (mean), all
sums in float64.  ``--out_path`` gets one JSON line per row: ``tokens``, ``nll`` (sum, nats), ``ppl``
(``exp(nll / tokens)``, null at 0 tokens), ``top1_acc``, ``mean_rank``, ``mean_entropy`` and, with
``--keep_tokens true``, the ``logprobs`` and ``ranks`` lists.

``--config_json`` takes the ``training_args.json`` of the training run as it is (config/score.py);
checkpoints are found and loaded as by ``run.generate``.
"""
import json
import math
import os

from config.score import ScoreSettings
from run.sample import find_checkpoint, shadow_frozen_weights


def create_parser():
    return ScoreSettings.to_argparse(add_json=True)


def read_rows(path, field, seq_len):
    """The rows of a ``run.generate`` file -> [(ids, prompt length)]."""
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            rec = json.loads(line)
            if "prompt" not in rec or field not in rec:
                raise ValueError(f"{path}, line {no}: no 'prompt' or no {field!r}")
            ids = list(rec["prompt"]) + list(rec[field])
            if len(ids) > seq_len:
                raise ValueError(f"{path}, line {no}: {len(ids)} tokens exceed seq_len {seq_len}")
            rows.append((ids, len(rec["prompt"])))
    return rows


def main(namespace):
    args: ScoreSettings = ScoreSettings.from_argparse(namespace)
    args.check()  # the model family and the scoring values, before any checkpoint is read
    rows = read_rows(args.path, args.field, args.seq_len) if args.path else None

    import torch

    from basic_utils import dist_util
    from utils.initialization import create_model_from_config

    dev = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda":
        torch.cuda.set_device(dev)

    settings = {k: v for k, v in args.dict().items() if k != "path"}
    model = create_model_from_config(**settings)
    ckpt = find_checkpoint(args.model_path, args.use_ema)
    print(f"### loading {ckpt}")
    model.load_state_dict(dist_util.load_state_dict(ckpt, map_location="cpu"))
    model.to(dev).eval()
    if args.precision == "bf16":
        shadow_frozen_weights(model)

    def batches():
        """-> (ids [B, L] on the device, lens, start) per batch."""
        if rows is None:
            from data import load_data_from_args
            # seed=0, as in run.generate: the rows of a split do not depend on a sampling seed
            data = load_data_from_args(split=args.split, data_dir=args.data_dir, batch_size=args.batch_size,
                                       deterministic=True, loop=False, num_loader_proc=0,
                                       dataset=args.dataset, seq_len=args.seq_len, vocab_size=args.vocab_size,
                                       seed=0, model=args.model)
            for b, batch in enumerate(data):
                if b >= args.num_batches:
                    break
                ids = batch["input_ids"].to(dev)
                B, L = ids.shape
                yield ids, torch.full((B,), L), torch.full((B,), args.prompt_len)
            return
        for r0 in range(0, len(rows), args.batch_size):
            part = rows[r0:r0 + args.batch_size]
            L = max(len(ids) for ids, _ in part)
            ids = torch.zeros(len(part), L, dtype=torch.long)
            for i, (row, _) in enumerate(part):
                ids[i, :len(row)] = torch.tensor(row, dtype=torch.long)
            yield ids.to(dev), torch.tensor([len(row) for row, _ in part]), torch.tensor([p for _, p in part])

    fout = None
    if args.out_path:
        os.makedirs(os.path.dirname(os.path.abspath(args.out_path)), exist_ok=True)
        fout = open(args.out_path, "w")
    tot = {"rows": 0, "tokens": 0, "nll": 0.0, "top1": 0, "top5": 0, "entropy": 0.0}
    try:
        for ids, lens, start in batches():
            res = {k: v.cpu() for k, v in model.score(ids, lens.to(dev), start=start.to(dev)).items()}
            mask = res["mask"]
            for i in range(ids.shape[0]):
                m = mask[i]
                n = int(m.sum())
                lp, rk, en = res["logp"][i][m].double(), res["rank"][i][m], res["entropy"][i][m].double()
                nll = 0.0 - float(lp.sum())
                tot["rows"] += 1
                tot["tokens"] += n
                tot["nll"] += nll
                tot["top1"] += int((rk == 0).sum())
                tot["top5"] += int((rk < 5).sum())
                tot["entropy"] += float(en.sum())
                if fout is not None:
                    line = {"tokens": n, "nll": nll, "ppl": math.exp(nll / n) if n else None,
                            "top1_acc": float((rk == 0).double().mean()) if n else None,
                            "mean_rank": float(rk.double().mean()) if n else None,
                            "mean_entropy": float(en.mean()) if n else None}
                    if args.keep_tokens:
                        line["logprobs"] = [float(x) for x in lp]
                        line["ranks"] = [int(x) for x in rk]
                    fout.write(json.dumps(line) + "\n")
    finally:
        if fout is not None:
            fout.close()
    n = tot["tokens"]
    mean = tot["nll"] / n if n else None
    summary = {"n_rows": tot["rows"], "n_tokens": n, "nll": mean,
               "ppl": math.exp(mean) if n else None, "bits_per_token": mean / math.log(2) if n else None,
               "top1": tot["top1"] / n if n else None, "top5": tot["top5"] / n if n else None,
               "entropy": tot["entropy"] / n if n else None}
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main(create_parser().parse_args())
