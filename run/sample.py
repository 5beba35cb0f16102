"""
Entry point: ``python -m run.sample --config_json cfg.json --model_path DIR --out_path out.jsonl``

Decodes a dataset split with a trained DiffuSeq checkpoint (one process; one GPU, or the CPU):
settings -> model + diffusion -> state dict -> ``eval()`` -> for each batch the reverse process
with every predicted x0 rounded to its nearest word embedding
(``GaussianDiffusion.sample_seq2seq``) -> one JSON line per sample with the ``source``,
``reference`` and ``recover`` token ids (padding stripped), and their texts when ``data_dir`` holds
a ``vocab.txt``.

``--config_json`` takes the ``training_args.json`` of the training run as it is
(config/sample.py).  A seed reproduces the output: by default the sampling noise comes from one
generator seeded with ``seed``.

``--step S`` decodes with a respaced chain of S steps, ``--sampler ddim --ddim_eta`` with DDIM
updates, ``--sampler dpmpp_2m`` / ``dpmpp_2m_sde`` with the second-order multistep DPM-Solver++
(deterministic / with noise; each update also reads the previous step's prediction, no extra
forward; ``--ddim_eta`` must stay 0), ``--top_p`` truncates every step's noise, and ``--mbr K`` decodes K candidates per source
and writes their minimum-Bayes-risk pick (``--keep_candidates true``: all of them too; the pick of
a whole batch is one n-gram match kernel on the device, ``utils.mbr.mbr_select_batch``;
``--mbr_metric rouge_l`` picks by ROUGE-L instead of BLEU, on one LCS kernel).  With
``--noise philox`` the noise is keyed by (seed + candidate, step, index of the sample in the split,
position) instead: the output no longer depends on ``batch_size``, ``--mbr K --seed s`` gives the
candidates that K runs with ``--mbr 1`` and the seeds s .. s + K - 1 give, and on a GPU each
reverse update outside the model is one fused kernel.
"""
import json
import os
import re

from config.sample import SampleSettings


def create_parser():
    return SampleSettings.to_argparse(add_json=True)


def find_checkpoint(model_path, use_ema=""):
    """``model_path`` itself when it is a file; else the newest ``ema_<use_ema>_NNNNNN.pt``
    (``use_ema`` set; rates compare as numbers) or ``model_NNNNNN.pt`` of that directory."""
    if os.path.isfile(model_path):
        return model_path
    if not os.path.isdir(model_path):
        raise FileNotFoundError(f"model_path {model_path!r} is neither a file nor a directory")
    best = None
    for name in os.listdir(model_path):
        if use_ema:
            m = re.fullmatch(r"ema_(.+)_(\d+)\.pt", name)
            try:
                ok = m is not None and float(m.group(1)) == float(use_ema)
            except ValueError:
                ok = False
        else:
            m = re.fullmatch(r"model_?(\d+)\.pt", name)
            ok = m is not None
        if ok and (best is None or int(m.groups()[-1]) > best[0]):
            best = (int(m.groups()[-1]), name)
    if best is None:
        what = f"ema_{use_ema}_NNNNNN.pt" if use_ema else "model_NNNNNN.pt"
        raise FileNotFoundError(f"no {what} in {model_path!r}")
    return os.path.join(model_path, best[1])


def shadow_frozen_weights(model):
    """Frozen weights: one bf16 cast per parameter, not one per forward (ops.shadow)."""
    import torch

    for p in model.parameters():
        p._dpa_shadow = p.detach().to(torch.bfloat16)


def load_vocab(data_dir):
    """id -> token of ``{data_dir}/vocab.txt`` (the WordPiece file the dataset's tokenizer reads),
    or None."""
    path = os.path.join(data_dir, "vocab.txt")
    if not os.path.exists(path):
        return None
    with open(path, encoding="utf-8") as f:
        return [line.rstrip("\n") for line in f]


def detokenize(ids, vocab):
    words = []
    for i in ids:
        tok = vocab[i] if 0 <= i < len(vocab) else "[UNK]"
        if tok.startswith("##") and words:
            words[-1] += tok[2:]
        else:
            words.append(tok)
    return " ".join(words)


def split_sample(ids, mask, recovered, pad_id=0):
    """(source, reference, recover) id lists of one sample: ``mask`` is 0 on the source and 1 on
    the target and the padding after it; padding (trailing ``pad_id``) is stripped - from the
    recovered target wherever the model put its first pad."""
    n_src = int((mask == 0).sum())
    source = ids[:n_src].tolist()
    reference = ids[n_src:].tolist()
    while reference and reference[-1] == pad_id:
        reference.pop()
    recover = recovered[n_src:].tolist()
    if pad_id in recover:
        recover = recover[:recover.index(pad_id)]
    return source, reference, recover


def recover_parts(recs, mask, pad_id=0):
    """The ``recover`` parts of K decoded ``[B, L]`` id tensors as one padded batch, with tensor
    ops on their device: -> (tokens [B, K, L], lens [B, K]) where ``tokens[b, k, :lens[b, k]]`` is
    what :func:`split_sample` returns for sample b of candidate k - the ids after the source
    (``mask`` == 0) up to the first ``pad_id``."""
    import torch

    rec = torch.stack(list(recs), 1)                                   # [B, K, L]
    L = rec.shape[-1]
    at = (mask == 0).sum(1).view(-1, 1, 1) + torch.arange(L, device=rec.device)  # position in rec
    inside = at < L
    tokens = rec.gather(2, at.clamp(max=L - 1).expand(rec.shape))
    live = (inside & (tokens != pad_id)).to(torch.int32)
    lens = live.cumprod(-1).sum(-1)                                    # tokens before the first pad
    return tokens, lens


def main(namespace):
    args: SampleSettings = SampleSettings.from_argparse(namespace)
    if args.sampler.startswith("dpmpp_2m") and args.ddim_eta != 0.0:
        raise ValueError(f"--ddim_eta {args.ddim_eta} does not apply to --sampler {args.sampler}: leave it at 0")

    import torch

    from basic_utils import dist_util
    from data import load_data_from_args
    from data.dataset import PAD_ID
    from utils.initialization import create_diffusion_from_config, create_model_from_config
    from utils.mbr import mbr_select_batch

    if args.model != "diffuseq":
        raise ValueError(f"run.sample decodes the diffuseq model, not {args.model!r}")
    dev = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda":
        torch.cuda.set_device(dev)

    model = create_model_from_config(**args.dict())
    diffusion, _ = create_diffusion_from_config(**args.dict())
    ckpt = find_checkpoint(args.model_path, args.use_ema)
    print(f"### loading {ckpt}")
    model.load_state_dict(dist_util.load_state_dict(ckpt, map_location="cpu"))
    model.to(dev).eval()
    if args.precision == "bf16":
        shadow_frozen_weights(model)

    data = load_data_from_args(split=args.split, data_dir=args.data_dir, batch_size=args.batch_size,
                               deterministic=True, loop=False, num_loader_proc=0,
                               dataset=args.dataset, seq_len=args.seq_len, vocab_size=args.vocab_size,
                               seed=args.seed, model=args.model)
    vocab = load_vocab(args.data_dir)
    out_path = args.out_path
    if not out_path:
        stem = os.path.splitext(os.path.basename(ckpt))[0]
        out_path = os.path.join(os.path.dirname(os.path.abspath(ckpt)), f"samples_{stem}_seed{args.seed}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    clamp_step = None if args.clamp_step < 0 else args.clamp_step
    if args.mbr < 1:
        raise ValueError(f"--mbr must be >= 1, got {args.mbr}")
    chain = dict(steps=args.step or None, sampler=args.sampler, eta=args.ddim_eta, top_p=args.top_p)
    n = 0
    with open(out_path, "w") as fout:
        for b, batch in enumerate(data):
            if b >= args.num_batches:
                break
            batch = {k: v.to(dev) for k, v in batch.items()}
            recs = []
            for c in range(args.mbr):
                if args.noise == "philox":  # candidate c is what seed + c alone decodes; n: first sample's index
                    out = diffusion.sample_seq2seq(model, batch, clamp_step=clamp_step, noise_seed=args.seed + c,
                                                   row_base=n, **chain)
                else:
                    out = diffusion.sample_seq2seq(model, batch, clamp_step=clamp_step, generator=gen, **chain)
                recs.append(out["tokens"])
            picks = None
            if args.mbr > 1:  # the candidates stay on the device: one n-gram match kernel, one copy
                picks = mbr_select_batch(*recover_parts(recs, batch["input_mask"], PAD_ID), metric=args.mbr_metric)
            recs = [rec.cpu() for rec in recs]
            ids, mask = batch["input_ids"].cpu(), batch["input_mask"].cpu()
            for i in range(ids.shape[0]):
                cands = [split_sample(ids[i], mask[i], rec[i], PAD_ID) for rec in recs]
                src, ref = cands[0][:2]
                hyps = [cand[2] for cand in cands]
                hyp = hyps[picks[i] if picks is not None else 0]
                line = {"source": src, "reference": ref, "recover": hyp}
                if args.keep_candidates:
                    line["candidates"] = hyps
                if vocab is not None:
                    line.update(source_text=detokenize(src, vocab), reference_text=detokenize(ref, vocab),
                                recover_text=detokenize(hyp, vocab))
                fout.write(json.dumps(line) + "\n")
            n += ids.shape[0]
    print(f"### wrote {n} samples to {out_path}")
    return out_path


if __name__ == "__main__":
    main(create_parser().parse_args())
