"""
Entry point: ``python -m run.generate --config_json cfg.json --model_path DIR --out_path out.jsonl``

Continues prompts with a trained GPT-2 checkpoint (one process; one GPU, or the CPU): settings ->
model -> state dict -> ``eval()`` -> for each batch of the split the first ``prompt_len`` tokens
of every ``input_ids`` row are the prompt, and ``GPT2LMModel.generate`` adds up to
``max_new_tokens`` tokens through its K/V cache (one prefill forward, then one single-token
decode step per new token) -> one JSON line per row with ``prompt``, ``continuation`` (cut at the
first ``eos_id``) and ``reference`` (the row's own next ``max_new_tokens`` tokens), as id lists.

``--config_json`` takes the ``training_args.json`` of the training run as it is
(config/generate.py).  ``--temperature 0`` is greedy and ignores the seed; otherwise
``--temperature``, ``--top_k`` and ``--top_p`` shape the draw and ``--seed`` reproduces it.
``--noise philox`` draws with ``ops.decode.sample_tokens``: noise keyed by (seed, step, the row's
index in the split, token id), so a row's draws do not depend on ``--batch_size``.

``--num_beams W`` (W > 1) runs ``GPT2LMModel.beam_search`` instead: ``continuation`` is the best of W
beams by ``score / length ** length_penalty``, and ``--keep_beams true`` adds ``beams`` (every beam's
ids, best first) and ``beam_scores`` (their summed log-probabilities).  The search is deterministic:
it ignores ``--temperature`` and ``--seed`` and excludes ``--top_k``, ``--top_p`` and ``--noise philox``.

``--lookahead T`` (2 .. 8, with ``--temperature 0``) runs ``GPT2LMModel.generate_lookahead``: greedy
decoding's own output, T tokens per model call - the last one and T - 1 guesses copied from behind the
latest earlier occurrence of the row's last ``--lookup_ngram`` tokens - of which the verified prefix is
kept.  The run prints the model calls it made and how many guesses were accepted.

``--repetition_penalty``, ``--presence_penalty``, ``--frequency_penalty`` and ``--no_repeat_ngram`` keep a
continuation from repeating itself: every step's logits go through ``ops.decode.penalize_logits_`` (one
kernel on a GPU) before the token is chosen, over the prompt and the tokens generated so far, or with
``--penalize_prompt false`` over the generated tokens alone.  ``--min_new_tokens M`` holds ``--eos_id`` off
for the first M tokens.  They combine with sampling, ``--noise philox`` and ``--num_beams`` and exclude
``--lookahead``.

``--logprobs true`` adds ``logprobs`` to each line, cut like ``continuation``: every token's log-probability
under its step's logits after the penalties and before temperature, ``--top_k`` and ``--top_p``
(``GPT2LMModel.generate(return_logprobs=True)``; ``python -m run.score --path`` gives the same numbers from a
teacher-forced forward when no penalty is set).  It excludes ``--num_beams > 1`` and ``--lookahead``.

``--kv_dtype fp8`` keeps the K/V cache in one byte per element - OCP e4m3fn codes and one power-of-two
exponent per cached row (``ops.decode`` has the format): half the cache memory and half the bytes every
decode step reads.  Its continuations are those of a slightly different model, not bf16's bit for bit.
It combines with sampling, ``--noise philox``, the penalties and ``--logprobs`` and excludes
``--num_beams > 1`` and ``--lookahead``.  The default is ``bf16``.
"""
import json
import os

from config.generate import GenerateSettings
from run.sample import find_checkpoint, shadow_frozen_weights


def create_parser():
    return GenerateSettings.to_argparse(add_json=True)


def main(namespace):
    args: GenerateSettings = GenerateSettings.from_argparse(namespace)
    args.check()  # the model family and the sampling values, before any checkpoint is read

    import torch

    from basic_utils import dist_util
    from data import load_data_from_args
    from utils.initialization import create_model_from_config

    dev = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda":
        torch.cuda.set_device(dev)

    model = create_model_from_config(**args.dict())
    ckpt = find_checkpoint(args.model_path, args.use_ema)
    print(f"### loading {ckpt}")
    model.load_state_dict(dist_util.load_state_dict(ckpt, map_location="cpu"))
    model.to(dev).eval()
    if args.precision == "bf16":
        shadow_frozen_weights(model)

    # seed=0: ``--seed`` is the sampling seed alone; it must not also pick the prompts (the synthetic
    # dataset draws its tokens from its seed), or a greedy run would depend on it
    data = load_data_from_args(split=args.split, data_dir=args.data_dir, batch_size=args.batch_size,
                               deterministic=True, loop=False, num_loader_proc=0,
                               dataset=args.dataset, seq_len=args.seq_len, vocab_size=args.vocab_size,
                               seed=0, model=args.model)
    out_path = args.out_path
    if not out_path:
        stem = os.path.splitext(os.path.basename(ckpt))[0]
        out_path = os.path.join(os.path.dirname(os.path.abspath(ckpt)), f"generated_{stem}_seed{args.seed}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    eos = None if args.eos_id < 0 else args.eos_id
    Lp, Ln = args.prompt_len, args.max_new_tokens
    n = 0
    look = {"model_calls": 0, "tokens": 0, "proposed": 0, "accepted": 0}
    with open(out_path, "w") as fout:
        for b, batch in enumerate(data):
            if b >= args.num_batches:
                break
            ids = batch["input_ids"].to(dev)
            lens = torch.full((ids.shape[0],), Lp, dtype=torch.int32, device=dev)
            if args.num_beams > 1:
                beams, beam_lens, beam_scores = model.beam_search(
                    ids[:, :Lp].contiguous(), lens, Ln, num_beams=args.num_beams, eos_id=eos,
                    length_penalty=args.length_penalty, **args.logit_processors())
                beams, beam_lens, beam_scores = beams.cpu(), beam_lens.cpu(), beam_scores.cpu()
                toks, new_lens = beams[:, 0], beam_lens[:, 0]
            elif args.lookahead:
                toks, new_lens, stats = model.generate_lookahead(
                    ids[:, :Lp].contiguous(), lens, Ln, lookahead=args.lookahead, ngram=args.lookup_ngram,
                    eos_id=eos, return_stats=True)
                for key, val in stats.items():
                    look[key] += val
                look["tokens"] += int(new_lens.sum())
            else:
                res = model.generate(ids[:, :Lp].contiguous(), lens, Ln, temperature=args.temperature,
                                     top_k=args.top_k, top_p=args.top_p, eos_id=eos, generator=gen,
                                     noise_seed=args.seed if args.noise == "philox" else None, row_base=n,
                                     **args.logit_processors(), **({"return_logprobs": True} if args.logprobs else {}),
                                     **({"kv_dtype": args.kv_dtype} if args.kv_dtype != "bf16" else {}))
                toks, new_lens = res[:2]
                if args.logprobs:
                    logprobs = res[2].cpu()
            ids, toks, new_lens = ids.cpu(), toks.cpu(), new_lens.cpu()

            def cut(row, length):
                cont = row[:int(length)].tolist()
                return cont[:cont.index(eos)] if eos is not None and eos in cont else cont

            for i in range(ids.shape[0]):
                line = {"prompt": ids[i, :Lp].tolist(), "continuation": cut(toks[i], new_lens[i]),
                        "reference": ids[i, Lp:Lp + Ln].tolist()}
                if args.num_beams > 1 and args.keep_beams:
                    # slots that never held a hypothesis (score -inf) are left out
                    live = [w for w in range(args.num_beams) if beam_scores[i, w] > float("-inf")]
                    line["beams"] = [cut(beams[i, w], beam_lens[i, w]) for w in live]
                    line["beam_scores"] = [float(beam_scores[i, w]) for w in live]
                if args.logprobs:
                    line["logprobs"] = [float(x) for x in logprobs[i, :len(line["continuation"])]]
                fout.write(json.dumps(line) + "\n")
            n += ids.shape[0]
    if args.lookahead:
        print(f"### lookahead {args.lookahead}: {look['model_calls']} model calls for {look['tokens']} tokens, "
              f"{look['accepted']} of {look['proposed']} guesses accepted")
    print(f"### wrote {n} continuations to {out_path}")
    return out_path


if __name__ == "__main__":
    main(create_parser().parse_args())
