"""
Generation settings (L4) for ``python -m run.generate``.

The model and data groups are the training ones, so the ``training_args.json`` a GPT-2 training
run writes next to its checkpoints is a valid ``--config_json`` here, through the key filtering of
``config/sample.py``: keys that only training reads are dropped, anything else unknown is still
rejected, and flags given on the command line are applied on top of the JSON.
"""
from typing import final
from argparse import ArgumentParser as Ap, ArgumentDefaultsHelpFormatter as Df

from .base import S, Choice, Item as _
from .sample import SampleSettings
from .train import DataSettings, ModelSettings


class ContinueSettings(S):
    model_path: str \
        = _("", "Checkpoint file, or a checkpoint directory: its newest ema_<use_ema>_NNNNNN.pt if use_ema "
                "is set, else its newest model_NNNNNN.pt.")
    use_ema: str \
        = _("", "EMA rate (e.g. 0.9999) whose weights to generate with when model_path is a directory.")
    split: str \
        = _("test", "Dataset split the prompts come from.")
    batch_size: int \
        = _(64, "Prompts per batch.")
    num_batches: int \
        = _(1, "Batches to continue.")
    prompt_len: int \
        = _(32, "Prompt: the first prompt_len tokens of each input_ids row.")
    max_new_tokens: int \
        = _(64, "Tokens to generate per prompt; prompt_len + max_new_tokens <= seq_len.")
    temperature: float \
        = _(1.0, "Softmax temperature; 0 = greedy (arg-max, ties to the lowest id).")
    top_k: int \
        = _(0, "Sample among the k most likely tokens (and ties with the k-th); 0 = off.")
    top_p: float \
        = _(0.0, "Nucleus sampling: the smallest set of most likely tokens whose mass reaches top_p; 0 = off.")
    eos_id: int \
        = _(-1, "Token id that ends a continuation; -1 = none.")
    seed: int \
        = _(102, "Sampling seed.")
    noise: Choice("torch", "philox") \
        = _("torch", "torch: one torch.Generator seeded with seed, consumed in batch order (a continuation "
                     "depends on the batching). philox: counter-based noise keyed by (seed, step, sample index "
                     "in the split, token id), so a row's draws do not depend on the batching; on a GPU the "
                     "choice of the next token is then one fused kernel per step.")
    num_beams: int \
        = _(1, "Beam search with this many beams per prompt (1 = off: greedy or sampling as above). Beam "
               "search ignores temperature and seed, and excludes top_k, top_p and --noise philox.")
    length_penalty: float \
        = _(0.0, "Beam search: the beams of a prompt are ordered by score / length ** length_penalty "
                 "(0 = the raw sum of log-probabilities).")
    keep_beams: bool \
        = _(False, "Beam search: also write 'beams' (every beam's ids, best first) and 'beam_scores'.")
    lookahead: int \
        = _(0, "Lookahead decoding with blocks of this many tokens (2 .. 8; 0 = off): greedy decoding's own "
               "output in fewer model calls. Needs --temperature 0 and excludes --num_beams > 1.")
    lookup_ngram: int \
        = _(2, "Lookahead decoding: a row's guesses continue the latest earlier occurrence of its last "
               "lookup_ngram tokens in its own prompt and output.")
    repetition_penalty: float \
        = _(1.0, "Logits of the ids a row already holds are divided by this if positive and multiplied by it if "
                 "negative (> 1 discourages repeats); 1 = off.")
    presence_penalty: float \
        = _(0.0, "Subtracted once from the logit of every id a row already holds; 0 = off.")
    frequency_penalty: float \
        = _(0.0, "Subtracted from the logit of an id once per occurrence in the row so far; 0 = off.")
    no_repeat_ngram: int \
        = _(0, "Ban every token that would complete an n-gram of this size the row already holds; 0 = off.")
    min_new_tokens: int \
        = _(0, "eos_id cannot be chosen before this many tokens were generated; needs --eos_id.")
    penalize_prompt: bool \
        = _(True, "The penalties and the n-gram ban see the prompt as well as the tokens generated so far; "
                  "false: the generated tokens alone.")
    logprobs: bool \
        = _(False, "Also write 'logprobs': each continuation token's log-probability under the step's logits "
                   "(after the penalties, before temperature, top_k and top_p). Excludes --num_beams > 1 and "
                   "--lookahead.")
    kv_dtype: Choice("bf16", "fp8") \
        = _("bf16", "Storage of the K/V cache. fp8: one byte per element (OCP e4m3fn codes and one power-of-two "
                    "exponent per cached row), half the memory and half the bytes a decode step reads; the "
                    "continuations can differ from bf16's. Excludes --num_beams > 1 and --lookahead.")
    out_path: str \
        = _("", "Output .jsonl file (default: generated_<checkpoint>_seed<seed>.jsonl next to the checkpoint).")
    precision: Choice("bf16", "fp32") \
        = _("bf16", "Compute precision the model was trained with.")
    use_hip_kernels: bool \
        = _(True, "Use the hand-written gfx950 kernels (required on GPU).")


@final
class GenerateSettings(
        ContinueSettings,
        ModelSettings,
        DataSettings
):

    @classmethod
    def to_argparse(cls, parser_or_group=None, add_json=False):
        if not add_json:
            return super(GenerateSettings, cls).to_argparse(parser_or_group)
        if parser_or_group is None:
            parser_or_group = Ap(formatter_class=Df)
        setting_group = parser_or_group.add_argument_group(title="settings")
        setting_group.add_argument(
            "--config_json", type=str, required=False,
            help="Load settings from this JSON file (a training config works); flags given explicitly "
                 "override it.")
        super(GenerateSettings, cls).to_argparse(setting_group, _suppress_defaults=True)
        return parser_or_group

    # the JSON loading and train-only key filtering of run.sample's settings, on this class's fields
    from_argparse = classmethod(SampleSettings.from_argparse.__func__)

    def logit_processors(self):
        """The keywords ``GPT2LMModel.generate`` and ``beam_search`` take for the logit processors."""
        return dict(repetition_penalty=self.repetition_penalty, presence_penalty=self.presence_penalty,
                    frequency_penalty=self.frequency_penalty, no_repeat_ngram=self.no_repeat_ngram,
                    min_new_tokens=self.min_new_tokens, penalize_prompt=self.penalize_prompt)

    def check(self):
        """Reject what no checkpoint could make sense of (before one is read)."""
        if self.model != "gpt2":
            raise ValueError(f"run.generate continues prompts with the gpt2 model, not {self.model!r}")
        if self.noise not in ("torch", "philox"):
            raise ValueError(f"--noise must be torch or philox, got {self.noise!r}")
        if self.kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"--kv_dtype must be bf16 or fp8, got {self.kv_dtype!r}")
        if self.kv_dtype == "fp8" and (self.num_beams > 1 or self.lookahead > 0):
            raise ValueError("--kv_dtype fp8 is served by generate's own loop: the table (--num_beams > 1) and "
                             "block (--lookahead) decode kernels have no fp8 variant")
        if not 0.0 <= self.top_p <= 1.0:
            raise ValueError(f"--top_p must be in [0, 1], got {self.top_p}")
        if self.temperature < 0:
            raise ValueError(f"--temperature must be >= 0, got {self.temperature}")
        if self.top_k < 0:
            raise ValueError(f"--top_k must be >= 0, got {self.top_k}")
        if self.num_beams < 1:
            raise ValueError(f"--num_beams must be >= 1, got {self.num_beams}")
        if self.num_beams > 1:
            if self.num_beams > 255:
                raise ValueError(f"--num_beams must be <= 255 (one byte per cache table entry), got {self.num_beams}")
            if self.top_k != 0 or self.top_p != 0.0 or self.noise == "philox":
                raise ValueError("--num_beams > 1 is a deterministic search: it excludes --top_k, --top_p and "
                                 "--noise philox")
            # the decode attention's grid is rows x heads workgroups, below 2^31
            if self.num_beams * self.batch_size > 0x7FFFFFFF // max(self.num_heads, 64):
                raise ValueError(f"--num_beams {self.num_beams} x --batch_size {self.batch_size} cache rows "
                                 "cannot be addressed")
        if self.lookahead != 0 and not 2 <= self.lookahead <= 8:
            raise ValueError(f"--lookahead must be 0 (off) or in 2 .. 8, got {self.lookahead}")
        if self.lookup_ngram < 1:
            raise ValueError(f"--lookup_ngram must be >= 1, got {self.lookup_ngram}")
        if self.lookahead:
            if self.temperature != 0:
                raise ValueError("--lookahead verifies guesses against the arg-max: it needs --temperature 0")
            if self.num_beams > 1:
                raise ValueError("--lookahead excludes --num_beams > 1")
        if not self.repetition_penalty > 0:
            raise ValueError(f"--repetition_penalty must be > 0, got {self.repetition_penalty}")
        if self.no_repeat_ngram < 0:
            raise ValueError(f"--no_repeat_ngram must be >= 0, got {self.no_repeat_ngram}")
        if not 0 <= self.min_new_tokens <= self.max_new_tokens:
            raise ValueError(f"--min_new_tokens must be in 0 .. --max_new_tokens {self.max_new_tokens}, got "
                             f"{self.min_new_tokens}")
        if self.min_new_tokens > 0 and self.eos_id < 0:
            raise ValueError("--min_new_tokens holds off eos_id: it needs --eos_id")
        if self.lookahead and self.logit_processors() != dict(
                repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0,
                min_new_tokens=0, penalize_prompt=True):
            raise ValueError("--lookahead excludes --repetition_penalty, --presence_penalty, --frequency_penalty, "
                             "--no_repeat_ngram, --min_new_tokens and --penalize_prompt: its guesses continue "
                             "repeated n-grams")
        if self.logprobs and (self.num_beams > 1 or self.lookahead):
            raise ValueError("--logprobs comes from generate's own loop: it excludes --num_beams > 1 (see "
                             "--keep_beams for beam scores) and --lookahead")
        if self.prompt_len < 1 or self.max_new_tokens < 1:
            raise ValueError("--prompt_len and --max_new_tokens must be >= 1")
        if self.prompt_len + self.max_new_tokens > self.seq_len:
            raise ValueError(f"--prompt_len {self.prompt_len} + --max_new_tokens {self.max_new_tokens} exceeds "
                             f"seq_len {self.seq_len}")


__all__ = ('GenerateSettings', 'ContinueSettings')
