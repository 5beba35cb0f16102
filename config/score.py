"""
Scoring settings (L4) for ``python -m run.score``.

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


class TeacherForcedSettings(S):
    model_path: str \
        = _("", "Checkpoint file, or a checkpoint directory: its newest ema_<use_ema>_NNNNNN.pt if use_ema "
                "is set, else its newest model_NNNNNN.pt.")
    use_ema: str \
        = _("", "EMA rate (e.g. 0.9999) whose weights to score with when model_path is a directory.")
    split: str \
        = _("test", "Dataset split whose input_ids rows are scored (not with --path).")
    batch_size: int \
        = _(64, "Rows per batch.")
    num_batches: int \
        = _(1, "Batches of the split to score (not with --path: a file is scored whole).")
    prompt_len: int \
        = _(1, "Split rows are scored from this position on (1 .. seq_len - 1); the tokens in front are "
               "context only.")
    path: str \
        = _("", "A run.generate .jsonl file to score instead of the split: each row is prompt + <field>, "
                "scored from len(prompt) on.")
    field: str \
        = _("continuation", "With --path: the id list that follows the prompt, continuation or reference.")
    out_path: str \
        = _("", "Write one JSON line per row (tokens, nll, ppl, top1_acc, mean_rank, mean_entropy) here.")
    keep_tokens: bool \
        = _(False, "Also write every scored token's log-probability and rank as `logprobs` and `ranks`.")
    precision: Choice("bf16", "fp32") \
        = _("bf16", "Compute precision the model was trained with.")
    use_hip_kernels: bool \
        = _(True, "Use the hand-written gfx950 kernels (required on GPU).")


@final
class ScoreSettings(
        TeacherForcedSettings,
        ModelSettings,
        DataSettings
):

    @classmethod
    def to_argparse(cls, parser_or_group=None, add_json=False):
        if not add_json:
            return super(ScoreSettings, cls).to_argparse(parser_or_group)
        if parser_or_group is None:
            parser_or_group = Ap(formatter_class=Df)
        setting_group = parser_or_group.add_argument_group(title="settings")
        setting_group.add_argument(
            "--config_json", type=str, required=False,
            help="Load settings from this JSON file (a training config works); flags given explicitly "
                 "override it.")
        super(ScoreSettings, cls).to_argparse(setting_group, _suppress_defaults=True)
        return parser_or_group

    # the JSON loading and train-only key filtering of run.sample's settings, on this class's fields
    from_argparse = classmethod(SampleSettings.from_argparse.__func__)

    def check(self):
        """Reject what no checkpoint could make sense of (before one is read)."""
        if self.model != "gpt2":
            raise ValueError(f"run.score scores tokens with the gpt2 model, not {self.model!r}")
        if self.field not in ("continuation", "reference"):
            raise ValueError(f"--field must be continuation or reference, got {self.field!r}")
        if not 1 <= self.prompt_len <= self.seq_len - 1:
            raise ValueError(f"--prompt_len must be in 1 .. seq_len - 1 = {self.seq_len - 1}, got {self.prompt_len}")
        if self.batch_size < 1 or self.num_batches < 1:
            raise ValueError("--batch_size and --num_batches must be >= 1")
        if self.path:
            defaults = type(self).model_fields
            if self.split != defaults["split"].default or self.prompt_len != defaults["prompt_len"].default:
                raise ValueError("--path scores a file: it excludes --split and --prompt_len")


__all__ = ('ScoreSettings', 'TeacherForcedSettings')
