"""
Decoding settings (L4) for ``python -m run.sample``.

The model, diffusion and data groups are the training ones, so the ``training_args.json`` a
training run writes next to its checkpoints is a valid ``--config_json`` here: keys that only
training reads (``TrainSettings`` fields that are not fields of ``SampleSettings``, e.g. ``lr`` or
``microbatch``) are dropped, anything else unknown is still rejected.  Flags given on the command
line are applied on top of the JSON, as for training.  ``batch_size`` and ``seed`` are shared
names: unless overridden, a training config's values are used for decoding too.
"""
import json
import sys
from typing import final
from argparse import ArgumentParser as Ap, ArgumentDefaultsHelpFormatter as Df

from .base import S, Choice, Item as _
from .train import DataSettings, DiffusionSettings, ModelSettings, TrainSettings


class DecodeSettings(S):
    model_path: str \
        = _("", "Checkpoint file, or a checkpoint directory: its newest ema_<use_ema>_NNNNNN.pt if use_ema "
                "is set, else its newest model_NNNNNN.pt.")
    use_ema: str \
        = _("", "EMA rate (e.g. 0.9999) whose weights to decode with when model_path is a directory.")
    split: str \
        = _("test", "Dataset split to decode.")
    batch_size: int \
        = _(64, "Batch size per decode step.")
    num_batches: int \
        = _(1, "Batches to decode.")
    clamp_step: int \
        = _(-1, "Round the predicted x0 to its nearest word embedding at the reverse steps t <= clamp_step; "
                "-1 = at every step.")
    step: int \
        = _(0, "Reverse steps of the respaced chain (2 .. diffusion_steps); 0 = all diffusion_steps.")
    sampler: Choice("ancestral", "ddim", "dpmpp_2m", "dpmpp_2m_sde") \
        = _("ancestral", "Reverse update: ancestral (DDPM posterior), ddim, or the second-order multistep "
                         "DPM-Solver++ (dpmpp_2m: deterministic; dpmpp_2m_sde: with noise), which reuses the "
                         "previous step's prediction.")
    ddim_eta: float \
        = _(0.0, "DDIM eta (0 = deterministic updates, 1 = the ancestral posterior variance); must be 0 with "
                 "the dpmpp samplers.")
    top_p: float \
        = _(0.0, "Truncate every step's noise to [-top_p, top_p] (DiffuSeq --top_p); 0 = off.")
    mbr: int \
        = _(1, "Candidates decoded per source; recover is their minimum-Bayes-risk pick (utils/mbr.py).")
    mbr_metric: Choice("bleu", "rouge_l") \
        = _("bleu", "Similarity the minimum-Bayes-risk pick sums over the other candidates: sentence BLEU "
                    "(utils/mbr.py) or ROUGE-L (utils/rouge.py).")
    noise: Choice("torch", "philox") \
        = _("torch", "torch: one torch.Generator seeded with seed (the output depends on the batching). "
                     "philox: counter-based noise keyed by (seed + candidate, step, sample index in the split, "
                     "position), so the output does not depend on the batching; on a GPU the reverse update "
                     "is then one fused kernel per step.")
    keep_candidates: bool \
        = _(False, "Also write every candidate's ids as `candidates` to each output row.")
    seed: int \
        = _(102, "Sampling seed.")
    out_path: str \
        = _("", "Output .jsonl file (default: samples_<checkpoint>_seed<seed>.jsonl next to the checkpoint).")
    precision: Choice("bf16", "fp32") \
        = _("bf16", "Compute precision the model was trained with.")
    use_hip_kernels: bool \
        = _(True, "Use the hand-written gfx950 kernels (required on GPU).")


@final
class SampleSettings(
        DecodeSettings,
        DiffusionSettings,
        ModelSettings,
        DataSettings
):

    @classmethod
    def to_argparse(cls, parser_or_group=None, add_json=False):
        if not add_json:
            return super(SampleSettings, cls).to_argparse(parser_or_group)
        if parser_or_group is None:
            parser_or_group = Ap(formatter_class=Df)
        setting_group = parser_or_group.add_argument_group(title="settings")
        setting_group.add_argument(
            "--config_json", type=str, required=False,
            help="Load settings from this JSON file (a training config works); flags given explicitly "
                 "override it.")
        super(SampleSettings, cls).to_argparse(setting_group, _suppress_defaults=True)
        return parser_or_group

    @classmethod
    def from_argparse(cls, namespace, _top=True):
        ns = dict(vars(namespace)) if not isinstance(namespace, dict) else dict(namespace)
        cfg = ns.pop("config_json", None)
        overrides = {k: v for k, v in ns.items() if k in cls.model_fields}
        unknown = set(ns) - set(overrides)
        assert not (_top and unknown), str(unknown)
        if not cfg:
            return cls(**overrides)
        with open(cfg, "r") as f:
            data = json.load(f)
        train_only = set(TrainSettings.model_fields) - set(cls.model_fields)
        data = {k: v for k, v in data.items() if k not in train_only}
        if overrides:
            print(f"<INFO> --config_json {cfg}: overriding {sorted(overrides)} from the command line",
                  file=sys.stderr)
        data.update(overrides)
        return cls(**data)


__all__ = ('SampleSettings', 'DecodeSettings')
