"""
Evaluation settings (L4) for ``python -m run.eval``.
"""
from typing import final

from .base import S, Item as _


@final
class EvalSettings(S):
    path: str \
        = _(..., "A .jsonl file written by run.sample: rows with `recover` and `reference` token ids and, "
                 "from --keep_candidates true, `candidates`.")
    batch_size: int \
        = _(4096, "Rows scored per n-gram match call.")
    rouge_l: bool \
        = _(False, "Also report `rouge_l` (mean ROUGE-L of recover against reference) and, for rows with "
                   "candidates, `self_rouge_l`.")
    diversity: bool \
        = _(False, "Also report `dist2`, `dist3`, `dist4` (mean distinct n-grams / n-grams of recover) and, "
                   "for rows with candidates, `div4` (distinct 4-grams of a row's candidates / their 4-grams).")


__all__ = ('EvalSettings',)
