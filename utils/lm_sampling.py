"""
Next-token choice from a language model's logits (plain PyTorch on the ``[B, V]`` logits; used by
``GPT2LMModel.generate``).

``temperature == 0`` is greedy: the arg-max, equal maxima going to the lowest id (the tie rule of
``ops.nn.linear_argmax``; ``torch.argmax`` documents no tie order).  Otherwise the logits are
divided by ``temperature``, filtered by ``top_k`` and then ``top_p``, and one id per row is drawn
from the softmax of what is left, with ``generator``.
"""
import torch


def greedy(logits):
    """Arg-max over the last dimension, ties to the lowest id; NaN logits never win."""
    V = logits.shape[-1]
    s = torch.where(torch.isnan(logits), float("-inf"), logits.float())
    m = s.amax(-1, keepdim=True)
    ar = torch.arange(V, device=logits.device)
    return torch.where(s == m, ar, V).amin(-1).clamp(max=V - 1)


def filter_top_k(logits, top_k):
    """Keep each row's ``top_k`` largest logits and everything equal to the k-th kept; the rest
    become -inf.  ``top_k <= 0`` or ``>= V``: unchanged."""
    if top_k <= 0 or top_k >= logits.shape[-1]:
        return logits
    kth = torch.topk(logits, int(top_k), dim=-1).values[..., -1:]
    return logits.masked_fill(logits < kth, float("-inf"))


def filter_top_p(logits, top_p):
    """Nucleus filter: in descending order keep the smallest prefix whose probability mass reaches
    ``top_p`` (never fewer than one id); the rest become -inf.  ``top_p <= 0``: unchanged."""
    if top_p <= 0.0:
        return logits
    srt, order = torch.sort(logits.float(), dim=-1, descending=True, stable=True)
    probs = torch.softmax(srt, -1)
    before = probs.cumsum(-1) - probs      # mass of the ids in front of each one
    drop_sorted = before >= top_p          # the prefix in front already reaches top_p
    drop_sorted[..., 0] = False
    drop = torch.zeros_like(drop_sorted).scatter_(-1, order, drop_sorted)
    return logits.masked_fill(drop, float("-inf"))


def filter_logits(logits, top_k=0, top_p=0.0):
    """``top_k`` first, then ``top_p`` on what it kept."""
    return filter_top_p(filter_top_k(logits, top_k), top_p)


def sample_next(logits, temperature=1.0, top_k=0, top_p=0.0, generator=None):
    """One id per row of ``logits`` [B, V] -> int64 [B]."""
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if not 0.0 <= top_p <= 1.0:
        raise ValueError(f"top_p must be in [0, 1], got {top_p}")
    if temperature == 0:
        return greedy(logits)
    kept = filter_logits(logits.float() / temperature, top_k, top_p)
    return torch.multinomial(torch.softmax(kept, -1), 1, generator=generator).squeeze(-1)
