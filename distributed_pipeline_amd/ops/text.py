"""
Token-sequence ops of decoding and evaluation on the gfx950 kernels of ``csrc/ngram_match.hip``,
``csrc/ngram_distinct.hip`` and ``csrc/lcs.hip``.

* :func:`ngram_matches` - the clipped 1..4-gram match counts between every pair of a group's
  sequences, the quantity sentence BLEU, minimum-Bayes-risk selection and self-BLEU are built on
  (``utils/mbr.py``).  Integers only: the kernel and the PyTorch path give the same tensor.
* :func:`ngram_distinct` - the number of distinct 1..4-grams of every sequence of a group and of
  the group's union, the quantity dist-n and div-n are built on (``utils/diversity.py``).
  Integers only as well.
* :func:`lcs_lengths` - the length of the longest common subsequence of every pair of a group's
  sequences, the quantity ROUGE-L is built on (``utils/rouge.py``).  Integers only as well.
"""
import torch

from ._ext import get_ext

_FALLBACK_ELEMS = 1 << 25  # pairwise comparisons (bools) one chunk of groups may hold


def ngram_matches(tokens, lens):
    """``tokens`` [G, K, L] (int32 / int64, any strides), ``lens`` [G, K] -> int32 [G, K, K, 4]:

        m[g, i, j, n - 1] = sum over the distinct n-grams y of min(count_i(y), count_j(y)),  n = 1..4

    where count_k counts the occurrences of y among the first ``lens[g, k]`` (clamped to [0, L], on
    the device) tokens of sequence k.  Positions at or beyond the length never count, whatever
    they hold; the ids inside the lengths must lie in [0, 2^31).  m is symmetric in (i, j) and its
    diagonal is max(len - n + 1, 0).

    On a HIP device with the extension and a shape the kernel covers (K <= 16, L <= 256) this is one
    kernel; anything else evaluates the same definition in PyTorch, chunked over G."""
    if tokens.dim() != 3 or lens.shape != tokens.shape[:2]:
        raise ValueError(f"ngram_matches: tokens [G, K, L] and lens [G, K], got {tuple(tokens.shape)} "
                         f"and {tuple(lens.shape)}")
    if tokens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ngram_matches: tokens must be int32 or int64, not {tokens.dtype}")
    G, K, L = tokens.shape
    lens = lens.to(tokens.device).clamp(0, L).to(torch.int32).contiguous()
    if tokens.is_cuda:
        ext = get_ext()
        if ext is not None:
            if not hasattr(ext, "ngram_matches"):
                raise RuntimeError("the native extension has no ngram_matches kernel: rebuild it")
            m = ext.ngram_matches(tokens.contiguous(), lens)
            if m is not None:
                return m
    return _ngram_matches_torch(tokens, lens)


def _ngram_matches_torch(tokens, lens):
    """The definition in rank/count form: position p of sequence i is a clipped match against j
    when its n-gram occurs more often in j than it has occurred in i before p."""
    G, K, L = tokens.shape
    out = torch.zeros((G, K, K, 4), dtype=torch.int32, device=tokens.device)
    if G == 0 or K == 0 or L == 0:
        return out
    chunk = max(1, _FALLBACK_ELEMS // (K * K * L * L))
    pos = torch.arange(L, device=tokens.device)
    below = (pos.view(1, L) < pos.view(L, 1)).view(1, 1, L, L)  # [.., p, q]: q < p
    for g0 in range(0, G, chunk):
        tok, ln = tokens[g0:g0 + chunk], lens[g0:g0 + chunk]
        valid = pos.view(1, 1, L) < ln.unsqueeze(-1)                                  # [g, K, L]
        # eq[g, i, p, j, q]: the n-grams at p of i and q of j exist and are equal (n = 1 first)
        one = (tok.view(-1, K, L, 1, 1) == tok.view(-1, 1, 1, K, L)) \
            & valid.view(-1, K, L, 1, 1) & valid.view(-1, 1, 1, K, L)
        eq = one
        for n in range(1, 5):
            if n > 1:
                nxt = torch.zeros_like(one)
                s = n - 1
                if s < L:
                    nxt[:, :, :L - s, :, :L - s] = one[:, :, s:, :, s:]
                eq = eq & nxt
            count = eq.sum(-1, dtype=torch.int32)                                     # [g, i, p, j]
            own = torch.diagonal(eq, dim1=1, dim2=3).permute(0, 3, 1, 2)              # [g, i, p, q]
            rank = (own & below).sum(-1, dtype=torch.int32)                           # [g, i, p]
            out[g0:g0 + chunk, :, :, n - 1] = (count > rank.unsqueeze(-1)).sum(2, dtype=torch.int32)
    return out


def ngram_distinct(tokens, lens):
    """``tokens`` [G, K, L] (int32 / int64, any strides), ``lens`` [G, K] -> int32 [G, K + 1, 4]:

        d[g, k, n - 1], k < K = number of distinct n-grams among the first ``lens[g, k]`` tokens of sequence k
        d[g, K, n - 1]        = number of distinct n-grams in the union of the group's K sequences,  n = 1..4

    with the lengths clamped to [0, L] (on the device).  Positions at or beyond the length never
    count, whatever they hold, and an n-gram that would cross the length does not exist; the ids
    inside the lengths must lie in [0, 2^31).  For K == 1 the union row equals the sequence's.

    On a HIP device with the extension and a shape the kernel covers (K <= 16, L <= 256) this is one
    kernel; anything else evaluates the same definition in PyTorch, chunked over G."""
    if tokens.dim() != 3 or lens.shape != tokens.shape[:2]:
        raise ValueError(f"ngram_distinct: tokens [G, K, L] and lens [G, K], got {tuple(tokens.shape)} "
                         f"and {tuple(lens.shape)}")
    if tokens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ngram_distinct: tokens must be int32 or int64, not {tokens.dtype}")
    G, K, L = tokens.shape
    if G == 0 or K == 0 or L == 0:
        return torch.zeros((G, K + 1, 4), dtype=torch.int32, device=tokens.device)
    lens = lens.to(tokens.device).clamp(0, L).to(torch.int32).contiguous()
    if tokens.is_cuda:
        ext = get_ext()
        if ext is not None:
            if not hasattr(ext, "ngram_distinct"):
                raise RuntimeError("the native extension has no ngram_distinct kernel: rebuild it")
            d = ext.ngram_distinct(tokens.contiguous(), lens)
            if d is not None:
                return d
    return _ngram_distinct_torch(tokens, lens)


def _ngram_distinct_torch(tokens, lens):
    """The definition in first-occurrence form: position p of sequence k holds a new n-gram for the
    sequence when the n-gram exists and no q < p of the sequence holds it, and a new one for the
    union when no position of a sequence k' < k holds it either."""
    G, K, L = tokens.shape
    out = torch.zeros((G, K + 1, 4), dtype=torch.int32, device=tokens.device)
    if G == 0 or K == 0 or L == 0:
        return out
    chunk = max(1, _FALLBACK_ELEMS // (K * K * L * L))
    pos = torch.arange(L, device=tokens.device)
    below = (pos.view(1, L) < pos.view(L, 1)).view(1, 1, L, L)  # [.., p, q]: q < p
    seq = torch.arange(K, device=tokens.device)
    before = (seq.view(1, K) < seq.view(K, 1)).view(1, K, 1, K)  # [.., k, p, j]: j < k
    for g0 in range(0, G, chunk):
        tok, ln = tokens[g0:g0 + chunk], lens[g0:g0 + chunk]
        valid = pos.view(1, 1, L) < ln.unsqueeze(-1)                                  # [g, K, L]
        # eq[g, k, p, j, q]: the n-grams at p of k and q of j exist and are equal (n = 1 first)
        one = (tok.view(-1, K, L, 1, 1) == tok.view(-1, 1, 1, K, L)) \
            & valid.view(-1, K, L, 1, 1) & valid.view(-1, 1, 1, K, L)
        eq = one
        for n in range(1, 5):
            if n > 1:
                nxt = torch.zeros_like(one)
                s = n - 1
                if s < L:
                    nxt[:, :, :L - s, :, :L - s] = one[:, :, s:, :, s:]
                eq = eq & nxt
            exists = pos.view(1, 1, L) + n <= ln.unsqueeze(-1)                        # [g, k, p]
            own = torch.diagonal(eq, dim1=1, dim2=3).permute(0, 3, 1, 2)              # [g, k, p, q]
            fresh = exists & ~(own & below).any(-1)                                   # [g, k, p]
            earlier = (eq.any(-1) & before).any(-1)                                   # [g, k, p]
            out[g0:g0 + chunk, :K, n - 1] = fresh.sum(-1, dtype=torch.int32)
            out[g0:g0 + chunk, K, n - 1] = (fresh & ~earlier).sum((1, 2), dtype=torch.int32)
    return out


def lcs_lengths(tokens, lens):
    """``tokens`` [G, K, L] (int32 / int64, any strides), ``lens`` [G, K] -> int32 [G, K, K]:

        out[g, i, j] = length of the longest common subsequence of the first ``lens[g, i]`` tokens of
                       sequence i and the first ``lens[g, j]`` tokens of sequence j

    with the lengths clamped to [0, L] (on the device).  Positions at or beyond the length never
    match, whatever they hold; the ids inside the lengths must lie in [0, 2^31).  out is symmetric
    in (i, j) and its diagonal is the lengths.

    On a HIP device with the extension and a shape the kernel covers (K <= 16, L <= 256) this is one
    kernel; anything else evaluates the same definition in PyTorch, chunked over G."""
    if tokens.dim() != 3 or lens.shape != tokens.shape[:2]:
        raise ValueError(f"lcs_lengths: tokens [G, K, L] and lens [G, K], got {tuple(tokens.shape)} "
                         f"and {tuple(lens.shape)}")
    if tokens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"lcs_lengths: tokens must be int32 or int64, not {tokens.dtype}")
    G, K, L = tokens.shape
    lens = lens.to(tokens.device).clamp(0, L).to(torch.int32).contiguous()
    if tokens.is_cuda:
        ext = get_ext()
        if ext is not None:
            if not hasattr(ext, "lcs_lengths"):
                raise RuntimeError("the native extension has no lcs_lengths kernel: rebuild it")
            out = ext.lcs_lengths(tokens.contiguous(), lens)
            if out is not None:
                return out
    return _lcs_lengths_torch(tokens, lens)


def _lcs_lengths_torch(tokens, lens):
    """The textbook dynamic programme, one row of it (one position p of sequence i) per step for all
    pairs at once: with prev / cur the rows p and p + 1 over the prefixes of sequence j,
    t[q + 1] = max(prev[q] + eq[q], prev[q + 1]) and cur = the running maximum of t."""
    G, K, L = tokens.shape
    out = torch.zeros((G, K, K), dtype=torch.int32, device=tokens.device)
    if G == 0 or K == 0 or L == 0:
        return out
    chunk = max(1, _FALLBACK_ELEMS // (K * K * (L + 1)))
    pos = torch.arange(L, device=tokens.device)
    for g0 in range(0, G, chunk):
        tok, ln = tokens[g0:g0 + chunk], lens[g0:g0 + chunk]
        g = tok.shape[0]
        valid = pos.view(1, 1, L) < ln.unsqueeze(-1)                                  # [g, K, L]
        prev = torch.zeros((g, K, K, L + 1), dtype=torch.int32, device=tokens.device)  # [g, i, j, q]
        for p in range(int(ln.max())):
            eq = (tok[:, :, p].view(g, K, 1, 1) == tok.view(g, 1, K, L)) \
                & valid[:, :, p].view(g, K, 1, 1) & valid.view(g, 1, K, L)
            t = torch.zeros_like(prev)
            t[..., 1:] = torch.maximum(prev[..., :-1] + eq.to(torch.int32), prev[..., 1:])
            prev = torch.cummax(t, -1).values
        out[g0:g0 + chunk] = prev[..., L]
    return out
