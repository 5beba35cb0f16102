"""
Diversity metrics on token ids (the dist-n and div-4 columns of the DiffuSeq paper):

* dist-n of one sequence: distinct n-grams / n-grams (dist-1 is the ``dist1`` of ``run.eval``);
* div-n of the candidates decoded for one source: distinct n-grams of their union / the sum of
  their n-gram totals (DiffuSeq's ``distinct_n_gram_inter_sent``) - higher is more diverse.

``distinct_ngrams`` / ``dist_n`` / ``div_n`` work on token-id lists in pure Python sets.
``dist_n_batch`` and ``div_n_batch`` take the sequences of many groups as one padded tensor: the
distinct counts come from one ``ops.text.ngram_distinct`` call (a kernel on a GPU).  The counts are
exact integers and every value is one IEEE double division of two of them, as in the list versions,
so both give the same numbers bit for bit.

One deliberate difference from DiffuSeq's evaluation script: its per-sentence ``distinct_n_gram``
returns 0 for the whole file as soon as one hypothesis has no n-gram.  Here such a sequence has
``dist_n == 0.0`` and contributes that 0 to a mean, as ``dist1`` of ``run.eval`` already does for
an empty row.
"""


def _total(length, n):
    return max(length - n + 1, 0)


def distinct_ngrams(seq, n):
    """Number of distinct n-grams of the sequence ``seq``: the size of the set of its n-gram tuples."""
    seq = list(seq)
    return len({tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)})


def dist_n(seq, n):
    """distinct n-grams / n-grams of ``seq`` (``max(len - n + 1, 0)`` of them); 0.0 without an n-gram."""
    seq = list(seq)
    total = _total(len(seq), n)
    return distinct_ngrams(seq, n) / total if total else 0.0


def div_n(cands, n):
    """Size of the union of the candidates' n-gram sets / the sum of their n-gram totals; 0.0 when
    no candidate has an n-gram."""
    cands = [list(c) for c in cands]
    total = sum(_total(len(c), n) for c in cands)
    union = set()
    for c in cands:
        union.update(tuple(c[i:i + n]) for i in range(len(c) - n + 1))
    return len(union) / total if total else 0.0


def _counts_and_totals(tokens, lens):
    """(d float64 [G, K + 1, 4], t float64 [G, K, 4]) on the CPU: the distinct counts of one
    ``ngram_distinct`` call and the n-gram totals ``max(len - n + 1, 0)``, both exact integers."""
    import torch

    from distributed_pipeline_amd.ops.text import ngram_distinct

    L = tokens.shape[2]
    lens = lens.to(tokens.device).clamp(0, L)
    d = ngram_distinct(tokens, lens).cpu().to(torch.float64)
    n = torch.arange(1, 5).view(1, 1, 4)
    t = (lens.cpu().to(torch.int64).unsqueeze(-1) - n + 1).clamp_min(0).to(torch.float64)
    return d, t


def _ratio(num, den):
    import torch

    return torch.where(den > 0, num / den.clamp_min(1.0), torch.zeros_like(num))


def dist_n_batch(tokens, lens):
    """``tokens`` [G, K, L] ids, ``lens`` [G, K] -> float64 [G, K, 4] on the CPU with
    ``[g, k, n - 1] = dist_n(sequence k of group g, n)``, bit for bit: the counts are exact
    integers and each value is the one IEEE division the list version makes."""
    d, t = _counts_and_totals(tokens, lens)
    return _ratio(d[:, :-1], t)


def div_n_batch(tokens, lens):
    """``tokens`` [G, K, L] ids, ``lens`` [G, K] -> float64 [G, 4] on the CPU with
    ``[g, n - 1] = div_n(the K sequences of group g, n)``, bit for bit: the counts are exact
    integers and each value is the one IEEE division the list version makes."""
    d, t = _counts_and_totals(tokens, lens)
    return _ratio(d[:, -1], t.sum(1))


__all__ = ('distinct_ngrams', 'dist_n', 'div_n', 'dist_n_batch', 'div_n_batch')
