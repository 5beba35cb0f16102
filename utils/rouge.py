"""
ROUGE-L on token ids (the sequence metric of the DiffuSeq paper that needs no downloaded model):
the F-measure of the longest common subsequence (LCS) of a hypothesis and a reference.

``lcs_length`` / ``rouge_l`` work on token-id lists in pure Python.  ``pairwise_rouge_l`` takes the
sequences of many groups as one padded tensor: the LCS lengths of every pair come from one
``ops.text.lcs_lengths`` call (a kernel on a GPU) and only the closed form ``rouge_l_from_lcs`` is
left to the host, in the same Python floats, so both give the same numbers bit for bit.
"""


def lcs_length(a, b):
    """Length of the longest common subsequence of the sequences ``a`` and ``b``: the textbook
    O(|a| |b|) dynamic programme."""
    a, b = list(a), list(b)
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0  # the previous row's entry left of the current column
        for q, y in enumerate(b):
            up = row[q + 1]
            row[q + 1] = diag + 1 if x == y else (up if up >= row[q] else row[q])
            diag = up
    return row[len(b)]


def rouge_l_from_lcs(lcs, len_h, len_r):
    """The closed form of :func:`rouge_l` from the LCS length of a hypothesis of ``len_h`` tokens and
    a reference of ``len_r`` tokens (Python ints): the harmonic mean of precision and recall."""
    if lcs == 0:
        return 0.0
    p = lcs / len_h
    r = lcs / len_r
    return 2 * p * r / (p + r)


def rouge_l(hyp, ref):
    """ROUGE-L F-measure (beta = 1) of ``hyp`` against one ``ref``; 0 when they share no token."""
    hyp, ref = list(hyp), list(ref)
    return rouge_l_from_lcs(lcs_length(hyp, ref), len(hyp), len(ref))


def _lcs_on_host(tokens, lens):
    """(lcs [G][K][K], lens [G][K]) as nested Python lists: one ``lcs_lengths`` call, one copy."""
    from distributed_pipeline_amd.ops.text import lcs_lengths

    L = tokens.shape[2]
    lens = lens.to(tokens.device).clamp(0, L)
    return lcs_lengths(tokens, lens).tolist(), lens.tolist()


def pairwise_rouge_l(tokens, lens):
    """``tokens`` [G, K, L] ids, ``lens`` [G, K] -> float64 [G, K, K] on the CPU with
    ``[g, i, j] = rouge_l(sequence i, sequence j)`` of group g (the same floats)."""
    import torch

    lcs, ln = _lcs_on_host(tokens, lens)
    return torch.tensor([[[rouge_l_from_lcs(cg[i][j], lg[i], lg[j]) for j in range(len(lg))]
                          for i in range(len(lg))] for cg, lg in zip(lcs, ln)],
                        dtype=torch.float64).reshape(tokens.shape[0], tokens.shape[1], tokens.shape[1])


__all__ = ('lcs_length', 'rouge_l', 'rouge_l_from_lcs', 'pairwise_rouge_l')
