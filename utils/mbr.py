"""
Minimum-Bayes-risk selection among decoded candidates (DiffuSeq decodes several candidates per
source and keeps the one closest to all the others).

``sentence_bleu`` / ``mbr_select`` work on token-id lists in pure Python.  ``mbr_select_batch`` and
``pairwise_bleu`` take the candidates of many sources as one padded tensor: the clipped n-gram
match counts of every pair come from one ``ops.text.ngram_matches`` call (a kernel on a GPU) and
only the closed form ``bleu_from_counts`` is left to the host, in the same Python floats, so the
batch pick equals ``mbr_select`` bit for bit.  ``metric="rouge_l"`` selects by ROUGE-L instead
(utils/rouge.py: LCS lengths from one ``ops.text.lcs_lengths`` call), with the same guarantee.
"""
import math
from collections import Counter


def _ngrams(seq, n):
    return Counter(tuple(seq[i:i + n]) for i in range(len(seq) - n + 1))


def bleu_from_counts(m1, m2, m3, m4, len_h, len_r):
    """The closed form of :func:`sentence_bleu` from the clipped 1..4-gram matches ``m_n`` of a
    hypothesis of ``len_h`` tokens against a reference of ``len_r`` tokens (Python ints)."""
    if len_h <= 0 or m1 == 0:
        return 0.0
    log_p = 0.0 + math.log(m1 / len_h)
    for n, m in ((2, m2), (3, m3), (4, m4)):
        t = max(len_h - n + 1, 0)
        log_p += math.log((m + 1) / (t + 1))
    bp = min(1.0, math.exp(1.0 - len_r / len_h))
    return bp * math.exp(log_p / 4.0)


def sentence_bleu(hyp, ref):
    """BLEU-4 of ``hyp`` against one ``ref`` with add-one smoothing on the orders 2-4:
    p_1 = m_1 / t_1, p_n = (m_n + 1) / (t_n + 1) (m_n: clipped n-gram matches, t_n: n-grams of
    the hypothesis), brevity penalty min(1, exp(1 - |ref| / |hyp|)); 0 for an empty hypothesis or
    one without a matching unigram."""
    hyp, ref = list(hyp), list(ref)
    if not hyp:
        return 0.0
    m = []
    for n in range(1, 5):
        h, r = _ngrams(hyp, n), _ngrams(ref, n)
        m.append(sum(min(cnt, r[g]) for g, cnt in h.items()))
    return bleu_from_counts(m[0], m[1], m[2], m[3], len(hyp), len(ref))


METRICS = ("bleu", "rouge_l")


def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError(f"unknown MBR metric {metric!r}: one of {', '.join(METRICS)}")


def mbr_select(cands, metric="bleu"):
    """Index of the candidate with the highest summed ``metric`` (``bleu``: :func:`sentence_bleu`,
    ``rouge_l``: ``utils.rouge.rouge_l``) against the others (ties: lowest)."""
    _check_metric(metric)
    if metric == "rouge_l":
        from utils.rouge import rouge_l as pair_score
    else:
        pair_score = sentence_bleu
    best, best_score = 0, -1.0
    for i, hyp in enumerate(cands):
        score = sum(pair_score(hyp, ref) for j, ref in enumerate(cands) if j != i)
        if score > best_score:
            best, best_score = i, score
    return best


def _counts_on_host(tokens, lens):
    """(m [G][K][K][4], lens [G][K]) as nested Python lists: one ``ngram_matches`` call, one copy."""
    from distributed_pipeline_amd.ops.text import ngram_matches

    L = tokens.shape[2]
    lens = lens.to(tokens.device).clamp(0, L)
    m = ngram_matches(tokens, lens)
    return m.tolist(), lens.tolist()


def pairwise_bleu(tokens, lens):
    """``tokens`` [G, K, L] ids, ``lens`` [G, K] -> float64 [G, K, K] on the CPU with
    ``[g, i, j] = sentence_bleu(candidate i, candidate j)`` of group g (the same floats)."""
    import torch

    m, ln = _counts_on_host(tokens, lens)
    return torch.tensor([[[bleu_from_counts(*mg[i][j], lg[i], lg[j]) for j in range(len(lg))]
                          for i in range(len(lg))] for mg, lg in zip(m, ln)],
                        dtype=torch.float64).reshape(tokens.shape[0], tokens.shape[1], tokens.shape[1])


def mbr_select_batch(tokens, lens, metric="bleu"):
    """:func:`mbr_select` of every group of ``tokens`` [G, K, L] (candidate k of group g: its first
    ``lens[g, k]`` ids) -> list of G indices, equal to the Python picks, ties included: the same
    BLEU (``metric="rouge_l"``: ROUGE-L, from one ``ops.text.lcs_lengths`` call) floats summed over
    j in the same order, first maximum wins."""
    _check_metric(metric)
    picks = []
    if metric == "rouge_l":
        from utils.rouge import _lcs_on_host, rouge_l_from_lcs

        for cg, lg in zip(*_lcs_on_host(tokens, lens)):
            best, best_score = 0, -1.0
            for i, li in enumerate(lg):
                score = sum(rouge_l_from_lcs(cg[i][j], li, lj) for j, lj in enumerate(lg) if j != i)
                if score > best_score:
                    best, best_score = i, score
            picks.append(best)
        return picks
    m, ln = _counts_on_host(tokens, lens)
    for mg, lg in zip(m, ln):
        best, best_score = 0, -1.0
        for i, li in enumerate(lg):
            score = sum(bleu_from_counts(*mg[i][j], li, lj) for j, lj in enumerate(lg) if j != i)
            if score > best_score:
                best, best_score = i, score
        picks.append(best)
    return picks
