"""
Minimum-Bayes-risk selection among decoded candidates (DiffuSeq decodes several candidates per
source and keeps the one closest to all the others).  Pure Python over token-id lists.
"""
import math
from collections import Counter


def _ngrams(seq, n):
    return Counter(tuple(seq[i:i + n]) for i in range(len(seq) - n + 1))


def sentence_bleu(hyp, ref):
    """BLEU-4 of ``hyp`` against one ``ref`` with add-one smoothing on the orders 2-4:
    p_1 = m_1 / t_1, p_n = (m_n + 1) / (t_n + 1) (m_n: clipped n-gram matches, t_n: n-grams of
    the hypothesis), brevity penalty min(1, exp(1 - |ref| / |hyp|)); 0 for an empty hypothesis or
    one without a matching unigram."""
    hyp, ref = list(hyp), list(ref)
    if not hyp:
        return 0.0
    log_p = 0.0
    for n in range(1, 5):
        h, r = _ngrams(hyp, n), _ngrams(ref, n)
        m = sum(min(cnt, r[g]) for g, cnt in h.items())
        t = max(len(hyp) - n + 1, 0)
        if n == 1:
            if m == 0:
                return 0.0
            log_p += math.log(m / t)
        else:
            log_p += math.log((m + 1) / (t + 1))
    bp = min(1.0, math.exp(1.0 - len(ref) / len(hyp)))
    return bp * math.exp(log_p / 4.0)


def mbr_select(cands):
    """Index of the candidate with the highest summed BLEU against the others (ties: lowest)."""
    best, best_score = 0, -1.0
    for i, hyp in enumerate(cands):
        score = sum(sentence_bleu(hyp, ref) for j, ref in enumerate(cands) if j != i)
        if score > best_score:
            best, best_score = i, score
    return best
