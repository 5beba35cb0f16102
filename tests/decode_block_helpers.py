"""Shared by the lookahead-decoding tests: the float64 definition of
``ops.decode.attention_decode_block``, a list implementation of ``lookup_draft``, an oracle draft
function, and ``generate_lookahead`` written out row by row in plain Python."""
import torch

from decode_helpers import ref64
from utils.lm_sampling import greedy


def block_counts(lens, counts, T, Lmax):
    """c_b of the definition, as a list."""
    counts = [T] * len(lens) if counts is None else list(counts)
    return [max(0, min(c, T, Lmax - n)) if 0 <= n < Lmax else 0 for n, c in zip(lens, counts)]


def ref64_block(qkv_new, k_cache, v_cache, lens, H, counts=None):
    """float64 [B, T, H*D]: ``ref64`` query by query, on copies of the caches that already hold the
    earlier rows of the block.  ``lens`` / ``counts``: lists.  Nothing is modified."""
    B, T, _ = qkv_new.shape
    Lmax, D = k_cache.shape[2], k_cache.shape[3]
    c = block_counts(lens, counts, T, Lmax)
    kc, vc = k_cache.clone(), v_cache.clone()
    new = qkv_new.view(B, T, 3, H, D)
    outs = []
    for j in range(T):
        lj = [n + j if j < c[b] else -1 for b, n in enumerate(lens)]
        outs.append(ref64(qkv_new[:, j], kc, vc, torch.tensor(lj, dtype=torch.int32, device=qkv_new.device), H))
        for b, n in enumerate(lj):
            if n >= 0:
                kc[b, :, n], vc[b, :, n] = new[b, j, 1].to(kc.dtype), new[b, j, 2].to(vc.dtype)
    return torch.stack(outs, 1)


def list_lookup(s, n, g, M):
    """``lookup_draft`` for one row on lists -> (draft list of M, k)."""
    n = max(0, min(int(n), len(s)))
    s = list(s[:n])
    for i in range(n - g - 1, -1, -1):
        if s[i:i + g] == s[n - g:n]:
            out = list(s)
            for m in range(M):  # a copy that may run into its own output
                out.append(out[i + g + m])
            return out[n:], M
    return [0] * M, 0


def lookup_lists(history, n, *, ngram, max_draft):
    """``lookup_draft``'s signature on top of ``list_lookup``."""
    rows = [list_lookup(h, m, ngram, max_draft) for h, m in zip(history.tolist(), n.tolist())]
    dev = history.device
    return (torch.tensor([r[0] for r in rows], dtype=torch.long, device=dev).view(len(rows), max_draft),
            torch.tensor([r[1] for r in rows], dtype=torch.long, device=dev))


def oracle_draft(cont, plens, vocab, corrupt=None):
    """A draft function that hands out the given continuation ``cont`` [B, N] (row b's output so far
    is ``n[b] - plens[b]`` tokens long), always ``max_draft`` guesses.  ``corrupt``: bool [B, N], the
    output positions whose guess is replaced by a wrong id."""
    B, N = cont.shape
    plens = torch.as_tensor(plens, dtype=torch.long, device=cont.device)

    def draft(history, n, *, ngram, max_draft):
        at = (n.long() - plens).view(B, 1) + torch.arange(max_draft, device=cont.device).view(1, max_draft)
        tok = cont.gather(1, at.clamp(0, N - 1))
        if corrupt is not None:
            tok = torch.where(corrupt.gather(1, at.clamp(0, N - 1)), (tok + 1) % vocab, tok)
        tok = torch.where((at >= 0) & (at < N), tok, 0)
        return tok, torch.full((B,), max_draft, dtype=torch.long, device=cont.device)

    return draft


@torch.no_grad()
def lookahead_loop(model, input_ids, lens, N, T, ngram=2, eos_id=None, cache=None, draft=None):
    """``generate_lookahead`` written out: Python lists per row, one ``model.decode_block`` per
    iteration -> (tokens [B, N], new_lens list, stats dict, cache)."""
    draft = lookup_lists if draft is None else draft
    B, Lp = input_ids.shape
    dev = input_ids.device
    if cache is None:
        cache = model.init_cache(B, min(Lp + N, model.cfg["max_position_embeddings"]), dev)
    max_len = cache.max_len
    fill = 0 if eos_id is None else int(eos_id)
    plens = [int(x) for x in lens.tolist()]
    hist = [input_ids[b, :plens[b]].tolist() for b in range(B)]
    outs = [[] for _ in range(B)]
    first = greedy(model.prefill(input_ids, lens, cache)).tolist()
    pos = list(plens)  # cache.lens of a live row
    done = [False] * B  # parked: at eos_id, or no room in the cache to run the last token
    stats = {"model_calls": 0, "proposed": 0, "accepted": 0}

    def emit(b, tok):
        outs[b].append(tok)
        hist[b].append(tok)
        if (eos_id is not None and tok == fill) or pos[b] >= max_len:
            done[b] = True

    def idle(b):
        return done[b] or len(outs[b]) >= N

    for b in range(B):
        emit(b, first[b])
    for _ in range(N - 1):
        if all(idle(b) for b in range(B)):
            break
        cache.lens.copy_(torch.tensor([-1 if idle(b) else pos[b] for b in range(B)], dtype=torch.int32))
        width = Lp + N
        h = torch.tensor([row + [0] * (width - len(row)) for row in hist], dtype=torch.long, device=dev)
        n = torch.tensor([len(row) for row in hist], dtype=torch.long, device=dev)
        guess, k = draft(h, n, ngram=ngram, max_draft=T - 1)
        guess, k = guess.tolist(), k.tolist()
        counts = [0 if idle(b) else max(0, min(1 + k[b], max_len - pos[b], N - len(outs[b]))) for b in range(B)]
        block = [[hist[b][-1]] + guess[b] for b in range(B)]
        logits = model.decode_block(torch.tensor(block, dtype=torch.long, device=dev), cache,
                                    torch.tensor(counts, dtype=torch.int32, device=dev))
        picks = greedy(logits.view(B * T, -1)).view(B, T).tolist()
        stats["model_calls"] += 1
        for b in range(B):
            if counts[b] == 0:
                continue
            stats["proposed"] += counts[b] - 1
            a = 0
            while a + 1 < counts[b] and block[b][a + 1] == picks[b][a]:
                a += 1
            stats["accepted"] += a
            for j in range(a + 1):
                pos[b] += 1  # token j of the block is committed; picks[j] follows it
                emit(b, picks[b][j])
                if eos_id is not None and picks[b][j] == fill:
                    break
    cache.lens.copy_(torch.tensor([-1 if done[b] else pos[b] for b in range(B)], dtype=torch.int32))
    toks = torch.tensor([row + [fill] * (N - len(row)) for row in outs], dtype=torch.long, device=dev)
    return toks, [len(row) for row in outs], stats, cache
