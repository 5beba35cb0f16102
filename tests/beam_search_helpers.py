"""Shared by the ``GPT2LMModel.beam_search`` tests (CPU and GPU): a plain beam search that keeps one
cache row per beam and re-orders the cache physically each step, and the checks, each taking the
model and its device."""
import pytest
import torch

from decode_helpers import teacher_forced
from distributed_pipeline_amd.ops.decode import beam_step

NINF = float("-inf")
T = 24


def prompts(device, vocab, seed=2):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(vocab // 3, vocab, (3, 40), generator=g).to(device)
    return ids, torch.tensor([40, 17, 33], dtype=torch.int32, device=device)


def pick_eos(model, ids, lens, W):
    """An id some beams emit early and some never: the best beam's 6th token of prompt 0."""
    toks, _, _ = model.beam_search(ids, lens, T, num_beams=W)
    return int(toks[0, 0, 5])


@torch.no_grad()
def reordering_beam_search(model, ids, lens, T, W, eos_id=None):
    """The reference: every beam owns a whole cache row; after each ``beam_step`` the rows are
    re-ordered with ``index_select`` and the existing ``decode_step`` runs without a table.  As in
    ``beam_search`` the returned scores are the ``logp`` terms added up in float64 and the beams
    come back in their order (ties to the lower slot)."""
    B, Lp = ids.shape
    dev = ids.device
    fill = 0 if eos_id is None else int(eos_id)
    eos = -1 if eos_id is None else int(eos_id)
    cache = model.init_cache(B * W, Lp + T, dev)
    one = model.init_cache(B, Lp + T, dev)
    logits = model.prefill(ids, lens, one).unsqueeze(1).expand(B, W, -1)
    cache.buf.copy_(one.buf.repeat_interleave(W, dim=2))  # the prompt, physically, in every row
    glen = lens.to(torch.int32).clone()
    scores = torch.full((B, W), NINF, device=dev)
    scores[:, 0] = 0.0
    finished = torch.zeros(B, W, dtype=torch.bool, device=dev)
    hist = torch.full((B, W, T), fill, dtype=torch.long, device=dev)  # re-ordered like the cache
    total = torch.zeros(B, W, dtype=torch.float64, device=dev)
    n = torch.zeros(B, W, dtype=torch.long, device=dev)
    base = (torch.arange(B, device=dev) * W).view(B, 1)
    for t in range(T):
        scores, parent, token, nfin, logp = beam_step(logits, scores, finished, eos_id=eos, fill=fill,
                                                      return_logp=True)
        par = parent.long()
        total = total.gather(1, par) + logp.double()
        hist = hist.gather(1, par.unsqueeze(-1).expand(B, W, T))
        hist[:, :, t] = token
        exists = scores > NINF
        n = torch.where(exists, n.gather(1, par) + (~finished.gather(1, par)).long(), 0)
        finished = nfin | (exists & (glen >= cache.max_len).view(B, 1))
        if t + 1 == T:
            break
        cache.buf.copy_(cache.buf.index_select(2, (base + par).view(-1)))
        cache.lens.copy_(torch.where(exists & ~finished, glen.view(B, 1), -1).view(-1))
        logits = model.decode_step(token.view(-1), cache).view(B, W, -1)
        glen = glen + (glen < cache.max_len).to(glen.dtype)
    hist = torch.where(exists.unsqueeze(-1), hist, fill)
    scores = torch.where(exists, total.float(), NINF)
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    return hist.gather(1, order.unsqueeze(-1).expand(B, W, T)), n.gather(1, order), scores.gather(1, order)


def check_one_beam_is_greedy(model, device, vocab):
    ids, lens = prompts(device, vocab)
    want, want_lens = model.generate(ids, lens, T, temperature=0)
    toks, new_lens, scores = model.beam_search(ids, lens, T, num_beams=1)
    assert toks.shape == (3, 1, T) and new_lens.shape == scores.shape == (3, 1) and scores.dtype == torch.float32
    assert torch.equal(toks[:, 0], want) and torch.equal(new_lens[:, 0], want_lens)
    eos = int(want[1, 4])
    want, want_lens = model.generate(ids, lens, T, temperature=0, eos_id=eos)
    toks, new_lens, _ = model.beam_search(ids, lens, T, num_beams=1, eos_id=eos, check_every=3)
    assert torch.equal(toks[:, 0], want) and torch.equal(new_lens[:, 0], want_lens)
    assert int(want_lens[1]) == want[1].tolist().index(eos) + 1 < T


def check_against_reordering(model, device, vocab, W):
    ids, lens = prompts(device, vocab)
    eos = pick_eos(model, ids, lens, W)
    some_finish = False
    for e in (None, eos):
        want = reordering_beam_search(model, ids, lens, T, W, eos_id=e)
        got = model.beam_search(ids, lens, T, num_beams=W, eos_id=e)
        for a, b, name in zip(got, want, ("tokens", "new_lens", "scores")):
            assert torch.equal(a, b), (name, e, a, b)
        if e is not None:
            n = got[1]
            some_finish = bool((n < T).any()) and bool((n == T).any())
    assert some_finish, "eos_id must end some beams early and leave others running"


def check_scores_against_teacher_forcing(model, device, vocab, W):
    """-> (largest |score - teacher-forced sum| over the beams, the same for the greedy path)."""
    ids, lens = prompts(device, vocab)
    plens = lens.tolist()
    eos = pick_eos(model, ids, lens, W)

    def forced_sum(prompt_row, plen, cont, n):
        """Sum of log_softmax of the teacher-forced logits at the first n tokens of cont."""
        seq = torch.cat([prompt_row[:plen], cont[:n]]).view(1, -1)
        got, _ = teacher_forced(model, seq, [plen], plen)
        return sum(float(torch.log_softmax(got[(0, plen - 1 + i)].double(), -1)[int(cont[i])]) for i in range(n))

    # the greedy path's own difference: one beam is generate(temperature=0), and comes with its score.
    # Like the beams it is measured on rows that stop at eos_id and on rows that run all T tokens
    # (a sum of a few terms says nothing about the rounding of a sum of T), so with and without eos_id.
    d_greedy = 0.0
    for e in (eos, None):
        greedy, glens = model.generate(ids, lens, T, temperature=0, eos_id=e)
        one, one_lens, one_scores = model.beam_search(ids, lens, T, num_beams=1, eos_id=e)
        assert torch.equal(one[:, 0], greedy) and torch.equal(one_lens[:, 0], glens)
        d_greedy = max([d_greedy] + [abs(float(one_scores[b, 0]) - forced_sum(ids[b], plens[b], greedy[b], int(glens[b])))
                                     for b in range(3)])

    toks, new_lens, scores = model.beam_search(ids, lens, T, num_beams=W, eos_id=eos)
    assert bool((new_lens < T).any()) and bool((new_lens == T).any())
    d_beam = 0.0
    for b in range(3):
        for j in range(W):
            want = forced_sum(ids[b], plens[b], toks[b, j], int(new_lens[b, j]))
            d_beam = max(d_beam, abs(float(scores[b, j]) - want))
    return d_beam, d_greedy


def check_ordering_and_lengths(model, device, vocab, W):
    ids, lens = prompts(device, vocab)
    eos = pick_eos(model, ids, lens, W)
    toks, new_lens, scores = model.beam_search(ids, lens, T, num_beams=W, eos_id=eos)
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    for b in range(3):
        for j in range(W):
            row, n = toks[b, j].tolist(), int(new_lens[b, j])
            if eos in row:  # the closing eos_id counts, and the rest of the row is eos_id
                assert n == row.index(eos) + 1 and row[n:] == [eos] * (T - n)
            else:
                assert n == T
    for lp in (0.7, 2.0):
        t2, n2, s2 = model.beam_search(ids, lens, T, num_beams=W, eos_id=eos, length_penalty=lp)
        key = s2 / n2.clamp(min=1).float() ** lp
        assert (key[:, :-1] >= key[:, 1:]).all()
        for b in range(3):  # a permutation of the same beams
            a = sorted((toks[b, j].tolist(), int(new_lens[b, j]), float(scores[b, j])) for j in range(W))
            c = sorted((t2[b, j].tolist(), int(n2[b, j]), float(s2[b, j])) for j in range(W))
            assert a == c


def check_cache_and_table(model, device, vocab, W):
    ids, lens = prompts(device, vocab)
    eos = pick_eos(model, ids, lens, W)
    for rows in (3 * W + 1, 3, 3 * W - 1):
        if rows != 3 * W:
            with pytest.raises(ValueError):
                model.beam_search(ids, lens, T, num_beams=W, cache=model.init_cache(rows, 40 + T, device))
    for bad in (0, -1, 256):
        with pytest.raises(ValueError):
            model.beam_search(ids, lens, T, num_beams=bad)
    cache = model.init_cache(3 * W, 40 + T, device)
    toks, new_lens, scores = model.beam_search(ids, lens, T, num_beams=W, eos_id=eos, cache=cache)
    common = (lens.long() + T - 1).view(3, 1)  # T - 1 decode steps behind the prompt
    got = cache.lens.long().view(3, W)
    assert ((got == -1) | (got == common)).all() and (got == common).any() and (got == -1).any()
    assert cache.table.dtype == torch.uint8 and cache.table.shape == (3, W, 40 + T)
    assert int(cache.table.max()) < W
    if W > 1:
        assert int(cache.table.max()) > 0  # beams were re-parented
