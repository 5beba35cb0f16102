"""Shared by the logit-penalty tests (CPU and GPU): an independent yardstick of
``ops.decode.penalize_logits_`` - Python lists and sets for the counts and the banned set,
``numpy.float32`` scalars for the arithmetic, the rounding to the logits' dtype through torch - the
cases, and the checks, each taking the device it runs on.  Every comparison is of bits."""
import collections

import numpy as np
import pytest
import torch

from distributed_pipeline_amd.ops.decode import penalize_logits_, penalize_logits_ref

NINF = float("-inf")
SPECIALS = [0.0, -0.0, float("inf"), NINF, float("nan"), -2.75, 3.5, -1e-3, 7.0]


# ---- the yardstick --------------------------------------------------------------------------------

def window(hist_row, n, start, Lh):
    """The window of one row as a list, or None for a parked row."""
    if n < 0:
        return None
    hi = min(n, Lh)
    lo = 0 if start is None else min(max(start, 0), Lh)
    return hist_row[lo:hi] if hi > lo else []


def banned_set(w, g):
    m = len(w)
    return {w[i] for i in range(g - 1, m) if w[i - g + 1:i] == w[m - g + 1:m]} if g >= 1 else set()


def yardstick(logits, hist, n, start=None, theta=1.0, a_p=0.0, a_f=0.0, g=0):
    """-> the updated logits as a new contiguous CPU tensor of the same dtype."""
    out = logits.detach().cpu().clone()
    R, V = out.shape
    Lh = hist.shape[1]
    H, N = hist.cpu().tolist(), n.cpu().tolist()
    S = None if start is None else start.cpu().tolist()
    f = np.float32
    theta, a_p, a_f = f(theta), f(a_p), f(a_f)
    for r in range(R):
        w = window(H[r], N[r], None if S is None else S[r], Lh)
        if not w:
            continue
        ban = banned_set(w, g)
        for x, c in collections.Counter(w).items():
            if not 0 <= x < V:
                continue
            s = f(out[r, x].float().item())
            with np.errstate(all="ignore"):
                s = s * theta if s < 0 else s / theta
                s = s - (a_p + a_f * f(c))
            if x in ban:
                s = f(NINF)
            out[r, x] = torch.tensor(float(s), dtype=torch.float32).to(out.dtype)
    return out


def same_bits(a, b):
    """Equal bit for bit; two NaNs are equal whatever their payload."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
    as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(((a.view(as_int) == b.view(as_int)) | (torch.isnan(a) & torch.isnan(b))).all())


# ---- cases ----------------------------------------------------------------------------------------

def make_case(seed, R, V, Lh, g, *, dtype=torch.float32, hist_dtype=torch.int64, start_mode="none", theta=1.3,
              a_p=0.0, a_f=0.0, strided=False):
    """Random rows over a small alphabet (so ids and n-grams repeat, with counts well above 3), with
    ids below 0 and at or above V inside the windows, special values at the logits the windows
    touch, ``n`` on both sides of every edge and a tail beyond ``hi`` that holds in-range ids no
    window has (reading it would change their logits or the bans)."""
    rng = np.random.RandomState(seed)
    alphabet = sorted({int(x) for x in rng.randint(0, V, size=min(V, 6))})
    odd = [-1, -7, V, V + 5] + ([2 ** 32 + alphabet[0], -2 ** 40] if hist_dtype == torch.int64 else [])
    poison = [x for x in range(V - 1, -1, -1) if x not in alphabet][:2] or [alphabet[0]]
    edges = [Lh, Lh - 1, Lh + 1, 0, -1, 1, 2, g, g + 1, g - 1, Lh // 2, Lh + 1000, -5, 3, Lh - 2]
    n = [edges[(r + seed) % len(edges)] for r in range(R)]
    n[0] = Lh  # a full window in every case
    hist = np.empty((R, Lh), dtype=np.int64)
    for r in range(R):
        row = rng.choice(alphabet, size=Lh)
        row[rng.rand(Lh) < 0.08] = rng.choice(odd)
        if r % 4 == 1:
            row[:] = alphabet[0]  # a run of one id: every position behind the first g - 1 is a ban source
        hi = max(0, min(n[r], Lh))
        row[hi:] = rng.choice(poison, size=Lh - hi)
        hist[r] = row
    start = None
    if start_mode != "none":
        modes = {"zero": lambda r: 0, "inside": lambda r: max(n[r], 0) // 3 + (r % 2), "equal": lambda r: n[r],
                 "beyond": lambda r: n[r] + 2, "mixed": lambda r: [0, max(n[r], 0) // 2, n[r], n[r] + 1, -3, 1][r % 6]}
        start = torch.tensor([modes[start_mode](r) for r in range(R)], dtype=torch.int64)
    logits = torch.randn(R, V + 8, generator=torch.Generator().manual_seed(seed)) * 3
    for r in range(R):
        for k, x in enumerate(alphabet + poison):
            logits[r, 3 + x] = SPECIALS[(k + r) % len(SPECIALS)]
    return dict(logits=logits.to(dtype), hist=torch.from_numpy(hist).to(hist_dtype),
                n=torch.tensor(n, dtype=torch.int64), start=start, theta=theta, a_p=a_p, a_f=a_f, g=g, strided=strided)


def crafted(w, V, g, **kw):
    """One row whose window is exactly ``w``."""
    logits = torch.linspace(-4.0, 4.0, V + 8).view(1, -1).clone()
    case = dict(logits=logits, hist=torch.tensor([w + [w[0]] * 2], dtype=torch.int64), n=torch.tensor([len(w)]),
                start=None, theta=1.3, a_p=0.25, a_f=-0.5, g=g, strided=False)
    case.update(kw)
    return case


# name -> a function that builds the case; R, V and Lh in the names
BF, I32 = torch.bfloat16, torch.int32
CASES = {
    # the n-gram edges, by hand (V = 97): sources at the first eligible and at the last position,
    # overlapping sources, a banned id whose first occurrence is no source, g = m and g = m + 1
    "first_eligible_source": lambda: crafted([5, 9, 7, 5, 3, 5], 97, 2),
    "last_position_source": lambda: crafted([8, 1, 2, 6, 1, 2, 4, 1, 2], 97, 3),
    "run_of_one_id": lambda: crafted([4] * 7, 97, 3),
    "first_occurrence_is_no_source": lambda: crafted([6, 2, 2, 6, 2, 1, 6, 2], 97, 3),
    "g_equals_m": lambda: crafted([2, 2, 2], 97, 3),
    "g_equals_m_plus_1": lambda: crafted([2, 2, 2], 97, 4),
    "g1_bans_the_window": lambda: crafted([3, 96, 0, 3, -2, 97], 97, 1),
    "counts_and_negative_alphas": lambda: crafted([1, 1, 1, 1, 2, 2, 2, 5], 97, 0, a_p=-0.75, a_f=0.3),
    # random rows: every Lh of the kernel's paths (positions per thread 1, 2, 4, 8; waves in and out of
    # the window), every V and R, g in {0, 1, 2, 4}, theta in {1, 1.3, 0.7}, both dtypes of each tensor
    "R3_V5_L1": lambda: make_case(1, 3, 5, 1, 1, theta=0.7, a_p=0.5),
    "R3_V97_L63": lambda: make_case(2, 3, 97, 63, 2, dtype=BF, hist_dtype=I32, a_f=0.25, start_mode="beyond"),
    "R3_V97_L64": lambda: make_case(3, 3, 97, 64, 4, start_mode="mixed", a_p=-0.5, a_f=0.125),
    "R70_V97_L65": lambda: make_case(4, 70, 97, 65, 2, dtype=BF, start_mode="mixed", theta=0.7, a_p=0.3, a_f=0.1),
    "R3_V50257_L255": lambda: make_case(5, 3, 50257, 255, 4, dtype=BF, hist_dtype=I32, strided=True, a_f=0.2),
    "R3_V5_L256": lambda: make_case(6, 3, 5, 256, 1, theta=1.0, a_p=0.4, start_mode="inside"),
    "R70_V50257_L257": lambda: make_case(7, 70, 50257, 257, 2, dtype=BF, strided=True, start_mode="mixed", a_p=0.2,
                                         a_f=-0.05),
    "R1_V97_L1024": lambda: make_case(8, 1, 97, 1024, 4, hist_dtype=I32, theta=1.0, a_f=0.01),
    "R3_V50257_L1024": lambda: make_case(9, 3, 50257, 1024, 0, dtype=BF, hist_dtype=I32, start_mode="equal"),
    "R3_V97_L2048": lambda: make_case(10, 3, 97, 2048, 2, dtype=BF, start_mode="inside", strided=True),
    "R1_V50257_L2048": lambda: make_case(11, 1, 50257, 2048, 4, theta=0.7, a_p=0.1, a_f=0.003, start_mode="zero"),
    "R3_V97_L2049": lambda: make_case(12, 3, 97, 2049, 2, dtype=BF, hist_dtype=I32, a_p=0.5),  # the PyTorch path
}
GPU_ONLY_CASES = {
    "R70_V50257_L2048": lambda: make_case(13, 70, 50257, 2048, 4, dtype=BF, hist_dtype=I32, start_mode="mixed",
                                          a_p=0.2, a_f=0.01),
    "R70_V97_L1024": lambda: make_case(14, 70, 97, 1024, 2, strided=True, theta=0.7, a_f=0.02),
}


def place(case, device):
    """The case's tensors on ``device``: the logits cut from a wider buffer at an odd offset; with
    ``strided`` the history with strides of its own.  -> (buffer, logits view, hist, n, start)."""
    buf = case["logits"].to(device).clone()
    V = buf.shape[1] - 8
    logits = buf[:, 3:3 + V]
    hist = case["hist"].to(device)
    if case["strided"]:
        R, Lh = hist.shape
        wide = torch.full((R, 2 * Lh + 3), 1, dtype=hist.dtype, device=device)  # id 1 between the entries
        wide[:, 1:1 + 2 * Lh:2] = hist
        hist = wide[:, 1:1 + 2 * Lh:2]
    start = None if case["start"] is None else case["start"].to(device)
    return buf, logits, hist, case["n"].to(device), start


def scalars(case):
    return dict(repetition_penalty=case["theta"], presence_penalty=case["a_p"], frequency_penalty=case["a_f"],
                no_repeat_ngram=case["g"])


# ---- the checks -----------------------------------------------------------------------------------

def check_case(case, device):
    """The op against the yardstick on the whole buffer the logits are cut from; two calls give equal
    bits; the PyTorch path gives the same bits; int32 ``n`` / ``start`` give the same bits."""
    buf, logits, hist, n, start = place(case, device)
    before = buf.clone()
    want = before.cpu().clone()
    want[:, 3:3 + logits.shape[1]] = yardstick(logits, hist, n, start, case["theta"], case["a_p"], case["a_f"], case["g"])
    out = penalize_logits_(logits, hist, n, start=start, **scalars(case))
    assert out is logits
    assert same_bits(buf, want)
    if case["start"] is None:
        assert not same_bits(buf, before), "the case changes nothing"
    for path in (penalize_logits_, penalize_logits_ref):
        buf2, logits2, hist2, _, _ = place(case, device)
        path(logits2, hist2, n.to(torch.int32), start=None if start is None else start.to(torch.int32), **scalars(case))
        assert same_bits(buf2, buf), path.__name__


def check_defaults_change_nothing(device):
    case = make_case(21, 3, 97, 65, 0, dtype=BF)
    buf, logits, hist, n, start = place(case, device)
    before = buf.clone()
    assert penalize_logits_(logits, hist, n) is logits
    penalize_logits_(logits, hist, n, start=start, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                     no_repeat_ngram=0)
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16))


def check_rejections(device):
    logits = torch.zeros(4, 11, device=device)
    hist = torch.zeros(4, 6, dtype=torch.long, device=device)
    n = torch.full((4,), 6, device=device)
    ok = dict(repetition_penalty=1.2)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram=-1),
                dict(repetition_penalty=float("nan"))):
        with pytest.raises(ValueError):
            penalize_logits_(logits, hist, n, **bad)
    for args in ((logits, hist[:3], n), (logits, hist, n[:3]), (logits[0], hist, n), (logits, hist[0], n),
                 (logits, hist.float(), n), (logits, hist, n.float())):
        with pytest.raises(ValueError):
            penalize_logits_(*args, **ok)
    with pytest.raises(ValueError):
        penalize_logits_(logits, hist, n, start=n[:2], **ok)
    # rows that overlap: stride 0 (the first step of a beam search) and a stride below V
    with pytest.raises(ValueError, match="overlap"):
        penalize_logits_(logits[:1].expand(4, 11), hist, n, **ok)
    with pytest.raises(ValueError, match="overlap"):
        penalize_logits_(torch.zeros(40, device=device).as_strided((4, 11), (7, 1)), hist, n, **ok)
    assert not logits.any()  # nothing was written on the way
    # one row may have any stride
    penalize_logits_(logits[:1].expand(1, 11), hist[:1], n[:1], **ok)


# ---- generation: the loops written out around the yardstick ---------------------------------------

N_NEW = 24
PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2, no_repeat_ngram=3)
DEFAULTS = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0, min_new_tokens=0,
                penalize_prompt=True)


def gen_prompts(device, vocab, seed=2):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(vocab // 3, vocab, (4, 40), generator=g).to(device)
    return ids, torch.tensor([40, 17, 1, 33], dtype=torch.int32, device=device)


def _through_yardstick(logits, hist, n, start, pen):
    return yardstick(logits, hist, n, start, pen.get("repetition_penalty", 1.0), pen.get("presence_penalty", 0.0),
                     pen.get("frequency_penalty", 0.0), pen.get("no_repeat_ngram", 0)).to(logits.device)


@torch.no_grad()
def written_out_generate(model, ids, lens, N, pick, *, eos_id=None, min_new_tokens=0, penalize_prompt=True, **pen):
    """``generate``'s loop with the yardstick between the same model calls and each row's history as
    a Python list; ``pick(logits, t)`` chooses the tokens of step t."""
    B, Lp = ids.shape
    dev = ids.device
    cache = model.init_cache(B, Lp + N, dev)
    fill = 0 if eos_id is None else int(eos_id)
    plen = lens.tolist()
    rows = [ids[b, :plen[b]].tolist() for b in range(B)]
    out = torch.full((B, N), fill, dtype=torch.long, device=dev)
    new_lens = torch.zeros(B, dtype=torch.long, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    logits = model.prefill(ids, lens, cache)
    for t in range(N):
        if t < min_new_tokens:
            logits[:, fill] = NINF
        hist = torch.tensor([r + [0] * (Lp + N - len(r)) for r in rows])
        n = torch.tensor([len(r) for r in rows])
        logits = _through_yardstick(logits, hist, n, None if penalize_prompt else torch.tensor(plen), pen)
        tok = torch.where(done, fill, pick(logits, t))
        out[:, t] = tok
        for b, x in enumerate(tok.tolist()):
            rows[b].append(x)
        new_lens += (~done).long()
        if eos_id is not None:
            done = done | (tok == fill)
        done = done | (cache.lens >= cache.max_len)
        if t + 1 == N:
            break
        cache.lens.masked_fill_(done, -1)
        logits = model.decode_step(tok, cache)
    return out, new_lens


def _greedy(logits, t):
    from utils.lm_sampling import greedy
    return greedy(logits)


def check_generate_equals_the_written_out_loop(model, device, vocab):
    from distributed_pipeline_amd.ops.decode import sample_tokens
    from utils.lm_sampling import sample_next
    ids, lens = gen_prompts(device, vocab)

    def both(pick_factory, **kw):
        got = model.generate(ids, lens, N_NEW, **kw, **PENALTIES)
        kw = {k: v for k, v in kw.items() if k in ("eos_id", "min_new_tokens", "penalize_prompt")}
        want = written_out_generate(model, ids, lens, N_NEW, pick_factory(), **kw, **PENALTIES)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (got, want)
        return got

    plain, _ = model.generate(ids, lens, N_NEW, temperature=0)
    got, _ = both(lambda: _greedy, temperature=0)
    assert not torch.equal(got, plain)  # the penalties do change what is generated
    both(lambda: _greedy, temperature=0, penalize_prompt=False)

    def with_generator():
        gen = torch.Generator(device=device).manual_seed(5)
        return lambda logits, t: sample_next(logits, 0.9, 20, 0.0, gen)

    both(with_generator, temperature=0.9, top_k=20, generator=torch.Generator(device=device).manual_seed(5))

    def philox():
        return lambda logits, t: sample_tokens(logits, temperature=0.8, top_k=50, top_p=0.9, seed=77, step=t, row_base=3)

    both(philox, temperature=0.8, top_k=50, top_p=0.9, noise_seed=77, row_base=3)


def repeated_ngrams(prompt, cont, g):
    """How many g-grams that end inside ``cont`` occurred earlier in prompt + cont."""
    seq = list(prompt) + list(cont)
    seen = {tuple(seq[i - g + 1:i + 1]) for i in range(g - 1, len(prompt))}
    again = 0
    for i in range(max(len(prompt), g - 1), len(seq)):
        gram = tuple(seq[i - g + 1:i + 1])
        again += gram in seen
        seen.add(gram)
    return again


def check_no_repeat_ngram(model, device, vocab, g=2):
    """Greedy decoding of the random-init model repeats itself; with the ban no g-gram comes twice."""
    ids, lens = gen_prompts(device, vocab)
    free, _ = model.generate(ids, lens, N_NEW, temperature=0)
    held, new_lens = model.generate(ids, lens, N_NEW, temperature=0, no_repeat_ngram=g)
    assert new_lens.tolist() == [N_NEW] * 4
    prompts = [ids[b, :int(lens[b])].tolist() for b in range(4)]
    assert sum(repeated_ngrams(prompts[b], free[b].tolist(), g) for b in range(4)) > 0
    assert [repeated_ngrams(prompts[b], held[b].tolist(), g) for b in range(4)] == [0] * 4


def check_min_new_tokens(model, device, vocab, M=5):
    ids, lens = gen_prompts(device, vocab)
    free, _ = model.generate(ids, lens, N_NEW, temperature=0)
    eos = int(free[0, 0])  # what row 0 would emit first
    toks, new_lens = model.generate(ids, lens, N_NEW, temperature=0, eos_id=eos)
    assert int(new_lens[0]) == 1
    toks, new_lens = model.generate(ids, lens, N_NEW, temperature=0, eos_id=eos, min_new_tokens=M)
    assert not (toks[:, :M] == eos).any() and int(new_lens.min()) > M
    want = written_out_generate(model, ids, lens, N_NEW, _greedy, eos_id=eos, min_new_tokens=M)
    assert torch.equal(toks, want[0]) and torch.equal(new_lens, want[1])
    # together with the penalties, and more than the loop is long: eos_id never comes
    toks, new_lens = model.generate(ids, lens, 6, temperature=0, eos_id=eos, min_new_tokens=6, **PENALTIES)
    assert not (toks == eos).any() and new_lens.tolist() == [6] * 4
    with pytest.raises(ValueError, match="eos_id"):
        model.generate(ids, lens, 4, temperature=0, min_new_tokens=2)
    with pytest.raises(ValueError):
        model.generate(ids, lens, 4, temperature=0, eos_id=eos, min_new_tokens=-1)


def check_penalize_prompt_is_the_window(model, device, vocab):
    """A strongly negative presence penalty pulls the ids of the window up: with the prompt in the
    window the first token is one of the prompt's, without it the window is empty at the first step
    and the first token is the plain one."""
    ids, lens = gen_prompts(device, vocab)
    free, _ = model.generate(ids, lens, 4, temperature=0)
    kw = dict(temperature=0, presence_penalty=-1000.0)
    with_prompt, _ = model.generate(ids, lens, 4, penalize_prompt=True, **kw)
    without, _ = model.generate(ids, lens, 4, penalize_prompt=False, **kw)
    for b in range(4):
        assert int(with_prompt[b, 0]) in ids[b, :int(lens[b])].tolist()
        assert int(without[b, 0]) == int(free[b, 0])
        assert without[b].tolist() == [int(free[b, 0])] * 4  # then the window holds that token alone
    for flag, got in ((True, with_prompt), (False, without)):
        want, _ = written_out_generate(model, ids, lens, 4, _greedy, penalize_prompt=flag, presence_penalty=-1000.0)
        assert torch.equal(got, want)


@torch.no_grad()
def reordering_beam_search(model, ids, lens, T, W, *, eos_id=None, min_new_tokens=0, penalize_prompt=True, **pen):
    """``beam_search_helpers.reordering_beam_search`` - one cache row per beam, re-ordered with
    ``index_select`` - with one history row per beam re-ordered the same way and the yardstick on
    every step's logits."""
    from distributed_pipeline_amd.ops.decode import beam_step
    B, Lp = ids.shape
    dev = ids.device
    fill = 0 if eos_id is None else int(eos_id)
    eos = -1 if eos_id is None else int(eos_id)
    cache = model.init_cache(B * W, Lp + T, dev)
    one = model.init_cache(B, Lp + T, dev)
    plen = lens.long().cpu()
    start = None if penalize_prompt else plen
    logits = model.prefill(ids, lens, one)
    if min_new_tokens > 0:
        logits[:, fill] = NINF
    logits = _through_yardstick(logits, ids, plen, start, pen).unsqueeze(1).expand(B, W, -1)
    cache.buf.copy_(one.buf.repeat_interleave(W, dim=2))
    seqs = torch.zeros(B * W, Lp + T, dtype=torch.long)  # prompt and output of every beam
    seqs[:, :Lp] = ids.cpu().repeat_interleave(W, dim=0)
    at = plen.repeat_interleave(W)
    start = None if start is None else at.clone()
    glen = lens.to(torch.int32).clone()
    scores = torch.full((B, W), NINF, device=dev)
    scores[:, 0] = 0.0
    finished = torch.zeros(B, W, dtype=torch.bool, device=dev)
    hist = torch.full((B, W, T), fill, dtype=torch.long, device=dev)
    total = torch.zeros(B, W, dtype=torch.float64, device=dev)
    n = torch.zeros(B, W, dtype=torch.long, device=dev)
    base = (torch.arange(B, device=dev) * W).view(B, 1)
    for t in range(T):
        scores, parent, token, nfin, logp = beam_step(logits, scores, finished, eos_id=eos, fill=fill, return_logp=True)
        par = parent.long()
        total = total.gather(1, par) + logp.double()
        hist = hist.gather(1, par.unsqueeze(-1).expand(B, W, T))
        hist[:, :, t] = token
        exists = scores > NINF
        n = torch.where(exists, n.gather(1, par) + (~finished.gather(1, par)).long(), 0)
        finished = nfin | (exists & (glen >= cache.max_len).view(B, 1))
        if t + 1 == T:
            break
        order = (base + par).view(-1)
        seqs = seqs.index_select(0, order.cpu())
        seqs[torch.arange(B * W), at + t] = token.view(-1).cpu()
        cache.buf.copy_(cache.buf.index_select(2, order))
        live = exists & ~finished
        cache.lens.copy_(torch.where(live, glen.view(B, 1), -1).view(-1))
        logits = model.decode_step(token.view(-1), cache)
        if t + 1 < min_new_tokens:
            logits[:, fill] = NINF
        rows = torch.where(live.view(-1).cpu(), at + t + 1, -1)
        logits = _through_yardstick(logits, seqs, rows, start, pen).view(B, W, -1)
        glen = glen + (glen < cache.max_len).to(glen.dtype)
    hist = torch.where(exists.unsqueeze(-1), hist, fill)
    scores = torch.where(exists, total.float(), NINF)
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    return hist.gather(1, order.unsqueeze(-1).expand(B, W, T)), n.gather(1, order), scores.gather(1, order)


def check_beam_search_equals_the_reordering_search(model, device, vocab, W):
    import beam_search_helpers as bsh
    ids, lens = bsh.prompts(device, vocab)
    plain = model.beam_search(ids, lens, bsh.T, num_beams=W)
    eos = int(model.beam_search(ids, lens, bsh.T, num_beams=W, **PENALTIES)[0][0, 0, 5])
    for kw in (dict(), dict(eos_id=eos), dict(eos_id=eos, min_new_tokens=8, penalize_prompt=False)):
        want = reordering_beam_search(model, ids, lens, bsh.T, W, **kw, **PENALTIES)
        got = model.beam_search(ids, lens, bsh.T, num_beams=W, **kw, **PENALTIES)
        for a, b, name in zip(got, want, ("tokens", "new_lens", "scores")):
            assert torch.equal(a, b), (name, kw, a, b)
        if "min_new_tokens" in kw:
            assert not (got[0][:, :, :8] == eos).any()
        elif kw:
            assert bool((got[1] < bsh.T).any()), "eos_id must end some beams early"
    assert not torch.equal(got[0], plain[0])


def check_defaults_are_the_calls_without(model, device, vocab):
    ids, lens = gen_prompts(device, vocab)
    for kw in (dict(temperature=0), dict(temperature=0.8, top_k=30, noise_seed=11),
               dict(temperature=0, eos_id=int(model.generate(ids, lens, 8, temperature=0)[0][1, 3]))):
        a = model.generate(ids, lens, N_NEW, **kw)
        b = model.generate(ids, lens, N_NEW, **kw, **DEFAULTS)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = model.beam_search(ids, lens, N_NEW, num_beams=3)
    b = model.beam_search(ids, lens, N_NEW, num_beams=3, **DEFAULTS)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = model.generate_lookahead(ids, lens, N_NEW, lookahead=4)
    b = model.generate_lookahead(ids, lens, N_NEW, lookahead=4, **DEFAULTS)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def check_lookahead_raises(model, device, vocab):
    ids, lens = gen_prompts(device, vocab)
    for kw in (dict(repetition_penalty=1.2), dict(presence_penalty=0.1), dict(frequency_penalty=-0.1),
               dict(no_repeat_ngram=2), dict(min_new_tokens=1, eos_id=5), dict(penalize_prompt=False)):
        with pytest.raises(ValueError, match="lookahead"):
            model.generate_lookahead(ids, lens, 8, lookahead=4, **kw)
