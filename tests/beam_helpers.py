"""Shared by the ``ops.decode.beam_step`` tests (PyTorch path and kernel): the inputs, a float64
evaluation of the definition that is independent of the op, and the checks themselves, each taking
the function under test (``step(logits, scores, finished, eos_id, fill) -> 4 tensors``) and the
device it runs on."""
import functools

import numpy as np
import torch

VS = [3000, 4099, 50257]
WS = [1, 2, 3, 8]
B = 3
NINF = float("-inf")


def strided(x, device):
    """[B, W, V] values on ``device`` inside a wider buffer: batch stride > W V, an odd element offset."""
    Bn, W, V = x.shape
    sb = W * V + 5
    flat = torch.full((Bn * sb + 3,), float("nan"), dtype=x.dtype, device=device)
    view = flat[3:3 + Bn * sb].view(Bn, sb)[:, :W * V].view(Bn, W, V)
    view.copy_(x)
    assert view.stride() == (sb, V, 1) and view.storage_offset() == 3
    return view


@functools.lru_cache(maxsize=None)
def case(V, W, kind, dtype=torch.float32):
    """(logits [B, W, V], scores, finished) on the CPU.  ``plain``: every beam live; ``mixed``: some
    beams finished and some at -inf (at least one live beam per prompt)."""
    g = torch.Generator().manual_seed(7919 * V + 31 * W + (0 if kind == "plain" else 1))
    logits = (2 * torch.randn(B, W, V, generator=g)).to(dtype)
    scores = 1.5 * torch.randn(B, W, generator=g)
    finished = torch.zeros(B, W, dtype=torch.bool)
    if kind == "mixed":
        for b in range(B):
            for w in range(1, W):
                if (b + w) % 3 == 0:
                    finished[b, w] = True
                elif (b + w) % 3 == 1 and w >= 2:
                    scores[b, w] = NINF
    return logits, scores, finished


def candidates64(logits, scores, finished, fill, keep):
    """float64 evaluation of the definition -> per prompt the first ``keep`` candidates
    [(c, w, v, s_bits)] in the order (descending c, ascending w, ascending v); s_bits tells equal
    logits of one beam apart from different ones."""
    x = logits.detach().float().cpu().numpy()
    sc = scores.detach().cpu().numpy().astype(np.float64)
    fin = finished.cpu().numpy()
    out = []
    for b in range(x.shape[0]):
        cands = []
        for w in range(x.shape[1]):
            if not sc[b, w] > -np.inf:
                continue
            if fin[b, w]:
                cands.append((sc[b, w], w, fill, None))
                continue
            s32 = np.where(np.isnan(x[b, w]), np.float32(-np.inf), x[b, w])
            s = s32.astype(np.float64)
            m = s.max()
            if not np.isfinite(m):
                continue
            with np.errstate(divide="ignore"):
                c = sc[b, w] + ((s - m) - np.log(np.exp(s - m).sum()))
            order = np.argsort(-c, kind="stable")[:keep]
            cands += [(c[v], w, int(v), s32[v].tobytes()) for v in order if c[v] > -np.inf]
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        out.append(cands[:keep])
    return out


def e32_of(logits, scores, finished):
    """Largest error of the fp32 PyTorch path's candidates against float64 on this input."""
    s = logits.detach().float().cpu()
    s = torch.where(torch.isnan(s), NINF, s)
    d = s - s.amax(-1, keepdim=True)
    c32 = scores.cpu().unsqueeze(-1) + (d - torch.log(torch.exp(d).sum(-1, keepdim=True)))
    s64 = s.double()
    d64 = s64 - s64.amax(-1, keepdim=True)
    c64 = scores.cpu().double().unsqueeze(-1) + (d64 - torch.log(torch.exp(d64).sum(-1, keepdim=True)))
    ok = torch.isfinite(c64) & ~finished.cpu().unsqueeze(-1)
    return (c32.double() - c64)[ok].abs().max().item()


def assert_separated(cands, W, e32, same_logit_ok=False):
    """The precondition: every gap between consecutive float64 candidates among the first W + 1
    exceeds 8 e32 (with ``same_logit_ok``, candidates of one beam with the same logit bits are not
    counted: their order is the id order on every path)."""
    worst = float("inf")
    for row in cands:
        for a, b in zip(row[:W + 1], row[1:W + 1]):
            if same_logit_ok and a[1] == b[1] and a[3] is not None and a[3] == b[3]:
                continue
            worst = min(worst, a[0] - b[0])
    assert worst > 8 * e32, (worst, e32)
    return worst


def check_exact(step, device, V, W, kind, dtype=torch.float32):
    """Picks equal the float64 picks exactly and scores lie within 4 e32 + 2^-23 |c|, under the
    asserted precondition -> (new_scores, parent, token, new_finished) for further checks."""
    logits, scores, finished = case(V, W, kind, dtype)
    eos, fill = 17, 5
    cands = candidates64(logits, scores, finished, fill, W + 1)
    e32 = e32_of(logits, scores, finished)
    gap = assert_separated(cands, W, e32, same_logit_ok=dtype != torch.float32)
    out = step(strided(logits, device), scores.to(device), finished.to(device), eos, fill)
    ns, par, tok, nf = [t.cpu() for t in out]
    assert ns.dtype == torch.float32 and par.dtype == torch.int32 and tok.dtype == torch.int64 and nf.dtype == torch.bool
    assert ns.shape == par.shape == tok.shape == nf.shape == (B, W)
    for b, row in enumerate(cands):
        row = row[:W]
        assert len(row) == W  # these inputs always leave W candidates
        assert par[b].tolist() == [c[1] for c in row], (b, par[b].tolist(), row)
        assert tok[b].tolist() == [c[2] for c in row], (b, tok[b].tolist(), row)
        for j, c in enumerate(row):
            assert abs(float(ns[b, j]) - c[0]) <= 4 * e32 + 2.0 ** -23 * abs(c[0]), (b, j, float(ns[b, j]), c[0], e32)
            assert bool(nf[b, j]) == (bool(finished[b, c[1]]) or c[2] == eos)
    return (ns, par, tok, nf), gap / e32


def check_ties(step, device):
    """Exact by construction: equal scores over one bf16 row (beam stride 0), and the first step."""
    V = 4099
    g = torch.Generator().manual_seed(5)
    row = (2 * torch.randn(2, 1, V, generator=g)).bfloat16()
    row[1, 0, [7, 1000, 4098]] = row[1].max()  # row 1 holds its maximum three times more
    flat = row.float().view(2, V)
    assert (flat[0] == flat[0].max()).sum() == 1 and (flat[1] == flat[1].max()).sum() >= 3
    assert all(len(set(flat[b].tolist())) < V // 2 for b in range(2))  # bf16: many equal logits
    for W in (1, 3, 8):
        x = row.to(device).expand(2, W, V)
        assert W == 1 or x.stride(1) == 0
        scores = torch.full((2, W), -1.25, device=device)
        fin = torch.zeros(2, W, dtype=torch.bool, device=device)
        ns, par, tok, nf = [t.cpu() for t in step(x, scores, fin, -1, 0)]
        # row 0, a single maximum: the beams 0 .. W - 1 at its id
        assert par[0].tolist() == list(range(W)) and tok[0].tolist() == [int(flat[0].argmax())] * W
        # in general equal logits of equal scores are equal candidates: flat-index order decides
        order = torch.sort(flat.repeat(1, W), dim=-1, descending=True, stable=True).indices[:, :W]
        assert torch.equal(par.long(), order // V) and torch.equal(tok, order % V)
        ids = (flat[1] == flat[1].max()).nonzero().flatten().tolist()  # beam 0's copies come first, in id order
        assert par[1, :len(ids)].tolist() == [0] * min(W, len(ids)) and tok[1, :len(ids)].tolist() == ids[:W]
        assert not nf.any()
        # the first step: scores [0, -inf, ...] -> the row's W best ids, equal logits in id order
        scores = torch.full((2, W), NINF, device=device)
        scores[:, 0] = 0.0
        ns, par, tok, nf = [t.cpu() for t in step(x, scores, fin, -1, 0)]
        want = torch.sort(row.float().view(2, V), dim=-1, descending=True, stable=True).indices[:, :W]
        assert not par.any() and torch.equal(tok, want)
        assert (ns[:, :-1] >= ns[:, 1:]).all()


def check_finished(step, device):
    V, W = 3000, 3
    g = torch.Generator().manual_seed(6)
    x = (2 * torch.randn(2, W, V, generator=g)).to(device)
    # -0.0 and a denormal: the bits must come back unchanged
    scores = torch.tensor([[-3.0, -0.0, -9.0], [-2.0, -30.0, 1e-40]], device=device)
    fin = torch.tensor([[False, True, False], [False, False, True]], device=device)
    eos, fill = 11, 2999
    ns, par, tok, nf = [t.cpu() for t in step(x, scores, fin, eos, fill)]
    for b, w in ((0, 1), (1, 2)):  # the finished beam has the best score: rank 0
        assert int(par[b, 0]) == w and int(tok[b, 0]) == fill and bool(nf[b, 0])
        assert int(ns.view(torch.int32)[b, 0]) == int(scores.cpu().view(torch.int32)[b, w])
        assert (par[b, 1:] != w).all()  # exactly one candidate
    # a live beam that picks eos_id finishes
    x2 = x.clone()
    x2[0, 0, eos] = 50.0
    ns, par, tok, nf = [t.cpu() for t in step(x2, scores, fin, eos, fill)]
    j = [i for i in range(W) if int(par[0, i]) == 0 and int(tok[0, i]) == eos]
    assert len(j) == 1 and bool(nf[0, j[0]])
    assert not any(bool(nf[0, i]) for i in range(W) if i != j[0] and int(par[0, i]) != 1)
    ns, par, tok, nf = [t.cpu() for t in step(x2, scores, fin, -1, fill)]  # eos_id < 0: never
    assert [bool(v) for v in nf[0]] == [int(p) == 1 for p in par[0]]


def check_logp(step5, device):
    """``logp`` (the fifth output): ``new_scores == scores[parent] + logp`` in fp32, bit for bit, for a
    live beam's pick; 0 for a finished beam's candidate and for an empty slot; and the float64 value."""
    for V, W, kind, dtype in ((3000, 3, "mixed", torch.float32), (50257, 8, "mixed", torch.float32),
                              (4099, 8, "plain", torch.bfloat16)):
        logits, scores, finished = case(V, W, kind, dtype)
        ns, par, tok, nf, lp = [t.cpu() for t in step5(strided(logits, device), scores.to(device),
                                                       finished.to(device), 17, 5)]
        assert lp.dtype == torch.float32 and lp.shape == (B, W)
        pfin = finished.gather(1, par.long())
        assert (lp[pfin] == 0).all() and not pfin.all()
        live = ~pfin
        again = scores.gather(1, par.long()) + lp
        assert torch.equal(again[live].view(torch.int32), ns[live].view(torch.int32))
        s = torch.where(torch.isnan(logits.double()), NINF, logits.double())
        want = torch.log_softmax(s, -1).gather(1, par.long().unsqueeze(-1).expand(B, W, V)).gather(2, tok.unsqueeze(-1))
        e32 = e32_of(logits, scores, finished)
        assert ((lp.double() - want.squeeze(-1))[live].abs() <= 4 * e32).all()
    # an empty slot: V = 5, W = 8, first step
    x = torch.tensor([0.5, 2.0, -1.0, 2.0, 0.0]).view(1, 1, 5).expand(1, 8, 5)
    scores = torch.full((1, 8), NINF)
    scores[0, 0] = 0.0
    fin = torch.zeros(1, 8, dtype=torch.bool)
    ns, par, tok, nf, lp = [t.cpu() for t in step5(x.to(device), scores.to(device), fin.to(device), -1, 3)]
    assert (lp[0, 5:] == 0).all() and torch.equal(lp[0, :5].view(torch.int32), ns[0, :5].view(torch.int32))


def check_degenerate(step, device):
    inf, nan = float("inf"), float("nan")
    fill = 3
    # NaN and -inf logits are never picked while a finite candidate is left
    V, W = 3000, 3
    g = torch.Generator().manual_seed(8)
    x = 2 * torch.randn(1, W, V, generator=g)
    x[0, :, ::2] = nan
    x[0, :, 1::4] = -inf
    scores = torch.zeros(1, W)
    fin = torch.zeros(1, W, dtype=torch.bool)
    ns, par, tok, nf = [t.cpu() for t in step(x.to(device), scores.to(device), fin.to(device), -1, fill)]
    assert (tok % 4 == 3).all() and torch.isfinite(ns).all()
    # V = 5 with W = 8 on the first step: three empty slots
    V, W = 5, 8
    x = torch.tensor([0.5, 2.0, -1.0, 2.0, 0.0]).view(1, 1, V).expand(1, W, V)
    scores = torch.full((1, W), -inf)
    scores[0, 0] = 0.0
    fin = torch.zeros(1, W, dtype=torch.bool)
    ns, par, tok, nf = [t.cpu() for t in step(x.to(device), scores.to(device), fin.to(device), 1, fill)]
    assert tok[0].tolist() == [1, 3, 0, 4, 2, fill, fill, fill] and par[0].tolist() == [0] * 8
    assert torch.isfinite(ns[0, :5]).all() and (ns[0, 5:] == -inf).all()
    assert nf[0].tolist() == [True] + [False] * 7
    # an all -inf live row has no candidate; a +inf logit gives no NaN score and nothing out of range
    V, W = 3000, 2
    x = 2 * torch.randn(3, W, V, generator=g)
    x[0, 0] = -inf
    x[1, 1, 40] = inf
    x[2] = nan
    scores = torch.tensor([[0.0, -1.0], [-1.0, 0.0], [0.0, 0.0]])
    fin = torch.zeros(3, W, dtype=torch.bool)
    for dtype in (torch.float32, torch.bfloat16):
        ns, par, tok, nf = [t.cpu() for t in step(x.to(dtype).to(device), scores.to(device), fin.to(device), -1, fill)]
        assert not torch.isnan(ns).any()
        assert ((par >= 0) & (par < W)).all() and (((tok >= 0) & (tok < V)) | (tok == fill)).all()
        assert par[0].tolist() == [1, 1] and par[1].tolist() == [0, 0]
        assert (ns[2] == -inf).all() and par[2].tolist() == [0, 0] and tok[2].tolist() == [fill, fill] and not nf[2].any()
