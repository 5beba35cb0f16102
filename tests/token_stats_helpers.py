"""Shared by the ``ops.decode.token_stats`` tests (PyTorch path and kernel): the inputs, a float64
evaluation of the definition that takes nothing from the op but its conditioning rules (NaN -> -inf,
-0 -> +0), and the checks themselves, each taking the function under test (``stats(logits, targets)
-> logp, rank, entropy, top1``) and the device it runs on.

Float bound: ``|got - float64| <= 4 e32 + 2^-23 |value|``, e32 being the largest error of the fp32
PyTorch evaluation (``log_softmax``, ``-sum p log p``) against float64, measured here - for ``logp``
over all V ids of all rows of the case, for ``entropy`` over all rows of all cases of this file."""
import functools
import math

import torch

NINF = float("-inf")
VS = [5, 257, 1000, 4099, 50257]   # NG = 1, 1, 1, 2, 13; 5, 257 and 50257 leave the last group of four partly filled
RS = [1, 3, 70]
# (V, R): the grid above, NG = 16, a V the kernel declines, and more rows than a grid's y dimension takes
CASES = [(V, R) for V in VS for R in RS] + [(65536, 2), (65537, 2), (5, 70000)]
DTYPES = [torch.float32, torch.bfloat16]
ULP = 2.0 ** -23


def strided(x, device):
    """[R, V] values on ``device`` cut from a wider buffer: an odd row stride > V and an offset of one
    element -> (view, the whole buffer)."""
    R, V = x.shape
    sr = V + 5 + V % 2
    flat = torch.full((R * sr + 1,), float("nan"), dtype=x.dtype, device=device)
    view = flat[1:].view(R, sr)[:, :V]
    view.copy_(x)
    assert view.stride() == (sr, 1) and sr % 2 == 1 and view.storage_offset() == 1
    return view, flat


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def case(V, R, dtype=torch.float32):
    """(logits [R, V], targets int64 [R]) on the CPU.  Row 0 targets id 0, row 1 id V - 1, row 2 the
    first id of the last group of four; rows 3, 4 and 5 carry -1, V and 2^40 ("ignore")."""
    g = torch.Generator().manual_seed(104729 * V + 31 * R + (dtype == torch.bfloat16))
    logits = (2 * torch.randn(R, V, generator=g)).to(dtype)
    targets = torch.randint(0, V, (R,), generator=g)
    for r, t in enumerate((0, V - 1, (V - 1) // 4 * 4, -1, V, 2 ** 40)):
        if r < R:
            targets[r] = t
    return logits, targets


def condition(logits):
    """fp32(logit) with NaN -> -inf and -0 -> +0, as float64 on the CPU."""
    s = logits.detach().cpu().float().double()
    return torch.where(torch.isnan(s), NINF, s) + 0.0


def stats64(logits, targets):
    """The definition in float64 -> (logp f64, rank int64, entropy f64, top1 int64), all [R], CPU."""
    s = condition(logits)
    R, V = s.shape
    t = targets.detach().cpu().long().view(R, 1)
    scored = ((t >= 0) & (t < V)).view(R)
    tc = t.clamp(0, V - 1)
    ids = torch.arange(V).view(1, V)
    m = s.amax(-1, keepdim=True)
    st = s.gather(1, tc)
    d = s - m
    p = torch.exp(d)
    Z = p.sum(-1)
    lz = torch.log(Z)
    fin = torch.isfinite(m).view(R)
    nan = torch.full((R,), float("nan"), dtype=torch.float64)
    logp = torch.where(fin, (st - m).view(R) - lz, nan)
    logp = torch.where(scored, logp, torch.zeros(R, dtype=torch.float64))
    ent = torch.where(fin, lz - torch.where(d > NINF, p * d, 0.0).sum(-1) / Z, nan)
    rank = (s > st).sum(-1) + ((s == st) & (ids < tc)).sum(-1)
    rank = torch.where(scored, rank, -1)
    top1 = torch.where(s == m, ids, V).amin(-1)
    return logp, rank, ent, top1


def e32_logp(logits):
    """Largest error of fp32 ``log_softmax`` against float64 over every finite entry of every row."""
    s = condition(logits)
    got = torch.log_softmax(s.float(), -1).double()
    want = torch.log_softmax(s, -1)
    ok = torch.isfinite(want)
    return (got - want)[ok].abs().max().item() if ok.any() else 0.0


def e32_entropy_rows(logits):
    """Error of fp32 ``-sum p log p`` against float64, per row (NaN rows left out)."""
    s = condition(logits)

    def ent(x):
        lsm = torch.log_softmax(x, -1)
        p = torch.exp(lsm)
        return -torch.where(p > 0, p * lsm, 0.0).sum(-1)

    err = (ent(s.float()).double() - ent(s)).abs()
    return err[torch.isfinite(err)]


@functools.lru_cache(maxsize=None)
def e32_entropy():
    """Pooled over all rows of all cases of this file, so that one lucky row does not set the bound."""
    worst = 0.0
    for V, R in CASES:
        for dtype in DTYPES:
            worst = max(worst, e32_entropy_rows(case(V, R, dtype)[0]).max().item())
    for logits in (peaked_rows(), uniform_rows(), mass_rows()):
        worst = max(worst, e32_entropy_rows(logits).max().item())
    return worst


def _to_cpu(out):
    logp, rank, ent, top1 = out
    assert logp.dtype == torch.float32 and ent.dtype == torch.float32, (logp.dtype, ent.dtype)
    assert rank.dtype == torch.int32 and top1.dtype == torch.int32, (rank.dtype, top1.dtype)
    return logp.cpu(), rank.cpu().long(), ent.cpu(), top1.cpu().long()


def assert_matches(got, logits, targets, e_lp, e_en):
    """``got`` (on the CPU) against the float64 evaluation -> the worst float error over its bound."""
    logp, rank, ent, top1 = got
    R, V = logits.shape
    wl, wr, we, wt = stats64(logits, targets)
    assert logp.shape == rank.shape == ent.shape == top1.shape == (R,)
    assert torch.equal(rank, wr), (rank[rank != wr][:8], wr[rank != wr][:8])
    assert torch.equal(top1, wt), (top1[top1 != wt][:8], wt[top1 != wt][:8])
    t = targets.cpu().long()
    scored = (t >= 0) & (t < V)
    assert torch.equal(rank == 0, scored & (top1 == t))
    assert (rank < V).all() and (rank[scored] >= 0).all() and (rank[~scored] == -1).all()
    assert (logp[~scored] == 0).all()
    worst = 0.0
    for name, g, w, e in (("logp", logp, wl, e_lp), ("entropy", ent, we, e_en)):
        g = g.double()
        assert torch.equal(torch.isnan(g), torch.isnan(w)), name
        assert torch.equal(torch.isinf(g), torch.isinf(w)) and (g[torch.isinf(w)] == w[torch.isinf(w)]).all(), name
        ok = torch.isfinite(w)
        if ok.any():
            ratio = ((g - w).abs() / (4 * e + ULP * w.abs()).clamp(min=1e-300))[ok].max().item()
            assert ratio <= 1.0, (name, ratio, e)
            worst = max(worst, ratio)
    ok = ~torch.isnan(logp)
    assert (logp[ok] <= 0).all()
    ok = ~torch.isnan(ent)
    assert (ent[ok] >= -4 * e_en).all()
    return worst


def check_case(stats, device, V, R, dtype):
    """Contiguous logits with int64 targets, and the same values cut from a wider buffer with strided
    int32 targets: both against float64, equal to each other bit for bit, nothing else written."""
    logits, targets = case(V, R, dtype)
    e_lp, e_en = e32_logp(logits), e32_entropy()
    x = logits.to(device)
    t = targets.to(device)
    before = _bits(x).clone()
    first = _to_cpu(stats(x, t))
    assert torch.equal(_bits(x), before) and torch.equal(t.cpu(), targets)
    worst = assert_matches(first, logits, targets, e_lp, e_en)

    view, flat = strided(logits, device)
    wide = torch.full((R, 3), 7, dtype=torch.int32, device=device)
    t32 = wide[:, 1]
    t32.copy_(torch.where(targets > 2 ** 31 - 1, -5, targets).to(torch.int32))  # int32 cannot hold 2^40
    assert t32.stride() == (3,)
    before, tbefore = _bits(flat).clone(), wide.cpu().clone()
    second = _to_cpu(stats(view, t32))
    assert torch.equal(_bits(flat), before) and torch.equal(wide.cpu(), tbefore)  # the whole buffers
    for a, b in zip(first, second):
        assert torch.equal(_bits(a) if a.is_floating_point() else a, _bits(b) if b.is_floating_point() else b)
    again = _to_cpu(stats(x, t))
    for a, b in zip(first, again):
        assert a.numpy().tobytes() == b.numpy().tobytes()  # two calls agree bit for bit
    return e_lp, e_en, worst


def check_ties(stats, device):
    """Exact by construction: rows of the values {0, 1, 2} alone, the target inside a run of equals,
    the maximum held by many ids; and bf16 rows, where ties arise by themselves."""
    for V in (257, 4099, 50257):
        g = torch.Generator().manual_seed(V)
        x = torch.randint(0, 3, (6, V), generator=g).float()
        t = torch.tensor([V // 2, V // 3, V - 9, 9, V // 2 + 1, 2 * V // 3])
        ids = torch.arange(V).view(1, V)
        same = x == x.gather(1, t.view(-1, 1))
        assert ((same & (ids < t.view(-1, 1))).sum(-1) > 0).all() and ((same & (ids > t.view(-1, 1))).sum(-1) > 0).all()
        assert ((x == 2).sum(-1) > 1).all()
        for dtype in DTYPES:
            logp, rank, ent, top1 = _to_cpu(stats(x.to(dtype).to(device), t.to(device)))
            wl, wr, we, wt = stats64(x, t)
            assert torch.equal(rank, wr) and torch.equal(top1, wt)
            assert torch.equal(top1, (x == 2).long().argmax(-1))  # the lowest id holding the maximum
    x = (2 * torch.randn(5, 4099, generator=torch.Generator().manual_seed(5))).bfloat16()
    assert all(len(set(row.tolist())) < 4099 // 2 for row in x.float())  # bf16: many equal logits
    t = torch.tensor([7, 1000, 4098, 2048, 0])
    logp, rank, ent, top1 = _to_cpu(stats(x.to(device), t.to(device)))
    wl, wr, we, wt = stats64(x, t)
    assert torch.equal(rank, wr) and torch.equal(top1, wt)


@functools.lru_cache(maxsize=None)
def peaked_rows():
    x = torch.randn(3, 4099, generator=torch.Generator().manual_seed(11))
    x[torch.arange(3), torch.tensor([0, 2047, 4098])] += 100.0
    return x


@functools.lru_cache(maxsize=None)
def uniform_rows():
    return torch.full((2, 50257), -1.375)


@functools.lru_cache(maxsize=None)
def mass_rows():
    row = 2 * torch.randn(1, 257, generator=torch.Generator().manual_seed(13))
    return row.expand(257, 257).contiguous()


def check_invariants(stats, device):
    e_en = e32_entropy()
    # a peaked row: entropy and logp(peak) are 0 within the bound
    x = peaked_rows()
    t = torch.tensor([0, 2047, 4098])
    e_lp = e32_logp(x)
    logp, rank, ent, top1 = _to_cpu(stats(x.to(device), t.to(device)))
    assert torch.equal(top1, t) and (rank == 0).all()
    assert (logp.abs() <= 4 * e_lp).all() and (ent.abs() <= 4 * e_en).all(), (logp, ent, e_lp, e_en)
    # V equal logits: entropy = -logp = log V
    x = uniform_rows()
    V = x.shape[1]
    t = torch.tensor([0, V - 1])
    e_lp = e32_logp(x)
    logp, rank, ent, top1 = _to_cpu(stats(x.to(device), t.to(device)))
    assert rank.tolist() == [0, V - 1] and top1.tolist() == [0, 0]
    lv = math.log(V)
    assert ((-logp.double() - lv).abs() <= 4 * e_lp + ULP * lv).all(), (logp, lv, e_lp)
    assert ((ent.double() - lv).abs() <= 4 * e_en + ULP * lv).all(), (ent, lv, e_en)
    # exp(logp) over all V targets of one row sums to 1
    x = mass_rows()
    V = x.shape[1]
    e_lp = e32_logp(x[:1])
    logp, rank, ent, top1 = _to_cpu(stats(x.to(device), torch.arange(V, device=device)))
    assert abs(torch.exp(logp.double()).sum().item() - 1.0) <= V * 4 * e_lp, (e_lp,)
    assert sorted(rank.tolist()) == list(range(V))  # the ranks of one row's ids are a permutation
    return e_en


def check_nonfinite(stats, device):
    inf, nan = float("inf"), float("nan")
    V = 1000
    g = torch.Generator().manual_seed(17)
    x = 2 * torch.randn(6, V, generator=g)
    x[0, ::2] = -inf                 # -inf entries, a finite target: a finite entropy
    x[1, 1::2] = -inf                # the target itself at -inf
    x[2, ::3] = nan                  # NaN counts as -inf
    x[3] = -inf                      # all -inf
    x[4, 40] = inf                   # a +inf
    x[5, 5] = -0.0                   # -0 is +0: it ties with the +0 next to it
    x[5, 6] = 0.0
    t = torch.tensor([1, 501, 300, 7, 40, 6])
    for dtype in DTYPES:
        xd = x.to(dtype)
        logp, rank, ent, top1 = got = _to_cpu(stats(xd.to(device), t.to(device)))
        assert_matches(got, xd, t, e32_logp(xd), e32_entropy())
        assert torch.isfinite(ent[:3]).all() and torch.isfinite(logp[0])
        assert logp[1] == -inf and int(rank[1]) == V // 2 + 250  # the finite ids, then the -inf ids below 501
        assert logp[2] == -inf and int(rank[2]) == (V - 334) + 100
        assert torch.isnan(logp[3:5]).all() and torch.isnan(ent[3:5]).all()
        assert int(rank[3]) == 7 and int(top1[3]) == 0 and int(rank[4]) == 0 and int(top1[4]) == 40
    # an ignored target on degenerate rows: logp 0, not NaN
    logp, rank, ent, top1 = _to_cpu(stats(x[3:5].to(device), torch.tensor([-1, V]).to(device)))
    assert (logp == 0).all() and (rank == -1).all() and torch.isnan(ent).all() and top1.tolist() == [0, 40]


def check_against_ref(stats, ref, device, V, R, dtype):
    """Two paths on one device: integers equal, floats within the bound of each other's float64."""
    logits, targets = case(V, R, dtype)
    x, t = logits.to(device), targets.to(device)
    a, b = _to_cpu(stats(x, t)), _to_cpu(ref(x, t))
    assert torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for g, w, e in ((a[0], b[0], e32_logp(logits)), (a[2], b[2], e32_entropy())):
        assert ((g.double() - w.double()).abs() <= 2 * (4 * e + ULP * w.double().abs())).all()
