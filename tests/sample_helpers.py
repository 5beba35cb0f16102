"""Shared by the ``ops.decode.sample_tokens`` tests (CPU path and kernel): the inputs, a float64
yardstick of the definition that is independent of the op, and the checks themselves, each taking
the device it runs on.

The yardstick takes ``s = fp32(logit) / fp32(temperature)`` (numpy's float32 division) and does
everything else in float64 on the uniforms ``sample_uniforms`` returns."""
import functools
import math

import numpy as np
import torch

from distributed_pipeline_amd.ops.decode import sample_tokens, sample_uniforms

VS = [8, 257, 1000, 4099, 50257]
BS = [1, 3, 70]
SHAPES = [(V, B) for V in VS for B in BS]
# every pairing of dtype and layout, both temperatures, at every shape
CONFIGS = [(torch.float32, "contig", 0.7), (torch.bfloat16, "cut", 1.3), (torch.float32, "cut", 1.3),
           (torch.bfloat16, "contig", 0.7)]
SEED, STEP, ROW_BASE = 2 ** 40 + 7, 3, 5

DELTA = 1e-4   # top-p sandwich: see test_top_p_sandwich's docstring in the test files
EPS = 1e-4     # the draw: four times the 1.2e-5 bound on one perturbed score, across two scores, rounded up


@functools.lru_cache(maxsize=None)
def _logits_cpu(V, B, dtype):
    g = torch.Generator().manual_seed(1000 * V + B)
    # randn * 3, clipped so that |s| <= 64 at the smaller temperature
    return (torch.randn(B, V, generator=g) * 3).clamp(-44.8, 44.8).to(dtype)


def layout(x, kind, device):
    """``x`` on ``device``: contiguous, or rows cut out of a wider buffer (odd row stride, storage
    offset of one element)."""
    x = x.to(device)
    if kind == "contig":
        return x.contiguous()
    B, V = x.shape
    stride = (V + 3) | 1
    flat = torch.full((B * stride + 1,), float("nan"), dtype=x.dtype, device=device)
    view = flat[1:].view(B, stride)[:, :V]
    view.copy_(x)
    assert view.stride() == (stride, 1) and view.storage_offset() == 1 and stride % 2 == 1
    return view


def inputs(V, B, dtype, kind, device):
    return layout(_logits_cpu(V, B, dtype), kind, device)


def scaled(logits, temperature):
    """s as float32 numpy [B, V]: fp32 division, NaN -> -inf."""
    s = logits.detach().float().cpu().numpy() / np.float32(temperature)
    assert s.dtype == np.float32
    return np.where(np.isnan(s), np.float32(-np.inf), s)


@functools.lru_cache(maxsize=2)
def sorted64(V, B, dtype, temperature):
    """(s, s sorted in descending order) of the standard inputs as float64."""
    s = scaled(_logits_cpu(V, B, dtype), temperature).astype(np.float64)
    return s, -np.sort(-s, axis=-1)


class Yardstick:
    """float64 evaluation of steps 3-5 of the definition for one [B, V] array of s."""

    def __init__(self, s, srt, top_k):
        self.s, self.srt = s, srt
        B, V = self.s.shape
        self.kappa = self.srt[:, top_k - 1] if 0 < top_k < V else self.srt[:, -1]
        w = np.where(self.srt >= self.kappa[:, None], np.exp(self.srt - self.srt[:, :1]), 0.0)
        cs = np.cumsum(w, axis=-1)
        self.Z = cs[:, -1]
        # mass strictly above each sorted position: the sum in front of the first element of its run
        self.above = np.empty_like(cs)
        for b in range(B):
            first = np.searchsorted(-self.srt[b], -self.srt[b], side="left")
            self.above[b] = np.where(first > 0, cs[b, first - 1], 0.0)

    def tau(self, p):
        """tau64(p) per row (p outside (0, 1): top-p off)."""
        if not 0.0 < p < 1.0:
            return self.kappa
        keep = (self.above < p * self.Z[:, None]) & (self.srt >= self.kappa[:, None])
        n = keep.sum(-1)
        assert (n >= 1).all()
        return self.srt[np.arange(len(n)), n - 1]

    def count(self, thr):
        return (self.s >= np.asarray(thr, dtype=np.float64)[:, None]).sum(-1)


def yardstick(V, B, dtype, temperature, top_k):
    return Yardstick(*sorted64(V, B, dtype, temperature), top_k)


def yardstick_of(x, temperature, top_k):
    s = scaled(x, temperature).astype(np.float64)
    return Yardstick(s, -np.sort(-s, axis=-1), top_k)


@functools.lru_cache(maxsize=None)
def uniforms64(V, B, device):
    """The uniforms of the standard (SEED, STEP, ROW_BASE) call as float64 numpy."""
    return sample_uniforms(SEED, STEP, ROW_BASE, B, V, device).cpu().numpy().astype(np.float64)


def run(x, temperature, top_k=0, top_p=0.0, **kw):
    kw = {"seed": SEED, "step": STEP, "row_base": ROW_BASE, **kw}
    tok, thr, kept = sample_tokens(x, temperature=temperature, top_k=top_k, top_p=top_p, return_stats=True, **kw)
    B = x.shape[0]
    assert tok.dtype == torch.int64 and thr.dtype == torch.float32 and kept.dtype == torch.int32
    assert tok.shape == thr.shape == kept.shape == (B,) and tok.device == x.device
    return tok.cpu().numpy(), thr.cpu().numpy(), kept.cpu().numpy()


def assert_valid_draw(tok, thr, s32, u64, what=""):
    """Test 4: s_tok >= thr and the token's float64 perturbed score is within EPS of the float64
    maximum over {s >= thr}."""
    s = s32.astype(np.float64)
    B, V = s.shape
    assert ((tok >= 0) & (tok < V)).all(), what
    rows = np.arange(B)
    assert (s32[rows, tok] >= thr).all(), what
    score = np.where(s >= thr.astype(np.float64)[:, None], s - np.log(-np.log(u64)), -np.inf)
    gap = score.max(-1) - score[rows, tok]
    assert (gap <= EPS).all(), (what, float(gap.max()))
    return gap


# ---- the checks, each on one device ----------------------------------------------------------

def check_top_k_exact(V, B, device):
    for dtype, kind, T in CONFIGS:
        x = inputs(V, B, dtype, kind, device)
        s, srt = sorted64(V, B, dtype, T)
        for k in sorted({1, 2, min(50, V - 1), V - 1}):
            kappa = srt[:, k - 1]  # comparisons only: exact in any precision
            tok, thr, kept = run(x, T, top_k=k)
            assert np.array_equal(thr.astype(np.float64), kappa), (dtype, kind, k)
            assert np.array_equal(kept, (s >= kappa[:, None]).sum(-1)) and (kept >= k).all(), (dtype, kind, k)
        # V, V + 3 and 0: off - everything is kept and thr is the row's minimum
        for k in (0, V, V + 3):
            tok, thr, kept = run(x, T, top_k=k)
            assert np.array_equal(thr.astype(np.float64), srt[:, -1]) and (kept == V).all(), (dtype, kind, k)


def check_top_k_ties(device):
    x = torch.tensor([[1.0, 5.0, 5.0, -2.0, 5.0, 0.5, 5.0, 3.0, 3.0]], device=device)
    tok, thr, kept = run(x, 1.0, top_k=2)
    assert kept.tolist() == [4] and thr.tolist() == [5.0] and tok[0] in (1, 2, 4, 6)
    tok, thr, kept = run(x, 1.0, top_k=5)
    assert kept.tolist() == [6] and thr.tolist() == [3.0]


def check_top_p_sandwich(V, B, device):
    for dtype, kind, T in CONFIGS:
        x = inputs(V, B, dtype, kind, device)
        for k in (0, 50):
            y = yardstick(V, B, dtype, T, k)
            for p in (0.1, 0.5, 0.9, 0.999):
                tok, thr, kept = run(x, T, top_k=k, top_p=p)
                lo, hi = y.tau(p + DELTA), y.tau(p - DELTA)
                t64 = thr.astype(np.float64)
                bad = ~((lo <= t64) & (t64 <= hi))
                assert not bad.any(), (dtype, kind, k, p, int(bad.sum()), lo[bad][:3], t64[bad][:3], hi[bad][:3])
                assert np.array_equal(kept, y.count(thr)), (dtype, kind, k, p)


def check_top_p_pinned(device):
    ln2 = math.log(2.0)
    # masses 1, 1/2, .., 1/128 of Z = 255/128: the mass above the k-th is (2 - 2^(1-k)); 0.8 Z = 1.59375
    # lies strictly between the mass above the 3rd (1.5) and above the 4th (1.75), far from rounding
    x = torch.tensor([[-k * ln2 for k in range(8)]], device=device)
    assert run(x, 1.0, top_p=0.8)[2].tolist() == [3]
    for V in (5, 1000, 4099):
        for p in (0.01, 0.5, 0.99):
            x = torch.full((2, V), 1.25, device=device)
            tok, thr, kept = run(x, 0.7, top_p=p)
            assert kept.tolist() == [V, V] and thr.tolist() == [np.float32(1.25) / np.float32(0.7)] * 2
    x = torch.randn(3, 1000, generator=torch.Generator().manual_seed(3)).to(device)
    x[:, 417] = 40.0
    for p in (0.1, 0.9, 0.999):
        tok, thr, kept = run(x, 1.0, top_p=p)
        assert kept.tolist() == [1, 1, 1] and tok.tolist() == [417] * 3 and thr.tolist() == [40.0] * 3


def check_draw(V, B, device):
    worst = 0.0
    for dtype, kind, T in CONFIGS:
        x = inputs(V, B, dtype, kind, device)
        s32 = scaled(_logits_cpu(V, B, dtype), T)
        u = uniforms64(V, B, device)
        for k, p in ((0, 0.0), (50, 0.0), (0, 0.9), (50, 0.9)):
            tok, thr, kept = run(x, T, top_k=k, top_p=p)
            worst = max(worst, assert_valid_draw(tok, thr, s32, u, (dtype, kind, T, k, p)).max())
    return worst


def check_batch_independence(device):
    V = 4099
    for dtype in (torch.float32, torch.bfloat16):
        x = inputs(V, 70, dtype, "contig", device)[:12]
        kw = dict(top_k=50, top_p=0.9)
        full = run(x, 0.7, row_base=0, **kw)
        part = run(x[5:9], 0.7, row_base=5, **kw)
        for a, b in zip(full, part):
            assert a[5:9].tobytes() == b.tobytes()  # bit for bit
        again = run(x, 0.7, row_base=0, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))
    x = inputs(V, 70, torch.float32, "contig", device)
    base = run(x, 0.7)[0]
    assert not np.array_equal(base, run(x, 0.7, step=STEP + 1)[0])
    assert not np.array_equal(base, run(x, 0.7, seed=SEED + 1)[0])
    assert not np.array_equal(base, run(x, 0.7, seed=SEED + 2 ** 32)[0])
    assert not np.array_equal(base, run(x, 0.7, row_base=ROW_BASE + 1)[0])


# 1 - 1e-4 quantiles of the chi-squared distribution by degrees of freedom
CHI2_Q9999 = {1: 15.137, 2: 18.421, 3: 21.108, 4: 23.513}
DIST_ROW = [1.0, 0.2, -0.5, 2.0, 0.0, -3.0, 0.7, 1.5]


def check_distribution(device):
    """V = 8, one row repeated 4096 times, top_k = 5 and top_p = 0.9 -> the chi-squared statistic of
    the counts against the filtered softmax."""
    N = 4096
    x = torch.tensor([DIST_ROW], device=device).expand(N, 8).contiguous()
    tok, thr, kept = run(x, 1.0, top_k=5, top_p=0.9, seed=20240, step=0, row_base=0)
    y = yardstick_of(x[:1], 1.0, 5)
    tau = y.tau(0.9)[0]
    keep = y.s[0] >= tau
    assert (kept == keep.sum()).all() and (thr == np.float32(tau)).all()
    counts = np.bincount(tok, minlength=8)
    assert counts[~keep].sum() == 0  # no dropped id is ever drawn
    w = np.where(keep, np.exp(y.s[0]), 0.0)
    expect = N * w / w.sum()
    stat = float((((counts - expect) ** 2)[keep] / expect[keep]).sum())
    return stat, CHI2_Q9999[int(keep.sum()) - 1], int(keep.sum())


def check_degenerate(device):
    from utils.lm_sampling import greedy
    inf, nan = float("inf"), float("nan")
    g = torch.Generator().manual_seed(4)
    for V in (8, 1000, 4099):
        base = torch.randn(V, generator=g)
        rows = {"all -inf": torch.full((V,), -inf), "all nan": torch.full((V,), nan), "+inf": base.clone(),
                "two +inf": base.clone(), "nan among finite": base.clone(), "nan and -inf": torch.full((V,), -inf)}
        rows["+inf"][V - 3] = inf
        rows["two +inf"][[V // 2, V - 1]] = inf
        rows["two +inf"][0] = nan
        rows["nan among finite"][::2] = nan     # every even id
        rows["nan and -inf"][1::2] = nan
        x = torch.stack(list(rows.values())).to(device)
        for dtype in (torch.float32, torch.bfloat16):
            xd = x.to(dtype)
            want = greedy(xd).cpu().numpy()
            for k, p in ((0, 0.0), (3, 0.0), (0, 0.5), (3, 0.5)):
                tok, thr, kept = run(xd, 0.7, top_k=k, top_p=p)
                assert ((tok >= 0) & (tok < V)).all()
                for i, name in enumerate(rows):
                    if name == "nan among finite":
                        assert tok[i] % 2 == 1 and kept[i] >= 1, (name, k, p)  # a NaN never wins
                        # without a filter the NaNs, as -inf, are kept (and cannot win); a filter drops them
                        assert (kept[i] == V and thr[i] == -inf) if (k, p) == (0, 0.0) else np.isfinite(thr[i])
                    else:
                        assert tok[i] == want[i] and kept[i] == 0, (name, k, p)
                        assert thr[i] == (inf if "+inf" in name else -inf), name
