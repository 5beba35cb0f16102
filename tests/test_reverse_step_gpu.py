"""The fused reverse-step kernel (csrc/reverse_step.hip) through ``ops.diffusion.reverse_step``:
formula against float64, bf16 copy, kept source rows, the noise contract (batch independence,
64-bit counter, s == 0) and the statistics of the plain and the truncated noise."""
import math

import pytest
import torch

from distributed_pipeline_amd.ops import diffusion as dops
from distributed_pipeline_amd.ops._ext import get_ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -24


def _noise(shape, **kw):
    """z of the kernel: a = b = 0, s = 1 under an all-ones mask."""
    ones = torch.ones(shape[:-1], dtype=torch.long, device=DEV)
    xs = torch.zeros(shape, device=DEV)
    args = dict(seed=7, step=3, row_base=0, top_p=0.0)
    args.update(kw)
    return dops.reverse_step(None, x_start=xs, mask=ones, a=0.0, b=0.0, s=1.0, **args)[0]


@pytest.fixture()
def ext_calls(monkeypatch):
    """Counts the extension's reverse_step launches: every case here must take the kernel."""
    ext = get_ext(required=True)
    calls = []
    real = ext.reverse_step
    monkeypatch.setattr(ext, "reverse_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("top_p", [0.0, 0.9])
@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("B,L,E", [(3, 20, 16), (1, 77, 128)])
def test_formula_against_float64(ext_calls, B, L, E, rounded, top_p):
    g = torch.Generator().manual_seed(B * 1000 + E)
    V = 50
    x = torch.randn(B, L, E, generator=g).to(DEV)
    xs = torch.randn(B, L, E, generator=g).to(DEV)
    mask = (torch.rand(B, L, generator=g) < 0.6).long().to(DEV)  # boundaries inside a wave
    a, b, s = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.37, 0.61, 0.23))
    kw = dict(x_start=xs, mask=mask, a=a, b=b, s=s, seed=7, step=3, row_base=5, top_p=top_p)
    if rounded:
        W = torch.randn(V, E, generator=g).to(DEV)
        idx = torch.randint(0, V, (B, L), generator=g)
        idx[0, :4] = torch.tensor([-1, V, V + 7, -(2 ** 40)])  # out of range: a zero row
        idx = idx.to(DEV)
        ok = ((idx >= 0) & (idx < V)).unsqueeze(-1)
        x0 = 2.5 * W.double()[idx.clamp(0, V - 1)] * ok
        out, out16 = dops.reverse_step(x, idx=idx, weight=W, scale=2.5, want_bf16=True, **kw)
    else:
        pred = torch.randn(B, L, E, generator=g).to(DEV).to(torch.bfloat16)
        x0 = pred.double()
        out, out16 = dops.reverse_step(x, pred=pred, want_bf16=True, **kw)
    z = _noise((B, L, E), row_base=5, top_p=top_p).double()
    assert len(ext_calls) == 2
    assert out.dtype == torch.float32 and out.shape == (B, L, E) and out16.dtype == torch.bfloat16
    t0, t1, t2 = a * x0, b * x.double(), s * z
    ref = t0 + t1 + t2
    bound = 4 * EPS * (t0.abs() + t1.abs() + t2.abs())
    tgt = mask.unsqueeze(-1).expand(B, L, E) != 0
    err = (out.double() - ref).abs()
    print(f"max err / bound on the target rows: {float((err / bound.clamp_min(1e-300))[tgt].max()):.3f}")
    assert bool((err <= bound)[tgt].all())
    assert torch.equal(out[~tgt], xs[~tgt])              # source rows: x_start, bit for bit
    assert torch.equal(out16, out.to(torch.bfloat16))    # round to nearest even
    if rounded:
        bad = (~ok).expand(B, L, E) & tgt
        assert int(bad.sum()) > 0 or int(mask[0, :4].sum()) == 0
        e = (out.double() - (t1 + t2)).abs()
        assert bool((e <= 4 * EPS * (t1.abs() + t2.abs()))[bad].all())
    # without the optional outputs / inputs
    out_b, none = dops.reverse_step(x, pred=None if rounded else pred, idx=idx if rounded else None,
                                    weight=W if rounded else None, scale=2.5, **kw)
    assert none is None and torch.equal(out_b, out)


def test_batch_independence_and_keys(ext_calls):
    E = 128
    full = _noise((64, E))
    for r0, r1 in ((0, 7), (7, 40), (40, 64)):
        part = _noise((r1 - r0, E), row_base=r0)
        assert torch.equal(part, full[r0:r1])
    # as one [B, L, E] batch or as rows: the same bits
    assert torch.equal(_noise((4, 16, E)).view(64, E), full)
    for other in (dict(seed=8), dict(step=4), dict(row_base=1), dict(seed=7 + 2 ** 32)):
        assert float((_noise((64, E), **other) - full).abs().mean()) > 0.5
    assert len(ext_calls) == 9


def test_group_counter_is_64_bit(ext_calls):
    """E = 128: the group index of row_base = 2^27 is 2^32, whose low word is that of row 0."""
    E = 128
    lo = _noise((8, E), row_base=0)
    hi = _noise((8, E), row_base=2 ** 27)
    assert float((hi - lo).abs().mean()) > 0.5
    assert bool(torch.isfinite(hi).all())


def test_s_zero_reads_no_noise(ext_calls):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 9, 32, generator=g).to(DEV)
    pred = torch.randn(2, 9, 32, generator=g).to(DEV).to(torch.bfloat16)
    run = lambda seed: dops.reverse_step(x, pred=pred, a=0.5, b=0.25, s=0.0, seed=seed, step=0)[0]  # noqa: E731
    assert torch.equal(run(1), run(2))
    assert torch.equal(run(1), 0.5 * pred.float() + 0.25 * x)  # exact: powers of two, no mask
    assert len(ext_calls) == 3


def test_plain_noise_statistics(ext_calls):
    z = _noise((64, 128, 128)).double()
    n = z.numel()
    assert n == 1 << 20
    print(f"mean {float(z.mean()):.2e} std {float(z.std()):.6f}")
    assert abs(float(z.mean())) < 6e-3          # 6 / sqrt(n)
    assert abs(float(z.std()) - 1.0) < 5e-3     # 6 / sqrt(2 n), rounded up
    assert float(z.abs().max()) > 4.0           # the tails are there


@pytest.mark.parametrize("tau,var", [(0.9, 0.24202), (2.0, 0.77374)])
def test_truncated_noise_statistics(ext_calls, tau, var):
    z = _noise((64, 128, 128), top_p=tau).double()
    n = z.numel()
    phi = math.exp(-0.5 * tau * tau) / math.sqrt(2 * math.pi)
    assert abs(1 - 2 * tau * phi / math.erf(tau / math.sqrt(2)) - var) < 1e-5
    print(f"tau {tau}: max|z| {float(z.abs().max()):.6f} mean {float(z.mean()):.2e} var {float(z.var()):.5f}")
    assert float(z.abs().max()) <= tau
    assert float(z.abs().max()) > 0.999 * tau
    assert abs(float(z.mean())) < 6 * math.sqrt(var / n)
    assert abs(float(z.var()) / var - 1) < 0.01
    assert len(ext_calls) == 1
