"""csrc/linear_argmax.hip against a float64 reference.

Reference: the operands are rounded to bf16 and S = x W^T + c is computed in float64 from those
rounded values - exactly what the kernel reads (in ``nearest`` mode c is the float64
-1/2 ||w||^2 of the bf16 W).  The kernel's products are exact in fp32, so only its summation
order differs from the reference; per entry that is bounded by

    tau[n, v] = (E + 2) * 2^-23 * (sum_k |x_nk| |w_vk| + |c_v|).

Checks, for the logits and the nearest mode on x = randn, W = 0.5 randn (seed 0):
 1. every index is in [0, V);
 2. S[n, idx_n] >= max_v S[n, v] - tau[n, idx_n] on every row;
 3. ``best`` agrees with S[n, idx_n] within tau[n, idx_n];
 4. idx_n is the reference arg-max on every row whose reference top-2 gap exceeds 2 tau_n, with
    tau_n = max_v tau[n, v] (then no other row of W can overtake the winner under any
    summation order); the rows this leaves out must be <= 2 % of all rows.
"""
import pytest
import torch

from distributed_pipeline_amd.ops import nn as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (N, V, E): partial token block + partial last W tile | E = 256, V no multiple of 64 | the real
# vocabulary, many splits on a 2-D grid | 8 splits, the one-split-per-XCD 1-D grid | one token
# block past the no-split threshold (1024 blocks): a single sweep of the vocabulary | one token |
# E = 256 on the one-split-per-XCD 1-D grid, partial last token block
SHAPES = [(300, 1000, 128), (130, 517, 256), (4096, 30522, 128), (16384, 1000, 128), (131000, 500, 128),
          (1, 1000, 128), (16400, 1000, 256)]
_CACHE = {}


def _problem(N, V, E):
    """bf16 operands, a bias, and the float64 pieces of the reference; built once per shape."""
    key = (N, V, E)
    if key not in _CACHE:
        _CACHE.clear()  # one shape's float64 matrices at a time
        g = torch.Generator(device=DEV).manual_seed(0)
        x = torch.randn(N, E, device=DEV, generator=g).bfloat16()
        W = (0.5 * torch.randn(V, E, device=DEV, generator=g)).bfloat16()
        bias = torch.randn(V, device=DEV, generator=g)
        x64, W64 = x.double(), W.double()
        P = x64 @ W64.t()
        A = x64.abs() @ W64.abs().t()
        _CACHE[key] = (x, W, bias, P, A, -0.5 * (W64 * W64).sum(-1))
    return _CACHE[key]


def _reference(N, V, E, mode):
    x, W, bias, P, A, hsq = _problem(N, V, E)
    c64 = hsq if mode == "nearest" else bias.double()
    S = P + c64
    tau = (E + 2) * 2.0 ** -23 * (A + c64.abs())
    return x, W, bias, S, tau


def _check(idx, best, S, tau, V, check_best=True, max_left_out=0.02):
    N = S.shape[0]
    assert idx.shape == (N,) and idx.dtype == torch.int64
    assert int(idx.min()) >= 0 and int(idx.max()) < V                                   # 1
    rows = torch.arange(N, device=S.device)
    s_at, t_at = S[rows, idx], tau[rows, idx]
    top2 = S.topk(2, dim=-1)
    short = top2.values[:, 0] - s_at - t_at
    print(f"  max(top - S[idx] - tau) = {float(short.max()):.3e}")
    assert bool((short <= 0).all())                                                      # 2
    if check_best:
        err = (best.double() - s_at).abs() - t_at
        print(f"  max(|best - S[idx]| - tau) = {float(err.max()):.3e}")
        assert best.dtype == torch.float32 and bool((err <= 0).all())                    # 3
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * tau.amax(-1)
    left_out = 1.0 - float(clear.double().mean())
    print(f"  rows left out of the exact-index check: {100 * left_out:.3f} %")
    assert max_left_out is None or left_out <= max_left_out                              # 4
    assert torch.equal(idx[clear], top2.indices[:, 0][clear])


def _run(x, W, bias, mode, **kw):
    assert ops._argmax_native(x, W), "the HIP kernel must be the path under test"
    return ops.linear_argmax(x, W, bias if mode == "logits" else None, nearest=mode == "nearest", **kw)


@pytest.mark.parametrize("mode", ["logits", "nearest"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(shape, mode):
    N, V, E = shape
    x, W, bias, S, tau = _reference(N, V, E, mode)
    idx, best = _run(x, W, bias, mode)
    if N == 1:  # the 2 % allowance is a statement about many rows; one row must simply be clear
        assert float(S.topk(2).values[0, 0] - S.topk(2).values[0, 1]) > 2 * float(tau.max())
    _check(idx, best, S, tau, V)


@pytest.mark.parametrize("mode", ["logits", "nearest"])
@pytest.mark.parametrize("shape", SHAPES[:5], ids=lambda s: "x".join(map(str, s)))
def test_fallback_path_agrees(shape, mode):
    """The PyTorch path of ops.linear_argmax (taken for fp32 input) on the same inputs: checks 1, 2, 4."""
    N, V, E = shape
    x, W, bias, S, tau = _reference(N, V, E, mode)
    xf, Wf = x.float(), W.float()
    assert not ops._argmax_native(xf, Wf)
    idx, best = ops.linear_argmax(xf, Wf, bias if mode == "logits" else None, nearest=mode == "nearest")
    _check(idx, best, S, tau, V, check_best=False)


def test_precomputed_offsets_and_row_half_sqnorm():
    x, W, _, S, tau = _reference(300, 1000, 128, "nearest")
    c = ops.row_half_sqnorm(W)
    assert c.dtype == torch.float32 and c.shape == (1000,)
    hsq = -0.5 * (W.double() ** 2).sum(-1)
    assert bool(((c.double() - hsq).abs() <= 128 * 2.0 ** -24 * hsq.abs()).all())
    idx, best = ops.linear_argmax(x, W, c=c)
    idx2, best2 = ops.linear_argmax(x, W, nearest=True)
    assert torch.equal(idx, idx2) and torch.equal(best, best2)
    W256 = (0.5 * torch.randn(517, 256, device=DEV)).bfloat16()
    h256 = -0.5 * (W256.double() ** 2).sum(-1)
    assert bool(((ops.row_half_sqnorm(W256).double() - h256).abs() <= 256 * 2.0 ** -24 * h256.abs()).all())


def test_empty_input_launches_nothing():
    W = torch.randn(1000, 128, device=DEV).bfloat16()
    x = torch.empty(0, 128, device=DEV, dtype=torch.bfloat16)
    for kw in ({}, {"nearest": True}):
        idx, best = ops.linear_argmax(x, W, **kw)
        assert idx.shape == (0,) and idx.dtype == torch.int64 and idx.device.type == "cuda"
        assert best.shape == (0,) and best.dtype == torch.float32


@pytest.mark.parametrize("N,E", [(130, 256), (131000, 128)], ids=["split", "single_sweep"])
def test_zero_padded_rows_never_win(N, E):
    """V = 517: the last W tile is padded with zero rows, which would score 0; every true score
    is negative (bias -5, |x . w| << 5), so a padded row would win if it were not masked."""
    V = 517
    g = torch.Generator(device=DEV).manual_seed(1)
    x = (0.01 * torch.randn(N, E, device=DEV, generator=g)).bfloat16()
    W = (0.5 * torch.randn(V, E, device=DEV, generator=g)).bfloat16()
    bias = torch.full((V,), -5.0, device=DEV)
    S = x.double() @ W.double().t() + bias.double()
    assert float(S.max()) < 0
    idx, best = _run(x, W, bias, "logits")
    assert int(idx.max()) < V and int(idx.min()) >= 0
    tau = (E + 2) * 2.0 ** -23 * (x.double().abs() @ W.double().abs().t() + 5.0)
    # equal to the reference wherever the reference decides (scores this close together - x is
    # small on purpose - leave more than the usual share of rows undecided: no share bound here)
    _check(idx, best, S, tau, V, max_left_out=None)
    assert bool((best < 0).all())


@pytest.mark.parametrize("N,V", [(5, 1000), (4096, 30522), (131000, 500)],
                         ids=["tile_per_split", "multi_tile_splits", "single_sweep"])
@pytest.mark.parametrize("mode", ["logits", "nearest"])
def test_ties_go_to_the_lowest_index(N, V, mode):
    """Row 3 of W copied to rows 64 k + 5 (other tiles and, on the split paths, other splits), to
    row 7 (same tile, the other lane half) and row 40 (same tile, the second 32-row subtile);
    every token is that row, so all copies score the same maximum bit for bit."""
    g = torch.Generator(device=DEV).manual_seed(2)
    W = (0.5 * torch.randn(V, 128, device=DEV, generator=g)).bfloat16()
    ks = [k for k in (1, 2, 6, 7, 14, 15, 100, 400, 476) if 64 * k + 5 < V]
    copies = [7, 40] + [64 * k + 5 for k in ks]
    W[copies] = W[3].clone()
    x = W[3].clone().expand(N, 128).contiguous()
    idx, best = _run(x, W, None, mode)
    assert bool((idx == 3).all()), idx.unique().tolist()
    assert bool((best == best[0]).all())


def test_planted_answer_is_found_on_every_row():
    """x = W[ids] + 0.1 randn: the score margin to any other row is ~ |w_i - w_j|^2 / 2 ~ 30,
    the summation error < 0.01."""
    N, V, E = 4096, 30522, 128
    g = torch.Generator(device=DEV).manual_seed(3)
    W = (0.5 * torch.randn(V, E, device=DEV, generator=g)).bfloat16()
    ids = torch.randint(0, V, (N,), device=DEV, generator=g)
    ids[:4] = torch.tensor([0, V - 1, 63, 64], device=DEV)
    x = (W[ids].float() + 0.1 * torch.randn(N, E, device=DEV, generator=g)).bfloat16()
    idx, _ = _run(x, W, None, "nearest")
    assert torch.equal(idx, ids)


def test_non_finite_rows_stay_in_range_and_leave_the_others_alone():
    N, V, E = 300, 1000, 128
    x, W, bias, _, _ = _reference(N, V, E, "logits")
    bad = x.clone()
    bad[17] = float("nan")
    bad[130] = float("inf")
    bad[131, 5] = float("-inf")
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[[17, 130, 131]] = False
    for mode in ("logits", "nearest"):
        ref_idx, ref_best = _run(x, W, bias, mode)
        idx, best = _run(bad, W, bias, mode)
        assert int(idx.min()) >= 0 and int(idx.max()) < V
        assert torch.equal(idx[keep], ref_idx[keep]) and torch.equal(best[keep], ref_best[keep])
        assert int(idx[17]) == 0 and float(best[17]) == float("-inf")  # all-NaN scores: first row, -inf
