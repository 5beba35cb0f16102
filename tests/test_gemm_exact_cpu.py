"""The exact-integer and per-element GEMM oracles of gemm_exact_cases.py, checked on the host:
(a) the exactness preconditions hold at every shape the GPU tests use, (b) two corruptions of a
correct result pass the old max-error yardstick of test_gemm_kernels.py at its old tolerance,
(c) both fail the new checks.  No GPU and no extension."""
import pytest
import torch

import gemm_exact_cases as C


@pytest.mark.parametrize("T,K,N", C.ALL_FWD)
def test_preconditions_forward_and_dgrad(T, K, N):
    """Every builder asserts |ref| <= 256 (bf16 outputs) on its own reference; building the case
    is the check.  The operands are the integers the module docstring promises."""
    x, W, b, rs, ref = C.nt_case(1, T, K, N, bias=True, res=True)
    assert x.abs().max() <= 2 and W.abs().max() <= 1 and b.abs().max() <= 3 and rs.abs().max() <= 3
    assert ref.abs().max() <= C.BF16_EXACT_MAX
    p = (W != 0).float().mean().item()
    assert abs(p - C.weight_density(K)) < 0.02, p
    C.nn_case(2, T, K, N, acc=True)
    if T % 256 == 0 and N % 256 == 0:   # the fused act-backward kernels tile at 256 only
        for act in (2, 4):
            dy, W, aux, dz, cs = C.dact_case(3, T, K, N, act)
            assert dz.abs().max() <= C.BF16_EXACT_MAX and cs.abs().max() < C.FP32_EXACT_MAX


def test_preconditions_wgrad():
    for T, N, K in C.WGRAD_SHAPES:
        for bias in (True, False):
            C.wgrad_case(4, T, N, K, 1, bias)
    for T, N, K in C.WGRAD_MULTI:
        for nseg in (2, 3, 8):
            C.wgrad_case(5, T, N, K, nseg)
    for T, N, K, nseg in C.WGRAD_GROUP:
        C.wgrad_case(6, T, N, K, nseg)


def test_precondition_is_a_condition_not_a_mask():
    """A reference past 256 is refused, not clipped."""
    with pytest.raises(AssertionError):
        C.require_bf16_exact("x", torch.tensor([[257.0]], dtype=torch.float64))
    with pytest.raises(AssertionError):
        C.require_fp32_exact("x", torch.tensor([[2.0 ** 24]], dtype=torch.float64))
    with pytest.raises(AssertionError):
        C.require_bf16_exact("x", torch.tensor([[0.5]], dtype=torch.float64))


def test_dropped_k_term_integer_operands():
    """One k-term missing from one 16 x 16 block of an integer GEMM: at most 2 off where the old
    yardstick allows 2 % of a maximum above 100, and not equal."""
    T, K, N = 512, 768, 768
    x, W, b, _, ref = C.nt_case(7, T, K, N)
    bad = C.drop_k_term(ref, x, W).bfloat16()
    good = ref.bfloat16()
    assert C.report("good", good, ref) is None
    assert C.old_close(bad, ref), "the old yardstick was expected to miss a dropped k-term"
    msg = C.report("dropped k-term", bad, ref)
    assert msg is not None and "tile" in msg
    print(msg)


def test_dropped_k_term_real_operands():
    """The same corruption on the randn operands of test_gemm_kernels.py: outside the per-element
    bound for every k; inside the old 2 % of max|r| only when the lost products are small."""
    T, K, N = 512, 768, 768
    x, W, b = C.real_operands(C.generator(8), T, K, N)
    r, a = C.real_ref(x, W, b)
    bound = C.gemm_bound(r, a, K)
    good = r.bfloat16()     # a correctly rounded result is inside the bound everywhere
    assert C.report("good", good, r, bound) is None
    # Which k is dropped decides whether the old yardstick notices: the largest of the block's 256
    # lost products is max|x_k| max|w_k| over 16 rows / columns, about 2 * 0.1, and the old
    # tolerance is 0.02 * max|r| ~ 0.16.  So on these operands the old check catches the larger
    # terms (most k: measured, printed below) and misses the smaller ones; the new bound must
    # catch every one.  Count them, then run the full check at three k: the smallest, the median
    # and the largest lost product.
    size = C.d(x[16:32]).abs().amax(0) * C.d(W[32:48]).abs().amax(0)          # [K]
    old_tol = C.OLD_TOL * r.abs().max().item()
    # (a lost product below the tolerance by more than the bf16 rounding of r is surely missed)
    missed = int((size + C.U_BF16 * r.abs().max().item() <= old_tol).sum())
    print(f"dropped k-term, randn operands: the old yardstick surely misses {missed} of {K} k "
          f"(tolerance {old_tol:.3f}, lost product {size.min().item():.4f}..{size.max().item():.3f})")
    assert missed >= 1, missed
    order = size.argsort()
    for k in (int(order[0]), int(order[K // 2]), int(order[-1])):
        bad = C.drop_k_term(r, x, W, k=k).bfloat16()
        msg = C.report(f"dropped k-term {k}", bad, r, bound)
        assert msg is not None, k
        print(msg, "| old yardstick passes it:", C.old_close(bad, r.float()))
    assert C.old_close(C.drop_k_term(r, x, W, k=int(order[missed - 1])).bfloat16(), r.float())


def test_relu_for_gelu():
    """ReLU written for GELU differs by at most 0.17; 2 % of the largest output is more than
    that at the old test's (768, 768, 3072) shape.  The activated bound sees it."""
    T, K, N = 768, 768, 3072
    x, W, b = C.real_operands(C.generator(9), T, K, N)
    r, a = C.real_ref(x, W, b)
    want = C.act_ref(r, 1)
    bound = C.act_bound(r, a, K, 1)
    assert C.report("good", want.bfloat16(), want, bound) is None
    bad = C.relu_for_gelu(r).bfloat16()
    old_err = (bad.double() - want).abs().max().item()
    old_tol = C.OLD_TOL * want.abs().max().item()
    print(f"relu-for-gelu: max error {old_err:.4f}, old tolerance {old_tol:.4f}")
    assert C.old_close(bad, want.float()), (old_err, old_tol)
    msg = C.report("relu for gelu", bad, want, bound)
    assert msg is not None
    print(msg)


def test_report_names_tile_coordinates():
    ref = torch.zeros(512, 512, dtype=torch.float64)
    got = ref.clone()
    got[300, 260] = 1.0
    msg = C.report("t", got, ref)
    assert "(300, 260)" in msg and "(1, 1, 44, 4)" in msg, msg
    assert C.report("t", ref, ref) is None
    nan = ref.clone()
    nan[0, 0] = float("nan")
    assert C.report("t", nan, ref, torch.ones_like(ref)) is not None


def test_activation_lipschitz_constants():
    """L_ACT bounds max |act'| on a fine grid (and is not loose by more than 1 %)."""
    z = torch.linspace(-12, 12, 240001, dtype=torch.float64)
    for act in (1, 2, 3):
        m = C.dact_ref(z, act).abs().max().item()
        assert m <= C.L_ACT[act] <= 1.01 * m, (act, m)


def test_head_major_permutation():
    r = torch.arange(256 * 128, dtype=torch.float64).view(256, 128)
    h = C.head_major(r, 128).view(2, 2, 128, 64)
    assert h[1, 1, 5, 7] == r[128 + 5, 64 + 7]
