"""Exact-integer operands and per-element error bounds for the bf16 GEMM family.

Plain PyTorch on the host (no GPU, no extension): test_gemm_exact_cpu.py checks the helpers
themselves, test_gemm_exact_gpu.py runs the kernels against them.

Two oracles, both of which fail on ONE wrong element (the old yardstick of test_gemm_kernels.py,
max|a - r| <= tol * max|r|, is kept here as `old_close` only to show what it cannot see):

* Integer operands.  Activations / gradients uniform on {-2..2}, weights in {-1, 0, 1} with
  P(w != 0) = min(1/2, 384 / K), biases / residuals / accumulate-into tensors in {-3..3}.  Every
  product and every partial sum is a small integer, so an fp32 accumulation is exact in ANY order
  (|partial| <= 2 K < 2^24), every bf16 output is exact while |ref| <= 256 (all integers up to
  2^8 are bf16 numbers) and every fp32 output while |ref| < 2^24.  The builders assert exactly
  those two conditions on the reference and the kernels must then match it bit for bit.
  Dot-product spread: var(act) = 2, var(w) = p, so std = sqrt(2 p K) <= sqrt(768) ~ 27.7 for
  every K; 256 is more than 9 sigma away.

* Real-valued operands.  For the float64 reference r = x64 @ W64.T + b the bf16 output y obeys

      |y - r| <= 2^-8 |r| + K 2^-23 (|x| @ |W|.T + |b|)        (gemm_bound)

  element by element: the first term is the unit roundoff of the final round-to-nearest bf16
  conversion (spacing 2^(e-7) in [2^e, 2^(e+1)), so half a spacing is at most 2^-8 |v|); the
  second is the gamma_K forward-error bound of a K-term fp32 dot product plus the bias add
  (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5: gamma_n = n u / (1 - n u)
  with u = 2^-24), doubled to K 2^-23 so that it also covers the (1 + 2^-8) factor of rounding
  the perturbed value instead of r, any summation order and the MFMA's block-wise accumulation.
  Nothing here is fitted to kernel output.
"""
import math

import torch

TILE = 256                      # tile side used for the failure report
OLD_TOL = 2e-2                  # test_gemm_kernels._close: forward / dgrad tolerance
BF16_EXACT_MAX = 256            # every integer of magnitude <= 2^8 is a bf16 number
FP32_EXACT_MAX = 2 ** 24        # every integer of magnitude < 2^24 is an fp32 number
U_BF16 = 2.0 ** -8              # unit roundoff of round-to-nearest bf16 (8 significant bits)
U_DOT = 2.0 ** -23              # per-term weight of the fp32 dot-product bound (2 u, see above)

# Lipschitz constants of the activations (max |act'|), used to push a pre-activation bound
# through the activation:
#   GELU  z Phi(z):  act' = Phi(z) + z phi(z); act'' = phi(z) (2 - z^2) = 0 at z = sqrt 2, where
#                    act' = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 0.92135 + 0.20755 = 1.1289 -> 1.13
#   tanh:            act' = 1 - tanh^2 <= 1
#   SiLU  z s(z):    act' = s (1 + z (1 - s)), maximal at z ~ 2.3994 where it is 1.09984 -> 1.1
L_ACT = {0: 1.0, 1: 1.13, 2: 1.0, 3: 1.1}

# Accuracy of act'(aux) as the kernels evaluate it in fp32 (csrc/act.h): the erf approximation is
# stated there as |error| < 1.5e-7; the exp / rcp hardware ops and the ~8 fp32 operations around
# them each add at most 2^-24 relative on quantities <= 1.2, i.e. < 8 * 1.2 * 6e-8 = 5.8e-7.
# Together < 2^-20 = 9.5e-7 absolute on a derivative of magnitude <= 1.13.
EPS_DACT = 2.0 ** -20


def generator(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


# ---- operands ---------------------------------------------------------------------------

def int_acts(gen, *shape):
    """Activations / gradients: integers uniform on {-2..2}, bf16."""
    return torch.randint(-2, 3, shape, generator=gen).to(torch.bfloat16)


def weight_density(kred, cap=384):
    return min(0.5, cap / kred)


def int_weights(gen, rows, cols, kred, cap=384):
    """Weights in {-1, 0, 1} with P(w != 0) = min(1/2, cap / kred); kred is the length of the
    reduction this weight takes part in (cap = 384 unless a case needs a lower density)."""
    p = weight_density(kred, cap)
    nz = torch.rand(rows, cols, generator=gen) < p
    sign = torch.randint(0, 2, (rows, cols), generator=gen) * 2 - 1
    return (sign * nz).to(torch.bfloat16)


def int_small(gen, *shape):
    """Biases, residuals and accumulate-into tensors: integers uniform on {-3..3} (float32;
    the caller casts to bf16 where the kernel takes bf16)."""
    return torch.randint(-3, 4, shape, generator=gen).float()


def real_operands(gen, T, K, N):
    """The operands of test_gemm_kernels.py: x ~ randn, W ~ 0.05 randn, b ~ randn (bf16)."""
    x = torch.randn(T, K, generator=gen).bfloat16()
    W = (torch.randn(N, K, generator=gen) * 0.05).bfloat16()
    b = torch.randn(N, generator=gen).bfloat16()
    return x, W, b


# ---- preconditions ----------------------------------------------------------------------

def require_bf16_exact(name, ref):
    m = ref.abs().max().item()
    assert m <= BF16_EXACT_MAX, f"{name}: |ref| reaches {m} > {BF16_EXACT_MAX}; lower the density for this shape"
    assert torch.equal(ref, ref.round()), f"{name}: reference is not integer-valued"
    return ref


def require_fp32_exact(name, ref):
    m = ref.abs().max().item()
    assert m < FP32_EXACT_MAX, f"{name}: |ref| reaches {m} >= 2^24"
    assert torch.equal(ref, ref.round()), f"{name}: reference is not integer-valued"
    return ref


# ---- exact references (float64: exact on these integers) --------------------------------

def d(t):
    return t.double()


def ref_nt(x, W, b=None, res=None):
    """x W^T (+ b) (+ res), bf16 output."""
    r = d(x) @ d(W).t()
    if b is not None:
        r = r + d(b)
    if res is not None:
        r = r + d(res)
    return require_bf16_exact("nt", r)


def head_major(r, L):
    """[T, N] -> the [T / L, N / 64, L, 64] store order of gemm_nt(head_major_L=L), flat [T, N]."""
    T, N = r.shape
    return r.view(T // L, L, N // 64, 64).permute(0, 2, 1, 3).reshape(T, N).contiguous()


def ref_nn(dy, W, acc=None):
    """dy W (+ acc), bf16 output."""
    r = d(dy) @ d(W)
    if acc is not None:
        r = r + d(acc)
    return require_bf16_exact("nn", r)


def ref_nn_dact(dy, W, dact):
    """(dy W) * act'(aux) with an integer-valued act' -> (dz, column sums of dz).  The column
    sums are those of the EXACT dz, never of a kernel's output."""
    r = require_bf16_exact("nn_dact pre", d(dy) @ d(W))
    dz = require_bf16_exact("nn_dact", r * d(dact))
    return dz, require_fp32_exact("nn_dact colsum", dz.sum(0))


def ref_wgrad(dys, xs, dW0, db0=None):
    """dW0 + sum_s dy_s^T x_s (and db0 + sum_s colsum(dy_s)), fp32 outputs."""
    dW = d(dW0).clone()
    db = d(db0).clone() if db0 is not None else None
    for dy, x in zip(dys, xs):
        dW += d(dy).t() @ d(x)
        if db is not None:
            db += d(dy).sum(0)
    require_fp32_exact("wgrad dW", dW)
    if db is not None:
        require_fp32_exact("wgrad db", db)
    return dW, db


# ---- bounds for real-valued operands ----------------------------------------------------

def real_ref(x, W, b=None):
    """float64 r = x W^T (+ b) and |x| |W|^T (+ |b|) for the same operands."""
    r = d(x) @ d(W).t()
    a = d(x).abs() @ d(W).abs().t()
    if b is not None:
        r = r + d(b)
        a = a + d(b).abs()
    return r, a


def gemm_bound(r, absdot, K):
    """|y - r| <= 2^-8 |r| + K 2^-23 absdot (module docstring)."""
    return U_BF16 * r.abs() + K * U_DOT * absdot


def act_ref(z, act):
    """float64 activation: exact-erf GELU, tanh, SiLU."""
    if act == 1:
        return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))
    if act == 2:
        return torch.tanh(z)
    if act == 3:
        return z * torch.sigmoid(z)
    return z


def dact_ref(z, act):
    """float64 act'(z)."""
    if act == 1:
        return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    if act == 2:
        return 1 - torch.tanh(z) ** 2
    if act == 3:
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    return torch.ones_like(z)


def act_bound(r, absdot, K, act):
    """|y - act(r)| <= 2^-8 |act(r)| + L_act * gemm_bound: the pre-activation error pushed through
    the activation (mean-value theorem) plus the final bf16 rounding.  The kernels activate the
    fp32 accumulator, so the 2^-8 |r| part of gemm_bound is slack here; it is > 1e3 x the
    1.5e-7 |z| approximation error csrc/act.h states, which therefore needs no term of its own."""
    return U_BF16 * act_ref(r, act).abs() + L_ACT[act] * gemm_bound(r, absdot, K)


def dact_bound(r, absdot, K, dv):
    """dz = (dy W) * act'(aux) for an exact product r and float64 dv = act'(aux):

        |dz - r dv| <= 2^-8 |r dv| + |dv| gemm_bound(r) + |r| (1 + 2^-8) EPS_DACT

    The middle term holds the one rounding point this adds to gemm_bound: a kernel may round
    dy W to bf16 BEFORE the multiply (the 256-tile dact epilogue does; the existing reference
    `(dy W).bfloat16().float() * d` says the same), which is the 2^-8 |r| inside gemm_bound
    scaled by |dv|.  The last term is the fp32 evaluation error of act' (EPS_DACT) on a
    product already perturbed by at most 2^-8."""
    return U_BF16 * (r * dv).abs() + dv.abs() * gemm_bound(r, absdot, K) + r.abs() * (1 + U_BF16) * EPS_DACT


# ---- checks and the failure report ------------------------------------------------------

def _where(i, ncols):
    r, c = divmod(int(i), ncols)
    return (r, c), (r // TILE, c // TILE, r % TILE, c % TILE)


def report(name, got, ref, bound=None):
    """None when got matches ref (exactly, or within bound element by element); else a message
    naming the worst element: index, tile coordinates (row // 256, col // 256, row % 256,
    col % 256) and both values."""
    g = d(got.detach().cpu()).reshape(ref.shape if ref.dim() == 2 else (1, -1))
    r = d(ref).reshape(g.shape)
    err = (g - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if bound is None:
        bad = err > 0
        score = err
    else:
        b = d(bound).reshape(g.shape)
        bad = ~(err <= b)
        score = err - b
    nbad = int(bad.sum())
    if nbad == 0:
        return None
    i = torch.where(bad, score, torch.full_like(score, -float("inf"))).argmax()
    idx, tile = _where(i, g.shape[1])
    msg = (f"{name}: {nbad} of {g.numel()} elements wrong; worst at {idx} = tile (row//256, col//256, "
           f"row%256, col%256) {tile}: got {g.flatten()[i].item()!r} want {r.flatten()[i].item()!r}")
    if bound is not None:
        msg += f" |err| {err.flatten()[i].item():.3e} > bound {b.flatten()[i].item():.3e}"
    return msg


def assert_exact(name, got, ref):
    msg = report(name, got, ref)
    assert msg is None, msg


def assert_within(name, got, ref, bound):
    msg = report(name, got, ref, bound)
    assert msg is None, msg


def old_close(a, r, tol=OLD_TOL):
    """The yardstick of test_gemm_kernels._close, as a predicate."""
    err = (a.float() - r.float()).abs().max().item()
    return err <= tol * max(r.float().abs().max().item(), 1e-3)


# ---- corruption models (CPU test only) --------------------------------------------------

def drop_k_term(r, x, W, r0=16, c0=32, k=None):
    """r = x W^T with ONE k-term left out of the 16 x 16 block at (r0, c0): term k, or the first
    k whose outer product is non-zero somewhere in the block."""
    xb, wb = d(x[r0:r0 + 16]), d(W[c0:c0 + 16])
    for k in (range(x.shape[1]) if k is None else [k]):
        outer = xb[:, k:k + 1] * wb[:, k][None, :]
        if outer.abs().max() > 0:
            out = r.clone()
            out[r0:r0 + 16, c0:c0 + 16] -= outer
            return out
    raise AssertionError("no non-zero k-term in the block")


def relu_for_gelu(z):
    """What a forward epilogue would give with ReLU in GELU's place."""
    return torch.relu(z)


# ---- the shape table (tokens T, reduction K, output width N) ----------------------------

SHAPES_128 = [(128, 128, 128), (256, 384, 128)]            # set_gemm256(False)
SHAPES_256 = [(256, 128, 256), (512, 768, 768), (768, 3072, 256)]
SHAPE_STATIC = (1024, 256, 768)   # grid cap 3: 12 tiles on 3 workgroups, 4 each, K / 64 = 4
SHAPE_QUEUE = (2048, 128, 768)    # grid cap 8: 24 tiles > 8 workgroups -> the queue path
SHAPE_HALF = (512, 256, 512)      # set_gemmp_half(2) / (0)
SHAPE_GM8 = (2048, 128, 2048)     # (M / 256) % 8 == 0 and N / 256 >= 8: the GM = 8 tile order
ALL_FWD = SHAPES_128 + SHAPES_256 + [SHAPE_STATIC, SHAPE_QUEUE, SHAPE_HALF, SHAPE_GM8]
REAL_SHAPES = [(512, 768, 768), (256, 3072, 256)]

# weight-gradient cases (tokens T, dy width N, x width K); see test_gemm_exact_gpu.py for the
# split-K notes
WGRAD_SHAPES = [(128, 256, 256), (256, 256, 256), (512, 384, 128), (256, 128, 768), (1024, 768, 256)]
WGRAD_MULTI = [(256, 256, 512), (1024, 768, 256)]
# grouped launch: three sites of different shapes and segment counts (T, N, K, nseg)
WGRAD_GROUP = [(256, 768, 256, 3), (128, 256, 512, 1), (512, 512, 768, 8)]


def nt_case(seed, T, K, N, bias=True, res=False):
    g = generator(seed)
    x, W = int_acts(g, T, K), int_weights(g, N, K, K)
    b = int_small(g, N).bfloat16() if bias else None
    rs = int_small(g, T, N).bfloat16() if res else None
    return x, W, b, rs, ref_nt(x, W, b, rs)


def nn_case(seed, T, K, N, acc=False, cap=384):
    """dy [T, K] (K is the reduction), W [K, N] -> dx [T, N]."""
    g = generator(seed)
    dy, W = int_acts(g, T, K), int_weights(g, K, N, K, cap)
    dx0 = int_small(g, T, N).bfloat16() if acc else None
    return dy, W, dx0, ref_nn(dy, W, dx0)


def dact_case(seed, T, K, N, act):
    """act 2: aux = y in {-1, 0, 1}, act' = 1 - y^2 in {0, 1}.  act 4: aux = act' in {0, 1, 2};
    the product doubles, so the weight density is quartered (cap 96: std(dy W) <= 13.9, times
    2 is the 27.7 of every other case)."""
    g = generator(seed)
    cap = 96 if act == 4 else 384
    dy, W = int_acts(g, T, K), int_weights(g, K, N, K, cap)
    if act == 2:
        aux = torch.randint(-1, 2, (T, N), generator=g).to(torch.bfloat16)
        dv = 1 - aux.double() ** 2
    else:
        aux = torch.randint(0, 3, (T, N), generator=g).to(torch.bfloat16)
        dv = aux.double()
    dz, cs = ref_nn_dact(dy, W, dv)
    return dy, W, aux, dz, cs


def wgrad_case(seed, T, N, K, nseg=1, bias=True):
    g = generator(seed)
    dys = [int_acts(g, T, N) for _ in range(nseg)]
    xs = [int_acts(g, T, K) for _ in range(nseg)]
    dW0 = int_small(g, N, K)
    db0 = int_small(g, N) if bias else None
    dW, db = ref_wgrad(dys, xs, dW0, db0)
    return dys, xs, dW0, db0, dW, db
