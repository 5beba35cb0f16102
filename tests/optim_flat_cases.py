"""Inputs, guard-banded buffers and float64 references for the flat optimizer kernels of
csrc/optim.hip (sqnorm, adamw_ema, ema_update, cast_bf16).

Used by test_optim_flat.py; everything here is plain PyTorch on the host.  Inputs are drawn from
a host generator, so every device sees the same values.

Sizes: the element-wise kernels launch at most 2048 blocks x 256 threads x 4 elements, i.e.
SWEEP elements per pass of their grid-stride loop.  SIZES are the smallest n that reach
    4                   one thread
    1028                one block plus one thread of a second block
    SWEEP               exactly one full sweep (every thread once, nobody twice)
    SWEEP + 4           one thread enters a second sweep
    2 SWEEP + 3076      a ragged third sweep (three blocks and one thread)
sqnorm's grid is capped by partial.numel() instead, SQNORM_SHAPES below.
"""
import functools
import math

import torch

SWEEP = 2048 * 1024
SIZES = (4, 1028, SWEEP, SWEEP + 4, 2 * SWEEP + 3 * 1024 + 4)
LARGE = SIZES[2:]

# (partial.numel(), n): what the stage-1 grid and the finalize loop (1024 threads) do
SQNORM_SHAPES = (
    (1, 3076),                     # one block, 4 trips of the stride loop (the 4th ragged)
    (1, 65540),                    # one block, 65 trips
    (3, 5 * 1024 + 4),             # 3 blocks, a full second trip and one thread in a third
    (1024, 65536),                 # 64 blocks of a 1024-float partial: entries 64.. stay unread
    (1500, 1500 * 1024 + 2052),    # capped grid, partly second sweep; finalize: ragged 2nd trip
    (2048, SWEEP + 4),             # the trainer's partial size; finalize loop runs twice
)

# tolerances of test_optim_ops.py: (rtol, atol)
TOL_P = (1e-5, 5e-5)   # parameters and EMAs
TOL_M = (1e-5, 1e-6)
TOL_V = (1e-5, 1e-7)
REL_NORM = 1e-5

GUARD = 64
SENTINEL = -6.0221e23  # finite, exact in neither format's small integers; compared by bits

HYPER = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8)
GRAD_SCALE = 0.125
CLIP = (3.0, 0.37, 1.1)
# the first k are used for k EMAs: 0.9999 and 0.0 are in every count >= 2
RATES = (0.9999, 0.0, 0.5, 0.99, 0.9, 0.999)
STEPS = 3


def sweep_grid(n, cap=2048):
    """Blocks launched for n elements (csrc/optim.hip grid_for, 4 per thread, 256 threads)."""
    return max(1, min(cap, (n // 4 + 255) // 256))


# ---------------------------------------------------------------------------------------------
# guard-banded buffers
# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


class Guarded:
    """`view` = [below : below + n] of a tensor of below + n + above elements filled with
    SENTINEL.  Both bands belong to the test; a kernel that honours n never touches them."""

    def __init__(self, values, device, below=GUARD, above=GUARD):
        n = values.numel()
        full = torch.full((below + n + above,), SENTINEL, dtype=values.dtype)
        full[below:below + n] = values
        self.full = full.to(device)
        self.view = self.full[below:below + n]
        self.below = below
        self.band = torch.full((below + above,), SENTINEL, dtype=values.dtype)

    def assert_guards(self, name):
        n = self.view.numel()
        got = torch.cat([self.full[:self.below], self.full[self.below + n:]]).cpu()
        bad = (_bits(got) != _bits(self.band)).nonzero().flatten().tolist()
        assert not bad, (f"{name}: written outside its {n} elements, at band positions {bad[:8]} "
                         f"(below: 0..{self.below - 1}, above: from {self.below})")

    def snapshot(self):
        return self.full.clone()

    def assert_unchanged(self, snap, name):
        diff = (_bits(self.full) != _bits(snap)).sum().item()
        assert diff == 0, f"{name}: {diff} elements changed"


def bits_equal(a, b):
    return bool((_bits(a.cpu().contiguous()) == _bits(b.cpu().contiguous())).all())


# ---------------------------------------------------------------------------------------------
# AdamW inputs
# ---------------------------------------------------------------------------------------------
def _loguniform(n, gen):
    """Magnitudes log-uniform in [1e-12, 1e3], random sign, times rand: after the 0.125 * 0.37
    scale many elements have sqrt(v) near eps = 1e-8."""
    mag = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 15.0 - 12.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sign * torch.rand(n, generator=gen, dtype=torch.float64)).float()


@functools.lru_cache(maxsize=4)
def adamw_inputs(n, bf16_grad):
    """dict(p0, grads[STEPS], zero, emas0[6], m0, v0) of host tensors; callers must not modify
    them.  `zero`: the elements whose gradient is exactly 0 in every step (about 5 %, at least
    one).  m0 / v0: the moments a resumed run starts from, |m0| <= sqrt(v0) elementwise and both
    0 where the gradient is."""
    gen = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=gen)
    zero = torch.rand(n, generator=gen) < 0.05
    zero[n // 2] = True
    grads = []
    for _ in range(STEPS):
        g = _loguniform(n, gen)
        g[zero] = 0.0
        grads.append(g.bfloat16() if bf16_grad else g)
    emas0 = [torch.randn(n, generator=gen) * (0.5 + 0.25 * k) + (k - 2.0) for k in range(len(RATES))]
    gs = GRAD_SCALE * CLIP[1]
    v0 = (_loguniform(n, gen) * gs).square()
    m0 = (2.0 * torch.rand(n, generator=gen) - 1.0) * v0.sqrt() * 0.999
    v0[zero] = 0.0
    m0[zero] = 0.0
    assert bool((m0.abs() <= v0.sqrt()).all())
    return dict(p0=p0, grads=grads, zero=zero, emas0=emas0, m0=m0, v0=v0)


def grad_scale_f32(grad_scale, clip1):
    """The scale the kernel applies: the fp32 product grad_scale * clip[1]."""
    s = torch.tensor(grad_scale, dtype=torch.float32)
    if clip1 is not None:
        s = s * torch.as_tensor(clip1, dtype=torch.float32)
    return float(s)


# ---------------------------------------------------------------------------------------------
# float64 references (written out; not torch.optim)
# ---------------------------------------------------------------------------------------------
def ref_adamw(p, m, v, emas, grads, *, lr, beta1, beta2, eps, wd, step0, gs, rates):
    """STEPS of AdamW with decoupled weight decay and the EMAs of the updated parameters, all in
    float64, on the given fp32 / bf16 values.  gs: the gradient scale, one number or one per
    step.  Returns (p, m, v, emas) float64."""
    p, m, v = p.double(), m.double(), v.double()
    emas = [e.double() for e in emas]
    for k, g in enumerate(grads):
        step = step0 + k + 1
        g = g.double() * (gs[k] if isinstance(gs, (list, tuple)) else gs)
        p = p * (1.0 - lr * wd)
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        mhat = m / (1.0 - beta1 ** step)
        vhat = v / (1.0 - beta2 ** step)
        p = p - lr * mhat / (vhat.sqrt() + eps)
        emas = [e * r + p * (1.0 - r) for e, r in zip(emas, rates)]
    return p, m, v, emas


@functools.lru_cache(maxsize=2)
def adamw_standard_reference(n, bf16_grad):
    """Reference of the standard configuration (test_adamw_sizes), shared by both devices."""
    inp = adamw_inputs(n, bf16_grad)
    return ref_adamw(inp["p0"], torch.zeros(n), torch.zeros(n), inp["emas0"][:2], inp["grads"],
                     wd=0.1, step0=0, gs=grad_scale_f32(GRAD_SCALE, CLIP[1]), rates=RATES[:2], **HYPER)


def ref_ema(e, p, rate):
    return e.double() * rate + p.double() * (1.0 - rate)


def ref_norm(g, scale, max_norm):
    """[norm, coef, norm * coef] in float64 (clip_grad_norm_ semantics, 1e-6 in the divisor)."""
    norm = math.sqrt(g.double().square().sum().item()) * scale
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    return norm, coef, norm * coef


@functools.lru_cache(maxsize=2)
def ema_inputs(n):
    gen = torch.Generator().manual_seed(2000 + n)
    return torch.randn(n, generator=gen) * 3.0 + 1.0, torch.randn(n, generator=gen)


@functools.lru_cache(maxsize=4)
def sqnorm_inputs(n, bf16_grad):
    """(gradient, float64 sum-of-squares norm at scale 1)."""
    gen = torch.Generator().manual_seed(3000 + n)
    g = torch.randn(n, generator=gen)
    g = g.bfloat16() if bf16_grad else g
    return g, math.sqrt(g.double().square().sum().item())


# ---------------------------------------------------------------------------------------------
# fp32 -> bf16: every upper half with the lower halves that decide the rounding
# ---------------------------------------------------------------------------------------------
LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


@functools.lru_cache(maxsize=1)
def bf16_patterns():
    """(x fp32 [393216], expected bf16 bits as int32, nan mask, denormal mask).  Contains every
    tie (low 0x8000 on an even and on an odd upper half), every carry into the exponent, the 6
    finite values that round to +-Inf, +-Inf, 1534 NaNs and all denormal upper halves."""
    hi = torch.arange(65536, dtype=torch.int64).repeat_interleave(len(LOW_HALVES))
    lo = torch.tensor(LOW_HALVES, dtype=torch.int64).repeat(65536)
    u = (hi << 16) | lo
    x = (u - ((u >> 31) << 32)).to(torch.int32).view(torch.float32)  # two's complement of the sign bit
    want = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = torch.isnan(x)
    denormal = ((u >> 23) & 0xFF) == 0
    denormal &= (u & 0x7FFFFF) != 0
    assert x.numel() == 393216 and int(nan.sum()) == 1534
    # the integer formula is what torch's conversion computes for every non-NaN value
    got = _bits(x.bfloat16()).to(torch.int64) & 0xFFFF
    assert bool((got[~nan] == want[~nan]).all())
    assert int(((want & 0x7FFF) == 0x7F80)[~nan].sum()) == 2 + 6  # +-Inf, and 6 finite values -> +-Inf
    return x, want, nan, denormal


def bf16_bits(t):
    return _bits(t.cpu().contiguous()).to(torch.int64) & 0xFFFF
