"""The flat optimizer kernels of csrc/optim.hip (sqnorm, adamw_ema, ema_update, cast_bf16) against
float64 references, past their grid caps and at their argument edges (optim_flat_cases.py has
the sizes, inputs and references).

Every case runs on `cpu` too: the PyTorch fallback of ops/optim.py is the documented oracle of
these kernels and is held to the same reference and the same tolerances.

What the sizes reach (SWEEP = 2048 blocks x 256 threads x 4 = 2,097,152 elements):
  adamw_ema / ema_update / cast_bf16
    4, 1028             one thread; one block and one thread of a second
    SWEEP               every thread runs its loop body exactly once
    SWEEP + 4           thread 0 of block 0 runs a second trip
    2 SWEEP + 3076      two full trips and a ragged third
  sqnorm (grid capped at partial.numel())
    see optim_flat_cases.SQNORM_SHAPES: a single block striding 4 and 65 times, 3 blocks, the
    1024-float default with 64 blocks, a 1500-block and a 2048-block grid whose partials take
    the one-block finalize kernel (1024 threads) a ragged and a full second trip.

Every buffer a kernel writes is a view into a larger tensor filled with a sentinel, and the
elements around the view must come back bit-equal: an in-bounds check on memory the test owns.

Each test prints its largest error against float64 before it asserts (pytest -s shows them).
Measured with these inputs (three steps, lr 0.05; kernel on the MI355X / PyTorch fallback):
p 7e-7 / 9e-7, m 1.9e-6 / 1.9e-6 (resumed moments), v 4e-7 / 4e-7 relative, EMAs 1.2e-6 / 2e-6,
norm and clip coefficient 4e-8 / 9e-8 relative.  The v tolerance resolves a 1 - beta2 formed in
fp32 (1.3e-5 off for 0.999): the launcher rounds it from double for that reason.
"""
import itertools
import math

import pytest
import torch

import optim_flat_cases as C
from distributed_pipeline_amd.ops import optim as O

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
GRADS = [pytest.param(False, id="g32"), pytest.param(True, id="g16")]


def _maxerr(actual, ref):
    a = actual.detach().cpu().double()
    return (a - ref).abs().max().item() if a.numel() else 0.0


def _close(name, actual, ref, tol):
    torch.testing.assert_close(actual.detach().cpu().double(), ref, rtol=tol[0], atol=tol[1],
                               msg=lambda m: f"{name}: {m}")


def _rel_close(name, got, want, rel=C.REL_NORM):
    assert math.isclose(got, want, rel_tol=rel, abs_tol=0.0), f"{name}: {got!r} vs float64 {want!r}"


# ---------------------------------------------------------------------------------------------
# adamw_ema
# ---------------------------------------------------------------------------------------------
def _adamw_case(device, n, bf16_grad, *, n_ema, shadow, clip, wd, step0, skip, ref=None,
                below=C.GUARD, state_below=C.GUARD):
    """Three steps on guard-banded buffers.  skip == 1: every buffer bit-identical afterwards.
    Otherwise p, m, v and the EMAs against float64, the shadow against the bf16 rounding of the
    p that came out, zero-gradient elements with m = v = 0 exactly.  `below`: elements in front
    of p and the shadow inside their tensors, `state_below`: in front of g, m, v and the EMAs.
    Returns the largest errors."""
    inp = C.adamw_inputs(n, bf16_grad)
    resumed = step0 > 0
    m0 = inp["m0"] if resumed else torch.zeros(n)
    v0 = inp["v0"] if resumed else torch.zeros(n)
    rates = C.RATES[:n_ema]
    bufs = {"p": C.Guarded(inp["p0"], device, below=below),
            "m": C.Guarded(m0, device, below=state_below),
            "v": C.Guarded(v0, device, below=state_below)}
    for k in range(n_ema):
        bufs[f"ema{k}"] = C.Guarded(inp["emas0"][k], device, below=state_below)
    if shadow:
        bufs["shadow"] = C.Guarded(torch.full((n,), 7.0, dtype=torch.bfloat16), device, below=below)
    grads = [C.Guarded(g, device, below=state_below) for g in inp["grads"]]
    clip_t = torch.tensor(C.CLIP, dtype=torch.float32, device=device) if clip else None
    skip_t = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=device)
    before = {k: b.snapshot() for k, b in bufs.items()}

    for k, g in enumerate(grads):
        O.adamw_ema_(bufs["p"].view, g.view, bufs["m"].view, bufs["v"].view, weight_decay=wd,
                     step=step0 + k + 1, grad_scale=C.GRAD_SCALE, clip=clip_t,
                     shadow_bf16=bufs["shadow"].view if shadow else None,
                     emas=[bufs[f"ema{e}"].view for e in range(n_ema)], ema_rates=rates, skip=skip_t,
                     **C.HYPER)

    tag = (f"adamw_ema[{device} n={n} {'bf16' if bf16_grad else 'fp32'}-grad emas={n_ema} shadow={shadow} "
           f"clip={clip} wd={wd} step0={step0} skip={skip}]")
    for k, b in bufs.items():
        b.assert_guards(f"{tag} {k}")
    if skip == 1:
        for k, b in bufs.items():
            b.assert_unchanged(before[k], f"{tag} {k} under a set skip flag")
        return {}

    if ref is None:
        ref = C.ref_adamw(inp["p0"], m0, v0, inp["emas0"][:n_ema], inp["grads"], wd=wd, step0=step0,
                          gs=C.grad_scale_f32(C.GRAD_SCALE, C.CLIP[1] if clip else None), rates=rates,
                          **C.HYPER)
    rp, rm, rv, re = ref
    out = {k: b.view.cpu() for k, b in bufs.items()}
    errs = {"p": _maxerr(out["p"], rp), "m": _maxerr(out["m"], rm), "v": _maxerr(out["v"], rv),
            "v/max(|v|,0.01)": ((out["v"].double() - rv).abs() / rv.abs().clamp(min=1e-2)).max().item(),
            "ema": max([_maxerr(out[f"ema{k}"], re[k]) for k in range(n_ema)], default=0.0)}
    for k, t in out.items():
        assert bool(torch.isfinite(t.float()).all()), f"{tag} {k}: non-finite values"
    z = inp["zero"]
    assert bool((out["m"][z] == 0).all()) and bool((out["v"][z] == 0).all()), \
        f"{tag}: moments of zero-gradient elements moved"
    _close(f"{tag} p", out["p"], rp, C.TOL_P)
    _close(f"{tag} m", out["m"], rm, C.TOL_M)
    _close(f"{tag} v", out["v"], rv, C.TOL_V)
    for k in range(n_ema):
        _close(f"{tag} ema{k} (rate {rates[k]})", out[f"ema{k}"], re[k], C.TOL_P)
    if shadow:
        assert C.bits_equal(out["shadow"], out["p"].bfloat16()), f"{tag}: shadow is not bf16(p)"
    return errs


def _report(name, all_errs):
    keys = sorted({k for e in all_errs for k in e})
    worst = {k: max(e.get(k, 0.0) for e in all_errs) for k in keys}
    print(f"\n[optim_flat] {name}: max error vs float64 " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bf16_grad", GRADS)
@pytest.mark.parametrize("n", C.SIZES)
def test_adamw_sizes(device, bf16_grad, n):
    """The standard configuration (shadow, 2 EMAs, device clip buffer, wd 0.1, fresh start) at
    every size: a wrong stride, a missed tail or a second update in a later sweep shows here."""
    ref = C.adamw_standard_reference(n, bf16_grad)
    errs = _adamw_case(device, n, bf16_grad, n_ema=2, shadow=True, clip=True, wd=0.1, step0=0,
                       skip=None, ref=ref)
    _report(f"adamw_ema {device} n={n} bf16_grad={bf16_grad}", [errs])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bf16_grad", GRADS)
@pytest.mark.parametrize("n_ema", [0, 1, 4, 5, 6])
@pytest.mark.parametrize("skip", [None, 0, 1])
def test_adamw_argument_matrix(device, bf16_grad, n_ema, skip):
    """n = 1028: gradient dtype x EMA count (5 and 6: the tail launches) x skip flag here, and
    shadow x clip x weight decay x fresh / resumed step inside.  skip = 1 must leave p, m, v, the
    shadow and every EMA - the fifth and sixth too - bit-identical."""
    errs = []
    for shadow, clip, wd, step0 in itertools.product((True, False), (True, False), (0.1, 0.0), (0, 50000)):
        errs.append(_adamw_case(device, 1028, bf16_grad, n_ema=n_ema, shadow=shadow, clip=clip, wd=wd,
                                step0=step0, skip=skip))
    _report(f"adamw_ema matrix {device} bf16_grad={bf16_grad} emas={n_ema} skip={skip}", errs)


@pytest.mark.parametrize("device", DEVICES)
def test_adamw_zero_shaped_slices(device):
    """The (s, c, off) pattern of parallel/zero.py: p and the shadow are a slice at offset 1024
    of their buffers, g / m / v / EMAs a slice at offset 48 of theirs; everything outside the
    slices stays as it was."""
    n = 1028
    errs = _adamw_case(device, n, False, n_ema=2, shadow=True, clip=True, wd=0.1, step0=0, skip=None,
                       ref=C.adamw_standard_reference(n, False), below=1024, state_below=48)
    _report(f"adamw_ema ZeRO slices {device}", [errs])


@pytest.mark.parametrize("device", DEVICES)
def test_grad_norm_then_adamw_on_one_stream(device):
    """grad_norm_ writes the clip buffer, adamw_ema_ reads it: same stream, no host sync between
    them (the trainer's sequence).  Reference: float64 with the float64 norm's coefficient."""
    n = 1028
    inp = C.adamw_inputs(n, False)
    bufs = {k: C.Guarded(v, device) for k, v in
            (("p", inp["p0"]), ("m", torch.zeros(n)), ("v", torch.zeros(n)), ("ema0", inp["emas0"][0]))}
    grads = [g.to(device) for g in inp["grads"]]
    partial = torch.full((2048,), math.nan, device=device)
    out = torch.full((3,), math.nan, device=device)
    gs = []
    for k, g in enumerate(grads):
        norm = C.ref_norm(inp["grads"][k], C.GRAD_SCALE, 0.0)[0]
        max_norm = 0.25 * norm  # clips: coef ~ 0.25
        gs.append(C.grad_scale_f32(C.GRAD_SCALE, C.ref_norm(inp["grads"][k], C.GRAD_SCALE, max_norm)[1]))
        O.grad_norm_(g, out, partial, C.GRAD_SCALE, max_norm)
        O.adamw_ema_(bufs["p"].view, g, bufs["m"].view, bufs["v"].view, weight_decay=0.1, step=k + 1,
                     grad_scale=C.GRAD_SCALE, clip=out, emas=[bufs["ema0"].view], ema_rates=[0.99], **C.HYPER)
    rp, rm, rv, re = C.ref_adamw(inp["p0"], torch.zeros(n), torch.zeros(n), [inp["emas0"][0]], inp["grads"],
                                 wd=0.1, step0=0, gs=gs, rates=[0.99], **C.HYPER)
    for k, b in bufs.items():
        b.assert_guards(f"composition {k}")
    _report(f"grad_norm_ + adamw_ema {device}",
            [{"p": _maxerr(bufs["p"].view, rp), "m": _maxerr(bufs["m"].view, rm), "v": _maxerr(bufs["v"].view, rv),
              "ema": _maxerr(bufs["ema0"].view, re[0])}])
    _close("composition p", bufs["p"].view, rp, C.TOL_P)
    _close("composition m", bufs["m"].view, rm, C.TOL_M)
    _close("composition v", bufs["v"].view, rv, C.TOL_V)
    _close("composition ema", bufs["ema0"].view, re[0], C.TOL_P)


# ---------------------------------------------------------------------------------------------
# sqnorm
# ---------------------------------------------------------------------------------------------
def _grad_norm(device, g, nparts, scale, max_norm):
    """-> (out [3] on the host, partial on the host).  partial and out start as NaN: an entry of
    partial inside the launched grid must be overwritten before it is summed, one beyond it
    must be neither read (out would be NaN) nor written."""
    gg = C.Guarded(g, device)
    partial = torch.full((nparts,), math.nan, device=device)
    out = torch.full((3,), math.nan, device=device)
    O.grad_norm_(gg.view, out, partial, scale, max_norm)
    return out.cpu().double().tolist(), partial.cpu()


def _check_out(tag, out, ref):
    for name, got, want in zip(("norm", "coef", "norm * coef"), out, ref):
        _rel_close(f"{tag} {name}", got, want)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bf16_grad", GRADS)
@pytest.mark.parametrize("nparts,n", C.SQNORM_SHAPES)
def test_sqnorm_shapes(device, bf16_grad, nparts, n):
    g, norm1 = C.sqnorm_inputs(n, bf16_grad)
    scale, max_norm = 0.125, 0.5 * 0.125 * norm1  # clips: coef ~ 0.5
    out, partial = _grad_norm(device, g, nparts, scale, max_norm)
    ref = C.ref_norm(g, scale, max_norm)
    print(f"\n[optim_flat] sqnorm {device} partial={nparts} n={n} bf16_grad={bf16_grad}: "
          f"rel err norm={abs(out[0] - ref[0]) / ref[0]:.3e} coef={abs(out[1] - ref[1]) / ref[1]:.3e}")
    _check_out(f"sqnorm[{device} partial={nparts} n={n}]", out, ref)
    if device != "cpu":  # the fallback has no partial sums
        grid = C.sweep_grid(n, nparts)
        assert bool(torch.isfinite(partial[:grid]).all()), "a partial inside the grid was not written"
        assert bool(torch.isnan(partial[grid:]).all()), "a partial beyond the grid was written"


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("clip", ["off", "below", "above"])
def test_sqnorm_semantics(device, scale, clip):
    """out = [norm, coef, norm * coef]: max_norm = 0 and a max_norm above the norm give a
    coefficient of exactly 1.0."""
    nparts, n = C.SQNORM_SHAPES[2]
    g, norm1 = C.sqnorm_inputs(n, False)
    max_norm = {"off": 0.0, "below": 0.3 * scale * norm1, "above": 1.5 * scale * norm1}[clip]
    out, _ = _grad_norm(device, g, nparts, scale, max_norm)
    _check_out(f"sqnorm[{device} scale={scale} max_norm {clip}]", out, C.ref_norm(g, scale, max_norm))
    if clip != "below":
        assert out[1] == 1.0 and out[2] == out[0]
    else:
        assert out[1] < 1.0


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bf16_grad", GRADS)
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_sqnorm_zero_gradient(device, bf16_grad, max_norm):
    nparts, n = C.SQNORM_SHAPES[2]
    g = torch.zeros(n, dtype=torch.bfloat16 if bf16_grad else torch.float32)
    out, _ = _grad_norm(device, g, nparts, 0.125, max_norm)
    assert out == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bf16_grad", GRADS)
@pytest.mark.parametrize("value", [math.nan, math.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["first-sweep", "later-sweep", "last"])
def test_sqnorm_nonfinite_gradient(device, bf16_grad, value, where):
    """One NaN or +Inf anywhere makes out[0] non-finite (the trainer's NaN guard reads only
    out[0]; nothing is asserted of out[1] and out[2], where fminf and clamp treat NaN
    differently), and the next call with a clean gradient and the same partial is finite again."""
    nparts, n = C.SQNORM_SHAPES[0]
    clean, _ = C.sqnorm_inputs(n, bf16_grad)
    bad = clean.clone()
    bad[{"first-sweep": 5, "later-sweep": 1024 + 517, "last": n - 1}[where]] = value
    partial = torch.full((nparts,), math.nan, device=device)
    out = torch.zeros(3, device=device)
    O.grad_norm_(bad.to(device), out, partial, 0.125, 1.0)
    assert not math.isfinite(out[0].item())
    O.grad_norm_(clean.to(device), out, partial, 0.125, 1.0)
    _check_out("sqnorm after a non-finite gradient", out.cpu().double().tolist(), C.ref_norm(clean, 0.125, 1.0))


# ---------------------------------------------------------------------------------------------
# ema_update
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("rate", [0.0, 0.5, 0.9999])
@pytest.mark.parametrize("n", C.SIZES)
def test_ema_update(device, rate, n):
    e0, p0 = C.ema_inputs(n)
    e, p = C.Guarded(e0, device), C.Guarded(p0, device)
    O.ema_(e.view, p.view, rate)
    ref = C.ref_ema(e0, p0, rate)
    print(f"\n[optim_flat] ema_update {device} n={n} rate={rate}: max|de|={_maxerr(e.view, ref):.3e}")
    e.assert_guards("ema")
    assert C.bits_equal(p.full, C.Guarded(p0, "cpu").full), "ema_update changed the parameters"
    _close(f"ema_update[{device} n={n} rate={rate}]", e.view, ref, C.TOL_P)


# ---------------------------------------------------------------------------------------------
# fp32 -> bf16: cast_bf16 and the shadow of adamw_ema
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n", C.SIZES)
def test_cast_bf16_sizes(device, n):
    x = C.ema_inputs(n)[0]
    src = C.Guarded(x, device)
    dst = C.Guarded(torch.full((n,), 7.0, dtype=torch.bfloat16), device)
    O.cast_bf16_(src.view, dst.view)
    dst.assert_guards("cast_bf16 dst")
    assert C.bits_equal(dst.view, x.bfloat16())


def _check_rounding(tag, got_bits):
    """Bit-exact round-to-nearest-even for every non-NaN input; NaN stays NaN (the payload is not
    compared: the hardware conversion may keep it).  fp32 denormals are held to the same bits:
    measured on the MI355X, the packed conversion keeps them (no flush to zero), so no weaker
    assertion is made for them."""
    _, want, nan, _ = C.bf16_patterns()
    is_nan = ((got_bits & 0x7F80) == 0x7F80) & ((got_bits & 0x007F) != 0)
    assert bool(is_nan[nan].all()), f"{tag}: {int((~is_nan[nan]).sum())} NaN inputs came out as numbers"
    wrong = (got_bits != want) & ~nan
    first = wrong.nonzero().flatten()[:4].tolist()
    assert not first, (f"{tag}: {int(wrong.sum())} values are not round-to-nearest-even, first at "
                       + ", ".join(f"x bits {C.bf16_patterns()[0].view(torch.int32)[i].item() & 0xFFFFFFFF:#010x} -> "
                                   f"{got_bits[i].item():#06x} (want {want[i].item():#06x})" for i in first))


@pytest.mark.parametrize("device", DEVICES)
def test_cast_bf16_every_rounding_case(device):
    x = C.bf16_patterns()[0]
    dst = C.Guarded(torch.full((x.numel(),), 7.0, dtype=torch.bfloat16), device)
    O.cast_bf16_(C.Guarded(x, device).view, dst.view)
    dst.assert_guards("cast_bf16 dst")
    _check_rounding(f"cast_bf16[{device}]", C.bf16_bits(dst.view))


@pytest.mark.parametrize("device", DEVICES)
def test_adamw_shadow_every_rounding_case(device):
    """The shadow written by adamw_ema, through a step that leaves p as it is: zero gradient,
    lr = 0, weight decay 0."""
    x, _, nan, _ = C.bf16_patterns()
    n = x.numel()
    p = C.Guarded(x, device)
    shadow = C.Guarded(torch.full((n,), 7.0, dtype=torch.bfloat16), device)
    m, v = torch.zeros(n, device=device), torch.zeros(n, device=device)
    O.adamw_ema_(p.view, torch.zeros(n, device=device), m, v, lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8,
                 weight_decay=0.0, step=1, shadow_bf16=shadow.view)
    shadow.assert_guards("shadow")
    got = p.view.cpu()
    assert bool((got.view(torch.int32) == x.view(torch.int32))[~nan].all()), "a no-op step changed p"
    assert bool(torch.isnan(got[nan]).all())
    _check_rounding(f"adamw_ema shadow[{device}]", C.bf16_bits(shadow.view))
