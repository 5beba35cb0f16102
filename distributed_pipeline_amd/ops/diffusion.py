"""
Fused DiffuSeq diffusion-side ops on the gfx950 kernels of ``csrc/diffusion.hip``
(SURVEY K-M1..K-M4, K-M13; the workload of reference utils/trainer.py:1-4):

* :func:`emb_qsample` - word-embedding gather, x_start noise and masked
  ``q_sample`` in one kernel with the noise drawn in-kernel (counter-based
  Philox), returning ``(x_start fp32, x_start bf16, x_t bf16)``.  Its backward
  scatter-adds every gradient reaching the three outputs into the tied
  embedding's fp32 gradient (one atomic pass).
* :func:`diffusion_mse` - the per-sample ``mse`` (with DiffuSeq's t == 0 branch
  against the un-noised embedding) and ``tT`` terms, one workgroup per sample;
  the backward writes d(model output) in its dtype and d(x_start) in fp32.
* :func:`timestep_embedding` - sinusoidal [cos | sin] embedding straight to bf16.
* :func:`reverse_step` - one reverse-process update of decoding,
  ``a x0_hat + b x_t + s z`` (+ ``a_prev x0_hat_prev`` for the multistep
  samplers) with the source rows kept, as one kernel
  (``csrc/reverse_step.hip``) with batch-independent in-kernel noise; it carries
  its own PyTorch path for the CPU / fp32.

The training ops are only used for HIP tensors of a bf16 model; the PyTorch formulas
in ``models/gaussian_diffusion.py`` are the CPU / fp32 path and the numerics oracle
of ``tests/test_diffusion_kernels.py``.
"""
import math

import torch

from ._ext import get_ext
from .nn import RNG


def available(W):
    """True when the fused kernels can serve the embedding table ``W``."""
    if not (W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.shape[1] % 4 == 0):
        return False
    ext = get_ext()
    return ext is not None and hasattr(ext, "emb_qsample_fwd")


def _grad_buffer(p):
    """(fp32 buffer to accumulate p's gradient into, tensor to hand to autograd or None).

    The flat engine preallocates ``p.grad`` (a view of the flat gradient buffer): the
    kernels accumulate into it in place and autograd receives None (its
    AccumulateGrad node - and the engine's readiness hook - still runs)."""
    g = p.grad
    if g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape:
        return g, None
    g = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
    return g, g


def _c(t):
    return None if t is None else t.contiguous()


def _f(t):
    return None if t is None else t.contiguous().float()


class _EmbQSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, ids, mask, t, sa, s1a, std0, seed, off):
        ctx.set_materialize_grads(False)
        xs, xs16, xt = get_ext().emb_qsample_fwd(ids, mask, t, W.detach(), sa, s1a, float(std0),
                                                 int(seed), int(off), True)
        ctx.save_for_backward(ids, mask, t, sa)
        ctx.W = W
        return xs, xs16, xt

    @staticmethod
    def backward(ctx, d_xs, d_xs16, d_xt):
        ids, mask, t, sa = ctx.saved_tensors
        ret = None
        if ctx.needs_input_grad[0] and any(g is not None for g in (d_xs, d_xs16, d_xt)):
            buf, ret = _grad_buffer(ctx.W)
            get_ext().emb_qsample_bwd(ids, mask, t, sa, _c(d_xs), _c(d_xs16), _c(d_xt), buf)
        return (ret,) + (None,) * 8


class _DiffLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_start, out, ids, t, W, sa_last, t0_via_x_start):
        ctx.set_materialize_grads(False)
        mse, tT = get_ext().diff_loss_fwd(x_start, out, ids, t, W.detach(), float(sa_last))
        ctx.save_for_backward(x_start, out, ids, t)
        ctx.W, ctx.sa_last, ctx.fold = W, float(sa_last), bool(t0_via_x_start)
        return mse, tT

    @staticmethod
    def backward(ctx, dmse, dtT):
        x_start, out, ids, t = ctx.saved_tensors
        if dmse is None and dtT is None:
            return (None,) * 7
        buf = ret = None
        # t == 0 samples: d x0_mean into the embedding rows.  When x_start = W[ids] + noise
        # (emb_qsample) and both get gradients, that term rides on d_xs into the sorted,
        # deterministic embedding backward; otherwise fp32 atomics into W's gradient here.
        fold = ctx.fold and ctx.needs_input_grad[0] and ctx.needs_input_grad[4]
        if ctx.needs_input_grad[4] and dmse is not None and not fold:
            buf, ret = _grad_buffer(ctx.W)
        d_out, d_xs = get_ext().diff_loss_bwd(x_start, out, ids, t, ctx.W.detach(), _f(dmse), _f(dtT),
                                              ctx.sa_last, ctx.needs_input_grad[1],
                                              ctx.needs_input_grad[0], buf, fold_t0=fold)
        return (d_xs if ctx.needs_input_grad[0] else None,
                d_out if ctx.needs_input_grad[1] else None, None, None, ret, None, None)


def emb_qsample(W, ids, mask, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, std0):
    """-> (x_start fp32, x_start bf16, x_t bf16), each [B, L, E]; fresh noise per call."""
    seed, off = RNG.next()
    return _EmbQSampleFn.apply(W, ids.contiguous(), mask.to(torch.long).contiguous(),
                               t.to(torch.long).contiguous(), sqrt_alphas_cumprod,
                               sqrt_one_minus_alphas_cumprod, float(std0), seed, off)


def diffusion_mse(x_start, out, ids, t, W, sqrt_alpha_bar_last, t0_via_x_start=False):
    """-> (mse [B], tT [B]) fp32 (DiffuSeq ``training_losses_seq2seq`` terms).
    ``t0_via_x_start``: x_start is :func:`emb_qsample`'s (W[ids] + noise), so the t == 0 samples'
    embedding gradient may be routed through d x_start (deterministic)."""
    return _DiffLossFn.apply(x_start, out.contiguous(), ids.contiguous(), t.to(torch.long).contiguous(),
                             W, float(sqrt_alpha_bar_last), bool(t0_via_x_start))


def _erf_tau(top_p):
    """erf(tau / sqrt 2) in double: the mass of the standard normal inside [-tau, tau]."""
    return math.erf(float(top_p) / math.sqrt(2.0))


def step_generator(seed, step, device):
    """The ``torch.Generator`` of the PyTorch path's noise at (seed, step)."""
    g = torch.Generator(device=device)
    g.manual_seed((int(seed) * 1000003 + int(step)) % (2 ** 63))
    return g


def draw_noise(shape, device, generator, top_p=0.0):
    """Standard normal noise from ``generator``; with ``top_p`` = tau > 0 truncated to [-tau, tau]
    by inverse CDF (the distribution DiffuSeq's re-draw loop produces, without the loop)."""
    if top_p <= 0:
        return torch.randn(shape, dtype=torch.float32, device=device, generator=generator)
    u = torch.rand(shape, dtype=torch.float64, device=device, generator=generator)
    u = u.clamp_(2.0 ** -53, 1.0 - 2.0 ** -53)
    z = math.sqrt(2.0) * torch.erfinv((2.0 * u - 1.0) * _erf_tau(top_p))
    return z.clamp_(-float(top_p), float(top_p)).float()


def reverse_step(x, *, pred=None, idx=None, weight=None, scale=1.0, x_start=None, mask=None, a, b, s,
                 seed, step, row_base=0, top_p=0.0, noise=None, want_bf16=False,
                 pred_prev=None, idx_prev=None, a_prev=0.0):
    """One DiffuSeq reverse-process update ``[..., E]`` -> ``(out fp32, out bf16 | None)``:

        x0  = pred                          (the model's prediction)
              or scale * weight[idx]        (its rounding; ids outside [0, V): a zero row)
        y   = a * x0 + b * x + s * z
        out = where(mask == 0, x_start, y)  (mask [...] marks the target positions)

    ``x`` may be None when b == 0 and ``pred`` / ``idx`` when a == 0; a = b = 0, s = 1 draws the
    start noise.  On a HIP device with fp32 ``x`` / ``x_start``, a bf16 ``pred`` or an fp32
    ``weight``, E % 4 == 0 and no explicit ``noise`` this is one kernel (csrc/reverse_step.hip)
    whose z depends on (seed, step, row_base + row, column) only - not on the batch a row is in -
    and is truncated to [-top_p, top_p] when top_p > 0.  Anything else evaluates the same formula
    in fp32 PyTorch with ``noise`` or, without it, noise from a generator seeded with
    (seed, step): the same distribution, other bits, reproducible for the same batch.

    The multistep samplers (DPM-Solver++ 2M) add the previous update's x0 with ``a_prev != 0``:

        x0p = pred_prev  or  scale * weight[idx_prev]    (``weight`` and ``scale`` are shared with idx)
        y   = a * x0 + a_prev * x0p + b * x + s * z

    in the same kernel (a bf16 ``pred_prev`` or ids into the fp32 ``weight``; the two sources need
    not be of one kind); the term draws no noise.  With ``a_prev == 0`` the previous source is
    not looked at and the result is the three-term update's, bit for bit."""
    ref = next((t for t in (x, pred, x_start) if t is not None), None)
    if ref is None:
        raise ValueError("reverse_step: one of x, pred, x_start must be given (it fixes the shape)")
    if idx is not None and pred is None and weight is None:
        raise ValueError("reverse_step: idx needs weight")
    if mask is not None and x_start is None:
        raise ValueError("reverse_step: mask needs x_start")
    a, b, s, a_prev = float(a), float(b), float(s), float(a_prev)
    if (b != 0.0 and x is None) or (a != 0.0 and pred is None and idx is None):
        raise ValueError("reverse_step: b != 0 needs x, a != 0 needs pred or idx")
    if a_prev == 0.0:
        pred_prev = idx_prev = None
    elif pred_prev is None and idx_prev is None:
        raise ValueError("reverse_step: a_prev != 0 needs pred_prev or idx_prev")
    elif pred_prev is None and weight is None:
        raise ValueError("reverse_step: idx_prev needs weight")
    shape, dev = ref.shape, ref.device
    E = int(shape[-1])
    if _kernel_ok(dev, E, x, pred, idx, weight, x_start, noise) and _source_ok(pred_prev, idx_prev, weight):
        N = ref.numel() // E
        m = None if mask is None else mask.reshape(-1).to(torch.long).contiguous()
        ids = None if idx is None or pred is not None else idx.reshape(-1).to(torch.long).contiguous()
        hist = {}
        if a_prev != 0.0:
            hist = dict(a_prev=a_prev, pred_prev=_c(pred_prev),
                        idx_prev=None if pred_prev is not None else idx_prev.reshape(-1).to(torch.long).contiguous())
        gathers = ids is not None or hist.get("idx_prev") is not None
        out, out16 = get_ext().reverse_step(
            ref, N, E, x=_c(x), pred=_c(pred), idx=ids, W=weight.detach().contiguous() if gathers else None,
            x_start=_c(x_start), mask=m, scale=float(scale),
            a=a, b=b, s=s, seed=int(seed), step=int(step), row_base=int(row_base), tau=max(float(top_p), 0.0),
            erf_tau=_erf_tau(top_p) if top_p > 0 else 0.0, want_bf16=bool(want_bf16), **hist)
        return out.view(shape), (out16.view(shape) if want_bf16 else None)

    def source(p, i):
        if p is not None:
            return p.float()
        V = weight.shape[0]
        ok = (i >= 0) & (i < V)
        return float(scale) * weight.detach().float()[i.clamp(0, V - 1)] * ok.unsqueeze(-1)

    y = torch.zeros(shape, dtype=torch.float32, device=dev)
    if a != 0.0:
        y = y + a * source(pred, idx)
    if a_prev != 0.0:
        y = y + a_prev * source(pred_prev, idx_prev)
    if b != 0.0:
        y = y + b * x.float()
    if s != 0.0:
        if noise is None:
            noise = draw_noise(shape, dev, step_generator(seed, step, dev), top_p)
        y = y + s * noise.float()
    if mask is not None:
        y = torch.where(mask.unsqueeze(-1) == 0, x_start.float(), y)
    return y, (y.to(torch.bfloat16) if want_bf16 else None)


def _source_ok(pred, idx, weight):
    """An x0 source the kernel reads: a bf16 prediction, or ids into an fp32 table (or none)."""
    if pred is not None:
        return pred.dtype == torch.bfloat16
    return idx is None or weight.dtype == torch.float32


def _kernel_ok(dev, E, x, pred, idx, weight, x_start, noise):
    if dev.type != "cuda" or noise is not None or E % 4 != 0:
        return False
    if any(t is not None and t.dtype != torch.float32 for t in (x, x_start)):
        return False
    if not _source_ok(pred, idx, weight):
        return False
    ext = get_ext()
    if ext is None:
        return False
    if not hasattr(ext, "reverse_step"):
        raise RuntimeError("the native extension has no reverse_step kernel: rebuild it")
    return True


def timestep_embedding(timesteps, dim, max_period=10000):
    """Sinusoidal [cos | sin] timestep embedding [B, dim] in bf16."""
    return get_ext().timestep_emb(timesteps.float().contiguous(), int(dim), float(max_period))
