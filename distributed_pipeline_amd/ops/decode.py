"""
The two per-token ops of GPT-2 generation: single-query attention over a K/V cache, and the choice
of the next token.

Attention of one decode step
----------------------------
``attention_decode(qkv_new, k_cache, v_cache, lens, n_heads)`` appends the new token's key and
value to the caches (in place) and attends its query over everything cached so far:

* ``qkv_new`` [B, 3*H*D]: the token's packed projection, order [3][H][D] (the order of
  ``ops.nn.attention``'s ``qkv.view(B, L, 3, H, D)``);
* ``k_cache`` / ``v_cache`` [B, H, Lmax, D], possibly views into a larger buffer;
* ``lens`` int32 [B]: keys already cached per row.  It is NOT modified - the caller advances it
  with a device op, so a generation loop never synchronises with the host.

A row with ``0 <= lens[b] < Lmax`` stores the new k and v (bit for bit) at ``cache[b, :, lens[b]]``
and returns ``softmax(q K^T / sqrt(D)) V`` over the keys ``0 .. lens[b]``.  Any other ``lens[b]``
marks the row inactive (a finished, parked row): nothing is stored and its output is zeros.  Cache
rows beyond ``lens[b]`` never contribute, whatever they hold.

bf16 on a HIP device with D in {64, 128}: one kernel (csrc/attn_decode.hip).  Anything else (CPU,
fp32, other D, a cache whose rows are not packed): the same definition in fp32 PyTorch,
:func:`attention_decode_ref`.  Inference only: no autograd.

The next token: ``sample_tokens``
---------------------------------
``sample_tokens(logits [B, V], *, temperature, top_k=0, top_p=0.0, seed, step, row_base=0)`` draws
one id per row with noise that is a function of ``(seed, step, global row, id)`` alone.  For row b,
global row ``R = row_base + b`` (``seed``: its low 64 bits; ``step``: the index of the new token):

1. Scaling.  ``s_v = fp32(logit_v) / fp32(temperature)``, correctly rounded IEEE division (no
   reciprocal).  A NaN becomes -inf.  ``temperature == 0`` is ``utils.lm_sampling.greedy``.
2. Degenerate rows.  If the row's maximum is not finite (all -inf, or any +inf) the result is
   ``greedy``'s id for the row, ``thr`` is that maximum and ``kept`` is 0.  No path returns an id
   outside ``[0, V)``.
3. ``top_k``, when ``0 < top_k < V``: with kappa the ``top_k``-th largest s, keep ``s_v >= kappa``
   (ties with the k-th are kept, as in ``filter_top_k``).  Comparisons only: exact.  Any other
   ``top_k`` is off.
4. ``top_p``, when ``0 < fp32(top_p) < 1``, on what step 3 kept: ``m = max s``, ``w_v = exp(s_v - m)``,
   ``Z`` = the sum of w over the kept ids, ``G(x)`` = the sum of ``w_v`` over the kept ids with
   ``s_v > x``; keep v iff ``G(s_v) < top_p * Z``.  Equal logits are kept or dropped together and the
   maximum is always kept (``G(m) = 0``).  This differs from ``filter_top_p`` only for ties at the
   boundary, which that function splits by id.  Sums are fp32 in an order that is fixed per path
   (the kernel: per thread, then lanes, then waves; PyTorch: one cumulative sum down the sorted
   row), so the two paths can disagree where a mass lies within rounding of ``top_p * Z``.
5. The kept set is ``{v : s_v >= tau}`` for one tau per row, the smallest kept s: ``thr[b] = tau``,
   ``kept[b]`` = the size of the set.
6. The draw is Gumbel-max with counter-based uniforms.  One block of ``philox4`` (csrc/common.h)
   serves the ids ``4j .. 4j+3``: with ``V4 = ceil(V / 4)`` and the 64-bit group index
   ``grp = R * V4 + j`` it is ``philox4(seed_lo, step, grp_lo, grp_hi, seed_hi, SM_DOMAIN)`` - the
   layout of the decoding noise of csrc/reverse_step.hip under a domain constant of its own.  Word
   ``r[v & 3]`` gives ``u_v = (2 (r >> 9) + 1) / 2^24``, an odd integer below 2^24 over 2^24: exact
   in fp32 and strictly inside (0, 1).  ``g_v = -log(-log u_v)`` and the token is the arg-max of
   ``s_v + g_v`` (fp32) over the kept ids, ties to the lowest id.  ``u_v`` depends on
   ``(seed, step, R, v)`` and V only: not on B, on any launch geometry, or on training's RNG state.
   The two paths can disagree where two perturbed scores lie within rounding of each other.

fp32 or bf16 logits with last stride 1 (any row stride) and V <= 65536 on a HIP device: one kernel
per call (csrc/sample.hip), nothing read back to the host.  Anything else: the same definition in
PyTorch with the same uniform bits, :func:`sample_tokens_ref`.  ``sample_uniforms`` returns the
``u_v``, so tests and tools can pin the noise bit for bit.
"""
import math
import struct

import torch

from ._ext import get_ext

SM_DOMAIN = 0x536D706C  # csrc/sample.hip
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def attention_decode_ref(qkv_new, k_cache, v_cache, lens, n_heads):
    """The definition in fp32 PyTorch (any device, any dtype); also the numerics yardstick of
    the kernel's tests."""
    B, H, Lmax, D = k_cache.shape
    assert H == n_heads and qkv_new.shape == (B, 3 * H * D) and lens.shape == (B,)
    q, k, v = qkv_new.detach().reshape(B, 3, H, D).unbind(1)
    n = lens.long()
    active = (n >= 0) & (n < Lmax)
    at = n.clamp(0, Lmax - 1)
    rows = torch.arange(B, device=qkv_new.device)
    keep = active.view(B, 1, 1)
    # the append: an inactive row writes back what its slot already holds
    k_cache[rows, :, at] = torch.where(keep, k.to(k_cache.dtype), k_cache[rows, :, at])
    v_cache[rows, :, at] = torch.where(keep, v.to(v_cache.dtype), v_cache[rows, :, at])
    mask = (torch.arange(Lmax, device=qkv_new.device).view(1, Lmax) <= at.view(B, 1)).view(B, 1, Lmax)
    s = torch.einsum("bhd,bhld->bhl", q.float(), k_cache.float()) / math.sqrt(D)
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
    vf = torch.where(mask.unsqueeze(-1), v_cache.float(), 0.0)  # a NaN beyond lens must not reach the sum
    o = torch.einsum("bhl,bhld->bhd", p, vf)
    return torch.where(keep, o, 0.0).to(qkv_new.dtype).reshape(B, H * D)


@torch.no_grad()
def attention_decode(qkv_new, k_cache, v_cache, lens, n_heads):
    """-> out [B, H*D] in ``qkv_new``'s dtype; ``k_cache`` / ``v_cache`` updated in place."""
    if qkv_new.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None:
            if qkv_new.stride(-1) != 1 or qkv_new.stride(0) % 8 or qkv_new.data_ptr() % 16:
                qkv_new = qkv_new.contiguous()
            out = ext.attn_decode(qkv_new, k_cache, v_cache, lens, int(n_heads))
            if out is not None:
                return out
    return attention_decode_ref(qkv_new, k_cache, v_cache, lens, n_heads)


# ---- sample_tokens ------------------------------------------------------------------------------

def _s64(x):
    """The low 64 bits of a Python int as a signed int64 (two's complement)."""
    x = int(x) & _M64
    return x - (1 << 64) if x >> 63 else x


def _mulhilo(m, c):
    """(hi, lo) words of the 64-bit product m * c: m a 32-bit constant, c an int64 tensor of 32-bit
    values.  The product does not fit a signed int64, so c is split into 16-bit halves."""
    ch, cl = c >> 16, c & 0xFFFF
    ph, pl = ch * m, cl * m                    # < 2^48 each; product = ph * 2^16 + pl
    low = ((ph & 0xFFFF) << 16) + pl           # < 2^49
    return (ph >> 16) + (low >> 32), low & _M32


def _philox4(k0, k1, c0, c1, c2, c3):
    """csrc/common.h philox4 on int64 tensors (or ints) holding 32-bit words -> four words."""
    for _ in range(7):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def sample_uniforms_ref(seed, step, row_base, B, V, device="cpu"):
    """The uniforms of ``sample_tokens`` in integer tensor ops (any device) -> fp32 [B, V]."""
    seed = int(seed) & _M64
    V4 = (V + 3) // 4
    rows = torch.arange(B, dtype=torch.int64, device=device) + _s64(row_base)
    grp = rows.view(B, 1) * V4 + torch.arange(V4, dtype=torch.int64, device=device).view(1, V4)  # mod 2^64
    zero = torch.zeros_like(grp)
    r = _philox4(seed & _M32, int(step) & _M32, grp & _M32, (grp >> 32) & _M32, zero + (seed >> 32),
                 zero + SM_DOMAIN)
    r = torch.stack(r, -1).reshape(B, 4 * V4)[:, :V]
    return (2 * (r >> 9) + 1).float() * (1.0 / 16777216.0)


@torch.no_grad()
def sample_uniforms(seed, step, row_base, B, V, device="cpu"):
    """-> fp32 [B, V]: ``u_v`` of the module docstring for the rows ``row_base .. row_base + B - 1``.
    On a HIP device the kernel's own values (csrc/sample.hip, V <= 65536), elsewhere the replica."""
    device = torch.device(device)
    if device.type == "cuda":
        ext = get_ext()  # raises on a GPU without the built extension
        if ext is not None:
            out = ext.sample_uniforms(torch.empty(0, device=device), _s64(seed), int(step) & _M32, _s64(row_base),
                                      int(B), int(V))
            if out is not None:
                return out
    return sample_uniforms_ref(seed, step, row_base, B, V, device)


def _fp32(x):
    """The float nearest to ``x`` that fp32 holds (what a kernel argument becomes)."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


@torch.no_grad()
def sample_tokens_ref(logits, *, temperature, top_k=0, top_p=0.0, seed, step, row_base=0, uniforms=None):
    """The definition in PyTorch (any device, any float dtype) -> (tokens int64 [B], thr fp32 [B],
    kept int32 [B]).  ``uniforms``: the ``u_v`` to use instead of computing them."""
    from utils.lm_sampling import greedy
    B, V = logits.shape
    dev = logits.device
    s = logits.float() / torch.full((1,), float(temperature), dtype=torch.float32, device=dev)  # a true division
    s = torch.where(torch.isnan(s), float("-inf"), s) + 0.0  # -0 -> +0
    m = s.amax(-1, keepdim=True)
    thr = s.amin(-1, keepdim=True)
    if 0 < top_k < V:
        thr = torch.topk(s, int(top_k), dim=-1).values[:, -1:]
    p = _fp32(top_p)
    if 0.0 < p < 1.0:
        srt = torch.sort(s, dim=-1, descending=True).values
        w = torch.where(srt >= thr, torch.exp(srt - m), 0.0)
        csum = w.cumsum(-1)
        above = torch.cat([torch.zeros_like(csum[:, :1]), csum[:, :-1]], 1)  # mass in front of each position
        # the mass strictly above a value is the one in front of the first element of its run
        pos = torch.arange(V, device=dev).view(1, V)
        first = torch.where(torch.cat([torch.ones_like(srt[:, :1], dtype=torch.bool), srt[:, 1:] != srt[:, :-1]], 1),
                            pos, 0).cummax(-1).values
        keep = (above.gather(1, first) < csum[:, -1:] * p) & (srt >= thr)
        thr = srt.gather(1, (keep.sum(-1, keepdim=True) - 1).clamp(min=0))
    keep = s >= thr
    u = sample_uniforms(seed, step, row_base, B, V, dev) if uniforms is None else uniforms
    score = torch.where(keep, s - torch.log(-torch.log(u)), float("-inf"))
    best = score.amax(-1, keepdim=True)
    ids = torch.arange(V, device=dev)
    tok = torch.where(keep & (score == best), ids, V).amin(-1).clamp(max=V - 1)
    bad = ~torch.isfinite(m.squeeze(-1))
    tok = torch.where(bad, greedy(logits), tok)
    thr = torch.where(bad, m.squeeze(-1), thr.squeeze(-1))
    kept = torch.where(bad, 0, keep.sum(-1)).to(torch.int32)
    return tok, thr, kept


@torch.no_grad()
def sample_tokens(logits, *, temperature, top_k=0, top_p=0.0, seed, step, row_base=0, return_stats=False):
    """-> tokens int64 [B], or (tokens, thr fp32 [B], kept int32 [B]) with ``return_stats``."""
    if logits.dim() != 2:
        raise ValueError(f"logits must be [B, V], got {tuple(logits.shape)}")
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    B, V = logits.shape
    if temperature == 0:
        from utils.lm_sampling import greedy
        tok = greedy(logits)
        if not return_stats:
            return tok
        s = torch.where(torch.isnan(logits), float("-inf"), logits.float())
        return tok, s.amax(-1), torch.zeros(B, dtype=torch.int32, device=logits.device)
    k = int(top_k) if 0 < top_k < V else 0
    p = _fp32(top_p)
    p = p if 0.0 < p < 1.0 else 0.0
    if logits.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None and logits.dtype in (torch.float32, torch.bfloat16) and B > 0:
            x = logits if logits.stride(-1) == 1 else logits.contiguous()
            out = ext.sample_tokens(x, float(temperature), k, p, _s64(seed), int(step) & _M32, _s64(row_base),
                                    bool(return_stats))
            if out is not None:
                return tuple(out) if return_stats else out[0]
    out = sample_tokens_ref(logits, temperature=temperature, top_k=k, top_p=p, seed=seed, step=step,
                            row_base=row_base)
    return out if return_stats else out[0]
