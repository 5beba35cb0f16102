"""
Single-query attention over a K/V cache: the attention of one GPT-2 decode step.

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
"""
import math

import torch

from ._ext import get_ext


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
