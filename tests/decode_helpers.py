"""Shared by the generation tests: the float64 definition of ``ops.decode.attention_decode``,
caches allocated inside a pattern-filled buffer, and the tiny GPT-2 models."""
import math

import torch

# number of keys n = lens + 1 on both sides of every chunk of csrc/attn_decode.hip - keys per wave
# load (8 at D = 64, 4 at D = 128), per wave iteration (32 / 16), per workgroup iteration (128 / 64)
# - the edges of the issue's suggested structure (8 / 32 / 64), and the cache's first and last row
RAGGED_LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 1022, 1023]

PATTERN = 0x5A5A  # bf16 bits of the guard filling (a finite value)


def ref64(qkv_new, k_cache, v_cache, lens, H):
    """float64 softmax(q K^T / sqrt D) V over the cached keys 0 .. lens[b] - 1 and the new one;
    zeros for an inactive row.  The caches are read as they are before the call."""
    B, _, Lmax, D = k_cache.shape
    q, k, v = qkv_new.double().reshape(B, 3, H, D).unbind(1)
    out = torch.zeros(B, H, D, dtype=torch.float64, device=qkv_new.device)
    for b, n in enumerate(lens.tolist()):
        if not 0 <= n < Lmax:
            continue
        K = torch.cat([k_cache[b, :, :n].double(), k[b][:, None]], 1)
        Vv = torch.cat([v_cache[b, :, :n].double(), v[b][:, None]], 1)
        p = torch.softmax(torch.einsum("hd,hld->hl", q[b], K) / math.sqrt(D), -1)
        out[b] = torch.einsum("hl,hld->hd", p, Vv)
    return out.reshape(B, H * D)


def guarded_caches(B, H, Lmax, D, device, dtype=torch.bfloat16, spare=3):
    """(buf, k, v): k and v [B, H, Lmax, D] are views into ``buf`` [2, B, H, Lmax + 2 * spare, D],
    with ``spare`` rows in front of and behind every (b, h) block; everything holds PATTERN, so a
    stray store shows up as a changed pattern rather than as a fault."""
    shape = (2, B, H, Lmax + 2 * spare, D)
    if dtype == torch.bfloat16:
        buf = torch.full(shape, PATTERN, dtype=torch.int16, device=device).view(torch.bfloat16)
    else:
        buf = torch.full(shape, 1234.5, dtype=dtype, device=device)
    return buf, buf[0, :, :, spare:spare + Lmax], buf[1, :, :, spare:spare + Lmax]


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t


TINY = dict(model="gpt2", config_name="tiny", hidden_size=256, num_layers=2, vocab_size=3000, seq_len=256,
            dropout=0.0)


def teacher_forced(model, ids, plens, Lp):
    """prefill on the (zero-padded) prompts ``ids[b, :plens[b]]``, then decode steps fed each row's
    own next ids up to the last position -> {(b, position): logits [V]} for every fed position
    (the prompt's last one included)."""
    B, L = ids.shape
    dev = ids.device
    lens = torch.tensor(plens, dtype=torch.int32, device=dev)
    prompt = ids[:, :Lp].clone()
    prompt[torch.arange(Lp, device=dev).view(1, Lp) >= lens.view(B, 1)] = 0
    cache = model.init_cache(B, L, dev)
    got = {}
    logits = model.prefill(prompt, lens, cache)
    for b in range(B):
        got[(b, plens[b] - 1)] = logits[b].float()
    for t in range(L - min(plens)):
        pos = [p + t for p in plens]
        tok = torch.stack([ids[b, min(pos[b], L - 1)] for b in range(B)])
        logits = model.decode_step(tok, cache)
        for b in range(B):
            if pos[b] < L:
                got[(b, pos[b])] = logits[b].float()
    return got, cache
