"""Shared by test_kv_fp8_cpu.py and test_kv_fp8_gpu.py: an independent yardstick of the one-byte K/V
cache format of ``ops.decode`` - ``math.frexp`` for the row exponent and a hand-written e4m3fn value
table with round-to-nearest-even, in numpy and Python, none of the op's code - the attention
definition in float64 on the dequantized caches, pattern-guarded caches, and the checks themselves,
written once for both devices."""
import math

import numpy as np
import torch

from distributed_pipeline_amd.ops import decode as dec

PAT = 0x5A  # the guard byte of codes and exponents (a finite code, exponent 90)
SPARE = 3
B, H = 3, 2
LMAX = 320

# ---- the format, independently ---------------------------------------------------------------------

# the 127 non-negative finite e4m3fn values by code 0x00 .. 0x7e (0x7f is NaN): 4 exponent bits of
# bias 7, 3 mantissa bits, subnormals m / 8 * 2^-6
E4M3 = np.array([(c & 7) / 8.0 * 2.0 ** -6 if (c >> 3) == 0 else (1 + (c & 7) / 8.0) * 2.0 ** ((c >> 3) - 7)
                 for c in range(127)], dtype=np.float64)
assert E4M3[126] == 448.0 and E4M3[1] == 2.0 ** -9 and (np.diff(E4M3) > 0).all()


def yard_exponent(a):
    """The row exponent of the largest magnitude ``a`` (a Python float)."""
    if a == 0.0:
        return 0
    m, p = math.frexp(a)
    return max(p - 9 + (1 if m > 0.875 else 0), -127)


def yard_round(y):
    """float64 array -> e4m3fn codes, round to nearest, ties to the even code, sign kept (-0 included)."""
    mag = np.abs(y)
    assert (mag <= 448.0).all(), "the format never saturates"
    hi = np.clip(np.searchsorted(E4M3, mag, side="left"), 0, 126)  # first value >= mag
    lo = np.clip(hi - 1, 0, 126)
    d_hi, d_lo = E4M3[hi] - mag, mag - E4M3[lo]
    code = np.where(d_hi < d_lo, hi, np.where(d_lo < d_hi, lo, np.where(hi % 2 == 0, hi, lo)))
    code = np.where(E4M3[hi] == mag, hi, code)
    return (code + 128 * np.signbit(y)).astype(np.uint8)


def yard_quantize(x):
    """torch [..., D] (any float dtype, any device) -> (codes uint8 [..., D], exps int8 [...]) as numpy."""
    xd = x.detach().cpu().double().numpy()  # converted on the host: no device arithmetic on a subnormal
    flat = xd.reshape(-1, xd.shape[-1])
    exps = np.array([yard_exponent(float(np.abs(r).max())) for r in flat], dtype=np.int64)
    codes = yard_round(np.ldexp(flat, -exps[:, None]))  # float64: the scaling is exact
    return codes.reshape(xd.shape), exps.astype(np.int8).reshape(xd.shape[:-1])


def yard_dequantize(codes, exps):
    """numpy codes / exps -> float64 values; a NaN code gives NaN."""
    table = np.concatenate([E4M3, [np.nan]])
    val = table[codes & 127] * np.where(codes >= 128, -1.0, 1.0)
    return np.ldexp(val, exps.astype(np.int64)[..., None])


def yard_attention(qkv_new, k8, ke, v8, ve, lens, heads):
    """The definition in float64 on the caches as they are before the call -> (out [B, H * D] float64
    tensor on the CPU, new codes / exps of k and v as numpy)."""
    nb, _, lmax, D = k8.shape
    q, k, v = qkv_new.detach().cpu().double().reshape(nb, 3, heads, D).unbind(1)
    (kc, kx), (vc, vx) = yard_quantize(k), yard_quantize(v)
    k8n, ken, v8n, ven = (t.detach().cpu().numpy() for t in (k8, ke, v8, ve))
    out = torch.zeros(nb, heads, D, dtype=torch.float64)
    for b, n in enumerate(lens.tolist()):
        if not 0 <= n < lmax:
            continue
        K = np.concatenate([yard_dequantize(k8n[b, :, :n], ken[b, :, :n]), yard_dequantize(kc[b], kx[b])[:, None]], 1)
        V = np.concatenate([yard_dequantize(v8n[b, :, :n], ven[b, :, :n]), yard_dequantize(vc[b], vx[b])[:, None]], 1)
        K, V = torch.from_numpy(K), torch.from_numpy(V)
        p = torch.softmax(torch.einsum("hd,hld->hl", q[b], K) / math.sqrt(D), -1)
        out[b] = torch.einsum("hl,hld->hd", p, V)
    return out.reshape(nb, heads * D), (kc, kx, vc, vx)


def t8(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- the quantizer, bit for bit ------------------------------------------------------------------------

def quantizer_rows(D, seed=0):
    """About 200 fp32 rows of D values (every value a bf16 but 449 2^k): unit normals and the planted
    rows of the module docstring of the tests."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(120, D, generator=g).bfloat16().float(), torch.zeros(2, D)]
    for k in (-20, -3, 0, 5, 30):  # both sides of the 0.875 mantissa boundary
        for top in (448.0, 449.0, 450.0, 447.0):
            r = torch.randn(1, D, generator=g).clamp(-3, 3).bfloat16().float() * 2.0 ** (k + 6)
            r[0, int(torch.randint(D, (1,), generator=g))] = top * 2.0 ** k * (-1.0 if k == 5 else 1.0)
            rows.append(r)
    tiny = torch.zeros(2, D)
    tiny[0, 3], tiny[0, 7], tiny[0, 9] = 2.0 ** -130, 2.0 ** -131, -2.0 ** -133  # below the clamp
    tiny[1, 0], tiny[1, 5] = 2.0 ** -119, -2.0 ** -126
    big = (torch.randn(2, D, generator=g).clamp(-3, 3) * 2.0 ** 117).bfloat16().float()
    big[0, D - 1] = 2.0 ** 120
    big[1, 1] = -(2.0 ** 127) * 1.75  # 448 2^119: the largest magnitude whose dequantized row fp32 holds for sure
    rows += [tiny, big]
    out = torch.randn(20, D, generator=g).bfloat16().float()
    out[torch.arange(20), torch.randint(D, (20,), generator=g)] *= 1000.0  # the rest: subnormal codes and zero
    rows.append(out.bfloat16().float())
    # a row maximum of 256 has e = 0, so every other element is its own scaled value: the midpoints of
    # adjacent codes (exact ties, both signs) and negative values that round to zero
    mids = ((E4M3[:-1] + E4M3[1:]) / 2)
    mids = mids[mids < 256]
    vals = np.concatenate([mids, -mids, [-2.0 ** -11, -2.0 ** -12, -2.0 ** -20, -2.0 ** -10, 2.0 ** -11, -0.0],
                           E4M3[:120], -E4M3[:120]])
    pad = (-len(vals)) % (D - 1)
    vals = torch.from_numpy(np.concatenate([vals, np.zeros(pad)])).float().view(-1, D - 1)
    rows.append(torch.cat([vals[:, :5], torch.full((vals.shape[0], 1), 256.0), vals[:, 5:]], 1))
    # the same ties under a row exponent of 11 and of -30
    rows.append(rows[-1] * 2.0 ** 11)
    rows.append(rows[-2] * 2.0 ** -30)
    return torch.cat(rows)


def check_quantizer(device, D, dtype):
    x = quantizer_rows(D).to(dtype).to(device)
    want_c, want_e = yard_quantize(x)
    codes, exps = dec.kv_quantize(x)
    assert codes.dtype == torch.uint8 and exps.dtype == torch.int8 and codes.shape == x.shape and exps.shape == x.shape[:-1]
    bad_e = (exps.cpu().numpy() != want_e).nonzero()[0]
    assert bad_e.size == 0, (bad_e[:8], exps.cpu().numpy()[bad_e[:8]], want_e[bad_e[:8]])
    diff = np.argwhere(codes.cpu().numpy() != want_c)
    assert diff.size == 0, [(int(r), int(c), float(x[r, c]), int(codes[r, c]), int(want_c[r, c])) for r, c in diff[:8]]
    # what the format promises: a 2^-e in (224, 448] for every non-zero row above the clamp
    a = x.cpu().double().abs().amax(-1).numpy()
    live = (a > 0) & (want_e > -127)
    scaled = np.ldexp(a[live], -want_e[live].astype(np.int64))
    assert live.sum() > 150 and (scaled > 224).all() and (scaled <= 448).all()
    # the planted classes are there: subnormal codes, zeros of both signs, the largest code, the clamp
    mag = want_c & 127
    assert (mag == 126).any() and ((mag > 0) & (mag < 8)).any() and (want_c == 128).any() and (want_e == -127).any()
    # the dequantizer is the table, exactly
    back = dec.kv_dequantize(codes, exps)
    assert back.dtype == torch.float32
    assert np.array_equal(back.cpu().double().numpy(), yard_dequantize(want_c, want_e))
    # the PyTorch twin agrees with the op on this device, and two calls agree
    ref_c, ref_e = dec.kv_quantize_ref(x)
    assert torch.equal(ref_e, exps)
    diff = (ref_c != codes).nonzero().tolist()
    assert not diff, [(r, c, float(x[r, c]), int(exps[r]), int(ref_c[r, c]), int(codes[r, c])) for r, c in diff[:8]]
    again = dec.kv_quantize(x)
    assert torch.equal(again[0], codes) and torch.equal(again[1], exps)


# ---- guarded caches ------------------------------------------------------------------------------------

def guarded_fp8(nb, heads, lmax, D, device):
    """(cbuf, ebuf, k8, ke, v8, ve): code views [nb, heads, lmax, D] into cbuf [2, nb, heads, lmax + 2 SPARE, D]
    and exponent views [nb, heads, lmax] into ebuf [2, nb, heads, lmax + 2 SPARE], everything PAT."""
    cbuf = torch.full((2, nb, heads, lmax + 2 * SPARE, D), PAT, dtype=torch.uint8, device=device)
    ebuf = torch.full((2, nb, heads, lmax + 2 * SPARE), PAT, dtype=torch.int8, device=device)
    sl = slice(SPARE, SPARE + lmax)
    return cbuf, ebuf, cbuf[0, :, :, sl], ebuf[0, :, :, sl], cbuf[1, :, :, sl], ebuf[1, :, :, sl]


def check_kv_store(device, D, dtype):
    L, lens = 70, (1, 64, 70)
    g = torch.Generator().manual_seed(11)
    # a position stride wider than 3 H D, as the padded prefill's [:, :Lp] view has a wider batch stride
    wide = torch.randn(B, L + 2, 3 * H * D + 8, generator=g).to(dtype).to(device)
    qkv = wide[:, :L, :3 * H * D]
    cbuf, ebuf, k8, ke, v8, ve = guarded_fp8(B, H, LMAX, D, device)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=device)
    want_c, want_e = cbuf.clone(), ebuf.clone()
    kv = qkv.reshape(B, L, 3, H, D)
    for w in (0, 1):
        c, e = yard_quantize(kv[:, :, 1 + w])  # [B, L, H, D], [B, L, H]
        for b, n in enumerate(lens):
            want_c[w, b, :, SPARE:SPARE + n] = t8(c[b, :n].transpose(1, 0, 2), device)
            want_e[w, b, :, SPARE:SPARE + n] = t8(e[b, :n].transpose(1, 0), device)
    dec.kv_store(qkv, lens_t, k8, ke, v8, ve)
    assert torch.equal(cbuf, want_c) and torch.equal(ebuf, want_e)
    assert lens_t.tolist() == list(lens)
    # the PyTorch twin writes the same bytes
    cb2, eb2, *views = guarded_fp8(B, H, LMAX, D, device)
    dec.kv_store_ref(qkv, lens_t, *views)
    assert torch.equal(cb2, want_c) and torch.equal(eb2, want_e)


# ---- attention over the cache ------------------------------------------------------------------------------

def chunk_lens(D):
    """``lens`` on both sides of every chunk of csrc/attn_decode_fp8.hip, from its own constants - keys
    per wave load (64 lanes / (D / 8 lanes per key)), per wave iteration (AD_U = 4 loads) and per
    workgroup iteration (AD_WAVES = 4 waves), and the multiples of the last that fit - plus the cache's
    first and last row; a multiple of B values."""
    kpw = 64 // (D // 8)
    wk, it = 4 * kpw, 16 * kpw
    edges = {kpw, wk, it} | set(range(2 * it, LMAX, it))
    lens = sorted({0, 1, 2, LMAX - 2, LMAX - 1} | {e + d for e in edges for d in (-1, 0, 1) if 0 <= e + d < LMAX})
    spare = [12, 13]  # on no edge at either D
    while len(lens) % B:
        lens.append(spare.pop())
    return lens


def attn_inputs(D, kind, lens, g, device, dtype):
    """(qkv_new, k, v) in ``dtype`` on ``device``: ``normal`` - unit normals; ``ramp`` - keys along q whose
    scores climb by 65 from the first cached key to the new (last) one, so the running maximum moves at
    every fold and every merge (the set of test_attn_decode_gpu.py)."""
    n = len(lens)
    q = torch.randn(n, H, D, generator=g)
    v = torch.randn(n, H, LMAX + 1, D, generator=g)
    if kind == "normal":
        k = torch.randn(n, H, LMAX + 1, D, generator=g)
    else:
        cnt = torch.tensor(lens).clamp(0, LMAX - 1).view(n, 1, 1).float()
        j = torch.arange(LMAX + 1).view(1, 1, -1).float()
        alpha = 65.0 * ((j + 1).clamp(max=cnt + 1) / (cnt + 1) - 1.0)
        along = q * math.sqrt(D) / (q * q).sum(-1, keepdim=True)
        k = 0.01 * torch.randn(n, H, LMAX + 1, D, generator=g) + alpha.unsqueeze(-1) * along.unsqueeze(2)
    at = torch.tensor(lens).clamp(0, LMAX - 1)
    rows = torch.arange(n)
    qkv = torch.stack([q, k[rows, :, at], v[rows, :, at]], 1).reshape(n, 3 * H * D)
    return tuple(t.to(dtype).to(device) for t in (qkv, k[:, :, :LMAX], v[:, :, :LMAX]))


def attn_run(D, kind, lens, g, device, dtype, fn, tail=None):
    """One call of ``fn`` (the op, or the kernel's binding) on guarded caches filled by the yardstick's
    quantizer -> everything the checks need."""
    qkv, k0, v0 = attn_inputs(D, kind, lens, g, device, dtype)
    n = len(lens)
    cbuf, ebuf, k8, ke, v8, ve = guarded_fp8(n, H, LMAX, D, device)
    for c8, ce, src in ((k8, ke, k0), (v8, ve, v0)):
        c, e = yard_quantize(src)
        c8.copy_(t8(c, device))
        ce.copy_(t8(e, device))
    if tail is not None:  # (code byte, exponent byte) at and beyond lens[b] before the call
        for b, m in enumerate(lens):
            if 0 <= m < LMAX:
                for c8, ce in ((k8, ke), (v8, ve)):
                    c8[b, :, m:] = tail[0]
                    ce[b, :, m:] = tail[1]
    lens_t = torch.tensor(lens, dtype=torch.int32, device=device)
    want, new = yard_attention(qkv, k8, ke, v8, ve, lens_t, H)
    # the fp32 PyTorch path on the same inputs sets the arithmetic slack, never the code under test
    scratch = [t.clone() for t in (k8, ke, v8, ve)]
    e32 = (dec.attention_decode_fp8_ref(qkv.float(), *scratch, lens_t, H).double().cpu() - want).abs().max().item()
    before_c, before_e = cbuf.clone(), ebuf.clone()
    out = fn(qkv, k8, ke, v8, ve, lens_t, H)
    return dict(qkv=qkv, lens=lens, lens_t=lens_t, out=out, want=want, e32=e32, new=new, before_c=before_c,
                before_e=before_e, cbuf=cbuf, ebuf=ebuf, views=(k8, ke, v8, ve))


def expected_buffers(r, device):
    """The guarded buffers after the call: the rows lens[b] of the active rows hold the yardstick's codes
    and exponents of the new k and v, every other byte is what it was."""
    kc, kx, vc, vx = r["new"]
    want_c, want_e = r["before_c"].clone(), r["before_e"].clone()
    for b, m in enumerate(r["lens"]):
        if 0 <= m < LMAX:
            want_c[0, b, :, SPARE + m], want_c[1, b, :, SPARE + m] = t8(kc[b], device), t8(vc[b], device)
            want_e[0, b, :, SPARE + m], want_e[1, b, :, SPARE + m] = t8(kx[b], device), t8(vx[b], device)
    return want_c, want_e


def within_tolerance(r, e32, rows=None):
    """err / tol, tol = 2^-8 |want| + 4 e32: one bf16 ulp of the float64 yardstick (the rule of
    test_attn_decode_gpu.py) plus four times the fp32 PyTorch path's error on the same inputs.  An fp32
    output has no bf16 rounding but keeps the bound."""
    out, want = r["out"].double().cpu(), r["want"]
    if rows is not None:
        out, want = out[rows], want[rows]
    return ((out - want).abs() / (2.0 ** -8 * want.abs() + 4 * e32)).max().item()


# ---- the model -------------------------------------------------------------------------------------------

def fill_pattern(cache):
    cache.buf.fill_(PAT)
    cache.ebuf.fill_(PAT)


def teacher_forced_on(model, ids, plens, Lp, cache):
    """decode_helpers.teacher_forced on a given cache -> {(b, position): logits [V]}."""
    nb, L = ids.shape
    dev = ids.device
    lens = torch.tensor(plens, dtype=torch.int32, device=dev)
    prompt = ids[:, :Lp].clone()
    prompt[torch.arange(Lp, device=dev).view(1, Lp) >= lens.view(nb, 1)] = 0
    got = {}
    logits = model.prefill(prompt, lens, cache)
    for b in range(nb):
        got[(b, plens[b] - 1)] = logits[b].float()
    for t in range(L - min(plens)):
        pos = [p + t for p in plens]
        tok = torch.stack([ids[b, min(pos[b], L - 1)] for b in range(nb)])
        logits = model.decode_step(tok, cache)
        for b in range(nb):
            if pos[b] < L:
                got[(b, pos[b])] = logits[b].float()
    return got


@torch.no_grad()
def uncached_fp8_logits(model, seq, plen):
    """fp32 model, no cache: the logits [L, V] of one sequence under the definition - a position below
    ``plen`` (the prompt, run by the prefill) attends over the keys and values as they are, a later one
    over the yardstick's dequantized keys and values of every position up to its own."""
    from distributed_pipeline_amd.ops import nn as ops
    L = seq.shape[0]
    heads = model.cfg["num_heads"]
    causal = torch.ones(L, L, dtype=torch.bool, device=seq.device).tril()
    late = (torch.arange(L, device=seq.device) >= plen).view(1, L, 1)

    def attend(i, qkv):
        D = qkv.shape[-1] // (3 * heads)
        q, k, v = qkv.view(L, 3, heads, D).float().unbind(1)
        outs = []
        for kk, vv in ((k, v), tuple(
                torch.from_numpy(yard_dequantize(*yard_quantize(t))).float().to(seq.device) for t in (k, v))):
            s = torch.einsum("qhd,khd->hqk", q, kk) / math.sqrt(D)
            p = torch.softmax(s.masked_fill(~causal, float("-inf")), -1)
            outs.append(torch.einsum("hqk,khd->qhd", p, vv).reshape(1, L, heads * D))
        return torch.where(late, outs[1], outs[0]).to(qkv.dtype)

    dt = model.compute_dtype
    ln0 = model.h[0].ln_1
    x, a = ops.residual_layernorm(model.wte(seq.view(1, L), dt), None, ln0.weight, ln0.bias, 0.0, ln0.eps, False,
                                  pos=model.wpe(model.position_ids[:, :L], dt))
    a = model._blocks(x, a, attend)
    return ops.linear(a.view(L, -1), model.wte.weight).float()
