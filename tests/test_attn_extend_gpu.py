"""csrc/attn_extend.hip (K-M27) against ``ref64_block`` in float64, and the model paths built on it.  The kernel
rounds its weights to bf16, as the native ``ops.nn.attention`` forward does: the yardstick is that forward on the
same bf16 values as one causal sequence of ``lens + T`` tokens at the same T positions, and the kernel's largest
absolute error may be at most twice the yardstick's in the same run.  Caches: views into a pattern-filled buffer."""
import functools
import math

import pytest
import torch

from decode_block_helpers import block_counts, ref64_block
from decode_helpers import PATTERN, bits, guarded_caches
from distributed_pipeline_amd.ops import nn as ops
from distributed_pipeline_amd.ops.decode import attention_extend
from test_generate_gpu import _models, _prompts
from utils.lm_sampling import greedy

pytestmark = pytest.mark.gpu
H, LMAX, SPARE, NAN = 2, 320, 3, 0x7FC0
LENS = [0, 1, 31, 32, 33, 127, 128, 129, 191]  # both sides of every 32-key tile edge and of the 4-wave round


def _inputs(D, kind, lens, T, g):
    """bf16 (qkv_new [n, T, 3 H D], k, v [n, H, LMAX, D]): unit-normal values, or a ``ramp`` whose scores climb by
    65 from key 0 to the run's last key, so the running maximum moves in every tile, wave and at the merge."""
    n, dev = len(lens), "cuda"
    q = torch.randn(n, T, H, D, device=dev, generator=g)
    k, v = (torch.randn(n, H, LMAX + T, D, device=dev, generator=g) for _ in range(2))
    at = torch.tensor(lens, device=dev).clamp(0, LMAX - 1).view(n, 1) + torch.arange(T, device=dev).view(1, T)
    if kind == "ramp":
        d = torch.randn(n, 1, H, D, device=dev, generator=g)
        last = at[:, -1].view(n, 1, 1).float()
        alpha = 65.0 * (torch.arange(LMAX + T, device=dev).view(1, 1, -1).clamp(max=last) / last.clamp(min=1) - 1.0)
        along = d[:, 0] * math.sqrt(D) / (d[:, 0] ** 2).sum(-1, keepdim=True)
        q, k = d + 0.05 * q, 0.01 * k + alpha.unsqueeze(-1) * along.unsqueeze(2)
    rows = torch.arange(n, device=dev).view(n, 1)
    qkv = torch.stack([q, k[rows, :, at], v[rows, :, at]], 2).reshape(n, T, 3 * H * D).bfloat16()
    return qkv, k[:, :, :LMAX].bfloat16(), v[:, :, :LMAX].bfloat16()


def _run(D, kind, lens, T, seed, counts=None, tail=PATTERN):
    """One call on guarded caches that hold ``tail`` from ``lens[b]`` on -> (out, float64 reference, the yardstick
    at the same positions, c, qkv, buffer before, buffer after); prints and checks the error bound."""
    qkv, k0, v0 = _inputs(D, kind, lens, T, torch.Generator(device="cuda").manual_seed(seed))
    n, c = len(lens), block_counts(lens, counts, T, LMAX)
    buf, k, v = guarded_caches(n, H, LMAX, D, "cuda", spare=SPARE)
    k.copy_(k0), v.copy_(v0)
    seq = torch.zeros(n, -(-(max(lens) + T) // 64) * 64, 3, H, D, dtype=torch.bfloat16, device="cuda")
    for b, m in enumerate(lens):
        if 0 <= m < LMAX:
            seq[b, :m, 1], seq[b, :m, 2] = k[b, :, :m].transpose(0, 1), v[b, :, :m].transpose(0, 1)
            seq[b, m:m + c[b]] = qkv[b, :c[b]].view(-1, 3, H, D)
            k.view(torch.int16)[b, :, m:], v.view(torch.int16)[b, :, m:] = tail, tail
    want, yard = ref64_block(qkv, k, v, lens, H, counts), torch.zeros(n, T, H * D, dtype=torch.float64, device="cuda")
    if D != 32:
        att = ops.attention(seq.flatten(2), H, 0.0, True, False)
        for b, m in enumerate(lens):
            yard[b, :c[b]] = att[b, m:m + c[b]].double() if c[b] else 0
    before = buf.clone()
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    out = attention_extend(qkv, k, v, torch.tensor(lens, dtype=torch.int32, device="cuda"), H, counts=cnt)
    e, e_yard = (out.double() - want).abs().max().item(), (yard - want).abs().max().item()
    print(f"D={D} T={T} {kind} lens={lens}: max |err| = {e:.4e}, ops.attention's = {e_yard:.4e}, ratio {e / e_yard:.3f}")
    assert D == 32 or e <= 2 * e_yard, (e, e_yard)
    return out, want, yard, c, qkv, before, buf


@pytest.mark.parametrize("T", [1, 9, 32, 33, 128])
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_against_float64(D, T):
    for kind in ("normal", "ramp"):
        for i in range(0, len(LENS), 3):
            _, _, _, c, _, before, after = _run(D, kind, LENS[i:i + 3], T, 100 * D + T + i)
            assert c == [T] * 3 and not torch.equal(bits(before), bits(after))


@pytest.mark.parametrize("D", [64, 128])
def test_counts_parked_rows_and_what_is_written(D):
    T, lens, counts = 9, [-1, LMAX, LMAX - 5, 33, 0, 100, 31, 64], [9, 9, 9, 0, 1, 12, -2, 5]
    out, _, _, c, qkv, before, after = _run(D, "normal", lens, T, D, counts=counts, tail=NAN)
    assert c == [0, 0, 5, 0, 1, 9, 0, 5] and torch.isfinite(out.float()).all()
    new = qkv.view(len(lens), T, 3, H, D)
    for b, m in enumerate(lens):
        assert not out[b, c[b]:].any()
        for j in range(c[b]):  # exactly these rows change, to the bits of qkv_new
            before[0, b, :, SPARE + m + j], before[1, b, :, SPARE + m + j] = new[b, j, 1], new[b, j, 2]
    assert torch.equal(bits(before), bits(after))


def test_bit_equality_strides_and_fallbacks():
    lens, T = [5, 130, 64], 40
    out0, _, _, _, qkv, before, after = _run(64, "normal", lens, T, 7)
    assert torch.equal(out0, _run(64, "normal", lens, T, 7)[0])
    n = torch.tensor(lens, dtype=torch.int32, device="cuda")
    inside = lambda buf: (buf[0, :, :, SPARE:SPARE + LMAX], buf[1, :, :, SPARE:SPARE + LMAX])  # noqa: E731
    wide = torch.zeros(3, T, qkv.shape[2] + 16, dtype=qkv.dtype, device="cuda")
    for pad in (8, 1):  # qkv_new as a column slice of a wider tensor: 16-byte aligned rows, and not
        wide[:, :, pad:pad + qkv.shape[2]] = qkv
        buf = before.clone()
        assert torch.equal(attention_extend(wide[:, :, pad:pad + qkv.shape[2]], *inside(buf), n, H), out0)
        assert torch.equal(bits(buf), bits(after))
    tall = torch.full((2, 6, H, LMAX, 64), 3.0, dtype=qkv.dtype, device="cuda")  # the caches as rows [1::2]
    tall[0, 1::2], tall[1, 1::2] = inside(before)
    assert torch.equal(attention_extend(qkv, tall[0, 1::2], tall[1, 1::2], n, H), out0) and (tall[:, 0::2] == 3.0).all()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((tall[0, 1::2], tall[1, 1::2]), inside(after)))
    _run(64, "normal", lens, 129, 8)  # a longer run: the PyTorch path within the same bound
    out, want = _run(32, "normal", lens, 9, 9)[:2]  # no native yardstick at D = 32: fp32 sums rounded once to bf16
    assert ((out.double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-5).all()
    k, v = inside(before)
    for bad in (lambda: attention_extend(qkv, k, v, n, H + 1), lambda: attention_extend(qkv, k, v, n[:2], H),
                lambda: attention_extend(qkv, k, v, n, H, counts=n.long())):
        with pytest.raises(ValueError):
            bad()


@functools.lru_cache(maxsize=None)
def _forwards(heads):
    ref, nat, _ = _models(heads)
    ids = torch.randint(1000, 3000, (4, 96), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with torch.no_grad():
        return ids, ref(ids).float(), nat(ids).float()


@pytest.mark.parametrize("C", [5, 32, 64])
@pytest.mark.parametrize("heads", [4, 2])
def test_chunked_prefill_teacher_forced_logits(heads, C):
    """test_generate_gpu.py's rule: the cached path's largest logit error against the fp32 model's full forward
    <= 2 x the native full forward's, over the same positions."""
    nat, (ids, want, full) = _models(heads)[1], _forwards(heads)
    plens, steps, rows = [1, 5, 64, 65], 6, torch.arange(4, device="cuda")
    lens = torch.tensor(plens, dtype=torch.int32, device="cuda")
    prompt = torch.where(torch.arange(65, device="cuda").view(1, 65) < lens.view(4, 1), ids[:, :65], 0)
    cache = nat.init_cache(4, 96)
    cache.buf.view(torch.int16).fill_(PATTERN)
    got = [nat.prefill(prompt, lens, cache, chunk=C).float()]
    got += [nat.decode_step(ids[rows, lens.long() + t], cache).float() for t in range(steps)]
    at = [lens.long() - 1 + t for t in range(steps + 1)]
    e_cached = max((g - want[rows, p]).abs().max().item() for g, p in zip(got, at))
    e_full = max((full[rows, p] - want[rows, p]).abs().max().item() for p in at)
    print(f"heads={heads} chunk={C}: cached max |err| = {e_cached:.4e}, native full forward max |err| = {e_full:.4e}")
    assert e_cached <= 2 * e_full, (e_cached, e_full)
    for b, n in enumerate(plens):  # nothing behind prompt + steps
        assert cache.lens[b] == n + steps and (bits(cache.buf[:, :, b, :, n + steps:]) == PATTERN).all()
        assert not (bits(cache.buf[:, :, b, :, :n + steps]) == PATTERN).all()


@pytest.mark.parametrize("heads", [4, 2])
def test_greedy_generate_with_a_chunked_prefill(heads):
    nat, (ids, lens) = _models(heads)[1], _prompts()
    a, b = (nat.generate(ids, lens, 12, temperature=0, prefill_chunk=32) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    cache, last = nat.init_cache(4, 52), [None] * 4
    for p0 in (0, 32):  # the loop written out: extend, the head on each row's last prompt position, decode steps
        hid = nat.extend(ids[:, p0:p0 + 32], cache, (lens - p0).clamp(0, min(32, 40 - p0)))
        for r, n in enumerate(lens.tolist()):
            if p0 < n <= p0 + 32:
                last[r] = hid[r, n - 1 - p0]
    assert cache.lens.tolist() == lens.tolist()
    logits, toks = ops.linear(torch.stack(last), nat.wte.weight), []
    for t in range(12):
        toks.append(greedy(logits))
        logits = nat.decode_step(toks[-1], cache)
    assert torch.equal(a[0], torch.stack(toks, 1))
    plain, zero = nat.generate(ids, lens, 12, temperature=0), nat.generate(ids, lens, 12, temperature=0, prefill_chunk=0)
    assert torch.equal(plain[0], zero[0]) and torch.equal(plain[1], zero[1])
