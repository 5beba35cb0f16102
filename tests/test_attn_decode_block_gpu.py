"""csrc/attn_decode_block.hip (KV-cache append + attention of a block of T new tokens per row)
against a float64 evaluation of the definition on the same bf16 inputs, and bit for bit against the
T sequential calls of csrc/attn_decode.hip that define it.

Allowed error per element, the rule of test_attn_decode_gpu.py: ``2^-8 |o_ref| + 4 e32`` - one bf16
ulp of the reference plus four times ``e32``, the largest absolute error of the fp32 PyTorch path
(``attention_decode_block_ref`` on fp32 copies of the same inputs) against the same float64
reference, over the input set.

Every cache is a view into a larger buffer that holds a bit pattern, with spare rows in front of
and behind each (b, h) block; before a call the rows at and beyond ``lens[b]`` hold the pattern too
(a huge finite value), so a key of the block that was read from the cache instead of ``qkv_new``, or
a stray store, shows.
"""
import functools
import math

import pytest
import torch

from decode_block_helpers import block_counts, ref64_block
from decode_helpers import PATTERN, bits, guarded_caches
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import attention_decode_block, attention_decode_block_ref

pytestmark = pytest.mark.gpu

B, H, LMAX, SPARE = 3, 2, 1024, 3
# the window lens .. lens + T - 1 on both sides of every chunk edge of the kernel, at more than one
# offset - keys per wave load (8 at D = 64, 4 at D = 128), per wave iteration (32 / 16), per
# workgroup iteration (128 / 64) - and the cache's first and last rows
BLOCK_LENS = [0, 1, 3, 6, 7, 8, 14, 15, 16, 29, 31, 32, 61, 63, 64, 125, 127, 128, 250, 255, 1015, 1016, 1019, 1023]


def _inputs(D, kind, lens, T, g):
    """bf16 (qkv_new [n, T, 3 H D], k, v): ``normal`` - unit-normal q, k, v; ``ramp`` - the queries
    of a row lie close to one direction and the keys along it, with scores that climb by 65 from
    the first cached key through the T new ones, so for the last query every later chunk of keys
    raises the running maximum: in every lane group, at the group merge and at the wave merge."""
    dev = "cuda"
    n = len(lens)
    q = torch.randn(n, 1, H, D, device=dev, generator=g)
    v = torch.randn(n, H, LMAX + T, D, device=dev, generator=g)
    if kind == "normal":
        qs = torch.randn(n, T, H, D, device=dev, generator=g)
        k = torch.randn(n, H, LMAX + T, D, device=dev, generator=g)
    else:
        qs = q + 0.05 * torch.randn(n, T, H, D, device=dev, generator=g)
        qs[:, T - 1] = q[:, 0]
        cnt = torch.tensor(lens, device=dev).clamp(0, LMAX - 1).view(n, 1, 1).float() + (T - 1)  # keys before the last
        j = torch.arange(LMAX + T, device=dev).view(1, 1, -1).float()
        alpha = 65.0 * ((j + 1).clamp(max=cnt + 1) / (cnt + 1) - 1.0)                            # 0 at the last key
        along = q[:, 0] * math.sqrt(D) / (q[:, 0] * q[:, 0]).sum(-1, keepdim=True)
        k = 0.01 * torch.randn(n, H, LMAX + T, D, device=dev, generator=g) + alpha.unsqueeze(-1) * along.unsqueeze(2)
    at = torch.tensor(lens, device=dev).clamp(0, LMAX - 1).view(n, 1) + torch.arange(T, device=dev).view(1, T)
    rows = torch.arange(n, device=dev).view(n, 1)
    knew, vnew = k[rows, :, at], v[rows, :, at]  # [n, T, H, D]
    qkv = torch.stack([qs, knew, vnew], 2).reshape(n, T, 3 * H * D).bfloat16()
    return qkv, k[:, :, :LMAX].bfloat16(), v[:, :, :LMAX].bfloat16()


def _sequential(qkv, before, lens, c, D):
    """The T plain calls on a copy of the guarded buffer -> (out [n, T, H D], buffer)."""
    buf = before.clone()
    k, v = buf[0, :, :, SPARE:SPARE + LMAX], buf[1, :, :, SPARE:SPARE + LMAX]
    outs = []
    for j in range(qkv.shape[1]):
        lj = torch.tensor([m + j if j < c[b] else -1 for b, m in enumerate(lens)], dtype=torch.int32, device="cuda")
        outs.append(get_ext().attn_decode(qkv[:, j], k, v, lj, H))
        assert outs[-1] is not None
    return torch.stack(outs, 1), buf


def _run(D, kind, lens, T, g, counts=None, tail=None, poison_idle_tokens=False):
    """One kernel call on guarded caches -> everything the checks need."""
    qkv, k0, v0 = _inputs(D, kind, lens, T, g)
    n = len(lens)
    c = block_counts(lens, counts, T, LMAX)
    buf, k, v = guarded_caches(n, H, LMAX, D, "cuda", spare=SPARE)
    k.copy_(k0)
    v.copy_(v0)
    for b, m in enumerate(lens):
        if 0 <= m < LMAX:
            k.view(torch.int16)[b, :, m:] = PATTERN
            v.view(torch.int16)[b, :, m:] = PATTERN
            if tail is not None:  # the bf16 bits at and beyond lens[b] + c_b before the call
                k.view(torch.int16)[b, :, m + c[b]:] = tail
                v.view(torch.int16)[b, :, m + c[b]:] = tail
        if poison_idle_tokens and tail is not None:
            qkv.view(torch.int16)[b, c[b]:] = tail
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    counts_t = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    want = e32 = None
    if tail is None:
        want = ref64_block(qkv, k, v, lens, H, counts)
        e32 = (attention_decode_block_ref(qkv.float(), k.float(), v.float(), lens_t, H, counts=counts_t).double()
               - want).abs().max().item()
    before = buf.clone()
    seq_out, seq_buf = _sequential(qkv, before, lens, c, D)
    out = get_ext().attn_decode_block(qkv, k, v, lens_t, H, counts_t)
    assert out is not None, "the kernel must take bf16 D in {64, 128}"
    torch.cuda.synchronize()
    return dict(qkv=qkv, lens=lens, c=c, lens_t=lens_t, counts_t=counts_t, out=out, want=want, e32=e32,
                before=before, after=buf, seq_out=seq_out, seq_buf=seq_buf)


@functools.lru_cache(maxsize=None)
def _ragged(D, kind, T):
    g = torch.Generator(device="cuda").manual_seed(1000 * D + 10 * T + len(kind))
    return [_run(D, kind, BLOCK_LENS[i:i + B], T, g) for i in range(0, len(BLOCK_LENS), B)]


def _check_buffer(r, D):
    """Exactly the rows lens .. lens + c_b - 1 changed, to the bits of qkv_new."""
    n, T = r["qkv"].shape[:2]
    new = r["qkv"].view(n, T, 3, H, D)
    expect = r["before"].clone()
    for b, m in enumerate(r["lens"]):
        for j in range(r["c"][b]):
            expect[0, b, :, SPARE + m + j], expect[1, b, :, SPARE + m + j] = new[b, j, 1], new[b, j, 2]
    assert torch.equal(bits(r["after"]), bits(expect))


@pytest.mark.parametrize("kind", ["normal", "ramp"])
@pytest.mark.parametrize("T", [2, 3, 5, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_matches_float64(D, T, kind):
    runs = _ragged(D, kind, T)
    e32 = max(r["e32"] for r in runs)
    worst = 0.0
    for r in runs:
        err = (r["out"].double() - r["want"]).abs()
        tol = 2.0 ** -8 * r["want"].abs() + 4 * e32
        worst = max(worst, (err / tol).max().item())
        if kind == "ramp":  # the set is what it claims, for the last query of each block
            new = r["qkv"].double().view(B, T, 3, H, D)
            for b, m in enumerate(r["lens"]):
                c = r["c"][b]
                if m >= 64 and c == T:
                    q = new[b, T - 1, 0]
                    keys = torch.cat([r["before"][0, b, :, SPARE:SPARE + m].double(), new[b, :T - 1, 1].transpose(0, 1)], 1)
                    s = torch.einsum("hd,hld->hl", q, keys) / math.sqrt(D)
                    s_new = (q * new[b, T - 1, 1]).sum(-1) / math.sqrt(D)
                    assert (s_new > s.amax(-1)).all() and (s_new - s.amin(-1) > 60).all()
    print(f"attn_decode_block D={D} T={T} {kind}: e32={e32:.3e} worst err/tol={worst:.3f}")
    assert worst <= 1.0, (worst, e32)


@pytest.mark.parametrize("kind", ["normal", "ramp"])
@pytest.mark.parametrize("T", [2, 3, 5, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_equals_the_sequential_plain_calls_bit_for_bit(D, T, kind):
    diff = 0
    for r in _ragged(D, kind, T):
        _check_buffer(r, D)
        assert r["lens_t"].tolist() == list(r["lens"])
        assert torch.equal(bits(r["after"]), bits(r["seq_buf"]))
        diff += (bits(r["out"]) != bits(r["seq_out"])).sum().item()
    print(f"attn_decode_block D={D} T={T} {kind}: {diff} output elements differ from the sequential calls")
    assert diff == 0


@pytest.mark.parametrize("D", [64, 128])
def test_one_token_is_the_plain_call(D):
    for i in range(0, len(BLOCK_LENS), B):
        g = torch.Generator(device="cuda").manual_seed(5 + i)
        r = _run(D, "normal", BLOCK_LENS[i:i + B], 1, g)
        assert torch.equal(bits(r["out"]), bits(r["seq_out"])) and torch.equal(bits(r["after"]), bits(r["seq_buf"]))
        _check_buffer(r, D)
    # with counts it is the block kernel: the same bits, and zeros where counts is 0
    g = torch.Generator(device="cuda").manual_seed(6)
    r = _run(D, "normal", (129, 7, 1023, 40), 1, g, counts=(1, 0, 5, 1))
    assert r["c"] == [1, 0, 1, 1] and not bits(r["out"][1]).any()
    assert torch.equal(bits(r["out"]), bits(r["seq_out"])) and torch.equal(bits(r["after"]), bits(r["seq_buf"]))
    _check_buffer(r, D)


@pytest.mark.parametrize("T", [5, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_counts(D, T):
    lens = (100, 1020, 1023, -1, LMAX, LMAX + 5, 37, 64, 5, 200, 300, 1017)
    counts = (T, T, T, 3, T, 2, 1, 0, T + 3, 3, 4, -2)
    g = torch.Generator(device="cuda").manual_seed(20 + T)
    r = _run(D, "normal", lens, T, g, counts=counts)
    assert r["c"] == [T, 4, 1, 0, 0, 0, 1, 0, T, 3, 4, 0]
    for b, c in enumerate(r["c"]):
        assert not bits(r["out"][b, c:]).any()  # zeros, bit for bit
        if c:
            err = (r["out"][b, :c].double() - r["want"][b, :c]).abs()
            assert (err <= 2.0 ** -8 * r["want"][b, :c].abs() + 4 * r["e32"]).all()
    _check_buffer(r, D)
    assert r["lens_t"].tolist() == list(lens) and r["counts_t"].tolist() == list(counts)
    assert torch.equal(bits(r["out"]), bits(r["seq_out"])) and torch.equal(bits(r["after"]), bits(r["seq_buf"]))
    # the active rows do not depend on their inactive neighbours
    act = [b for b, c in enumerate(r["c"]) if c]
    _, k, v = guarded_caches(len(act), H, LMAX, D, "cuda", spare=SPARE)
    k.copy_(r["before"][0, act, :, SPARE:SPARE + LMAX])
    v.copy_(r["before"][1, act, :, SPARE:SPARE + LMAX])
    alone = get_ext().attn_decode_block(r["qkv"][act].contiguous(), k, v, r["lens_t"][act].contiguous(), H,
                                        r["counts_t"][act].contiguous())
    assert torch.equal(bits(alone), bits(r["out"][act]))


@pytest.mark.parametrize("D", [64, 128])
def test_rows_beyond_the_block_are_never_read(D):
    lens, counts, T = (0, 33, 1000, 1021, 250), (8, 3, 8, 8, 0), 8
    outs = []
    for tail in (0, 0x7FC0, -1):  # zeros, a quiet NaN, all ones (a NaN too)
        g = torch.Generator(device="cuda").manual_seed(7)
        r = _run(D, "normal", lens, T, g, counts=counts, tail=tail, poison_idle_tokens=True)
        outs.append(r["out"])
        assert torch.equal(bits(r["out"]), bits(r["seq_out"]))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(bits(outs[0]), bits(outs[2]))


def test_two_calls_agree_bitwise_and_strided_inputs_work():
    D, T, lens = 64, 4, (129, 7, 1021)
    outs = []
    for layout in ("packed", "packed", "wide", "odd"):
        g = torch.Generator(device="cuda").manual_seed(9)
        qkv, k0, v0 = _inputs(D, "normal", lens, T, g)
        if layout == "wide":    # rows 8 elements further apart: the kernel takes the strides
            qkv = torch.cat([qkv, torch.zeros(B, T, 8, dtype=qkv.dtype, device="cuda")], 2)[:, :, :3 * H * D]
        elif layout == "odd":   # rows that do not start on 16 bytes: the op copies
            qkv = torch.cat([qkv, torch.zeros(B, T, 1, dtype=qkv.dtype, device="cuda")], 2)[:, :, :3 * H * D]
        assert qkv.is_contiguous() == (layout == "packed")
        _, k, v = guarded_caches(B, H, LMAX, D, "cuda", spare=SPARE)
        k.copy_(k0)
        v.copy_(v0)
        lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
        if layout == "wide":
            assert get_ext().attn_decode_block(qkv, k.clone(), v.clone(), lens_t, H) is not None
        elif layout == "odd":
            assert get_ext().attn_decode_block(qkv, k.clone(), v.clone(), lens_t, H) is None
        outs.append(attention_decode_block(qkv, k, v, lens_t, H))
    for o in outs[1:]:
        assert torch.equal(bits(o), bits(outs[0]))


def test_head_dim_32_and_fp32_take_the_torch_path_and_match():
    D, T, lens, counts = 32, 3, (0, 64, 1022), (3, 2, 3)
    g = torch.Generator(device="cuda").manual_seed(10)
    qkv, k0, v0 = _inputs(D, "normal", lens, T, g)
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    counts_t = torch.tensor(counts, dtype=torch.int32, device="cuda")
    c = block_counts(lens, counts, T, LMAX)
    for dtype in (torch.bfloat16, torch.float32):
        buf, k, v = guarded_caches(B, H, LMAX, D, "cuda", dtype, spare=SPARE)
        k.copy_(k0)
        v.copy_(v0)
        x = qkv.to(dtype)
        assert get_ext().attn_decode_block(x, k.clone(), v.clone(), lens_t, H, counts_t) is None
        want = ref64_block(x, k, v, lens, H, counts)
        e32 = (attention_decode_block_ref(x.float(), k.float(), v.float(), lens_t, H, counts=counts_t).double()
               - want).abs().max().item()
        before = buf.clone()
        out = attention_decode_block(x, k, v, lens_t, H, counts=counts_t)
        assert out.dtype == dtype and out.shape == (B, T, H * D)
        ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
        assert ((out.double() - want).abs() <= ulp * want.abs() + 4 * e32).all()
        new = x.view(B, T, 3, H, D)
        for b, m in enumerate(lens):
            for j in range(c[b]):
                before[0, b, :, SPARE + m + j], before[1, b, :, SPARE + m + j] = new[b, j, 1], new[b, j, 2]
            assert not out[b, c[b]:].any()
        assert torch.equal(bits(buf), bits(before))
    # fp32 at a head size the kernel has: still the PyTorch path
    _, k, v = guarded_caches(B, H, LMAX, 64, "cuda", torch.float32, spare=SPARE)
    assert get_ext().attn_decode_block(torch.zeros(B, T, 3 * H * 64, device="cuda"), k, v, lens_t, H) is None


def test_cpu_tensors_and_bad_block_lengths():
    D = 64
    ext = get_ext()
    k, v = torch.zeros(B, H, LMAX, D, dtype=torch.bfloat16), torch.zeros(B, H, LMAX, D, dtype=torch.bfloat16)
    lens = torch.zeros(B, dtype=torch.int32)
    assert ext.attn_decode_block(torch.zeros(B, 2, 3 * H * D, dtype=torch.bfloat16), k, v, lens, H) is None
    k, v, lens = k.cuda(), v.cuda(), lens.cuda()
    for T in (0, 9):
        x = torch.zeros(B, T, 3 * H * D, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(RuntimeError, match="T must be in 1 .. 8"):
            ext.attn_decode_block(x, k, v, lens, H)
        with pytest.raises(ValueError):
            attention_decode_block(x, k, v, lens, H)
    x = torch.zeros(B, 2, 3 * H * D, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="counts must be int32"):
        ext.attn_decode_block(x, k, v, lens, H, torch.zeros(B, dtype=torch.long, device="cuda"))
    with pytest.raises(RuntimeError, match="counts must be int32"):
        ext.attn_decode_block(x, k, v, lens, H, torch.zeros(B + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="do not agree"):
        ext.attn_decode_block(x[:, :, :-8], k, v, lens, H)
    assert not bits(k).any() and not bits(v).any()  # nothing ran
