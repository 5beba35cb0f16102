"""csrc/attn_decode.hip through a cache indirection table (``ext.attn_decode_beam``): rows in groups
of W slots, cached key t of row r read from cache row ``(r // W) W + min(src[r, t], W - 1)``.

Numbers: against ``ref64`` on the gathered caches with the rule of ``test_attn_decode_gpu.py`` -
``2^-8 |o_ref| + 4 e32`` per element, ``e32`` the largest error of the fp32 PyTorch path against
float64 on the same inputs, so the fp32 path sets the slack and never the kernel.

Every call has two groups; ``lens`` come from ``RAGGED_LENS``, equal within a group's active rows,
and for W > 1 one row of each group is parked (at W = 1 a parked row would leave its group empty;
``test_inactive_rows_and_argument_checks`` parks a W = 1 group).  Caches are views into a
pattern-filled buffer, so a stray store changes the pattern instead of faulting."""
import functools

import pytest
import torch

from decode_helpers import RAGGED_LENS, bits, guarded_caches, ref64
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import attention_decode, attention_decode_ref

pytestmark = pytest.mark.gpu

H, LMAX, SPARE = 2, 1024, 3


def _table(kind, W, g):
    R = 2 * W
    if kind == "zero":        # every beam reads slot 0: the shared prompt
        return torch.zeros(R, LMAX, dtype=torch.uint8, device="cuda")
    if kind == "identity":
        return (torch.arange(R, device="cuda") % W).to(torch.uint8).view(R, 1).expand(R, LMAX).contiguous()
    src = torch.randint(0, W, (R, LMAX), device="cuda", generator=g)
    if kind == "high":        # half of the bytes at or above W: they must read slot W - 1
        high = torch.randint(W, 256, (R, LMAX), device="cuda", generator=g)
        src = torch.where(torch.rand(R, LMAX, device="cuda", generator=g) < 0.5, high, src)
    return src.to(torch.uint8)


def _gathered(c, src, W):
    """The cache every row effectively sees: [R, H, Lmax, D]."""
    R = c.shape[0]
    rows = torch.arange(R, device=c.device)
    from_row = (rows // W * W).view(R, 1) + src.long().clamp(max=W - 1)
    return c[from_row, :, torch.arange(LMAX, device=c.device).view(1, LMAX)].permute(0, 2, 1, 3).contiguous()


def _lens(W, pair):
    """Two groups with the common lengths ``pair``; for W > 1 slot 0 of group 0 and slot W - 1 of group
    1 are parked."""
    lens = [pair[0]] * W + [pair[1]] * W
    if W > 1:
        lens[0], lens[2 * W - 1] = -1, LMAX
    return lens


def _run(D, W, kind, pair, g, tail=None, lens=None):
    R = 2 * W
    lens = _lens(W, pair) if lens is None else lens
    qkv = torch.randn(R, 3 * H * D, device="cuda", generator=g).bfloat16()
    buf, k, v = guarded_caches(R, H, LMAX, D, "cuda", spare=SPARE)
    k.copy_(torch.randn(R, H, LMAX, D, device="cuda", generator=g))
    v.copy_(torch.randn(R, H, LMAX, D, device="cuda", generator=g))
    src = _table(kind, W, g)
    if tail is not None:  # the bits at and beyond each group's common length, in every slot of the group
        for grp, n in enumerate(pair):
            k.view(torch.int16)[grp * W:(grp + 1) * W, :, n:] = tail
            v.view(torch.int16)[grp * W:(grp + 1) * W, :, n:] = tail
            src[grp * W:(grp + 1) * W, n:] = tail & 0xFF
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ke, ve = _gathered(k, src, W), _gathered(v, src, W)
    want = ref64(qkv, ke, ve, lens_t, H)
    e32 = (attention_decode_ref(qkv.float(), ke.float(), ve.float(), lens_t, H).double() - want).abs().max().item()
    before, src0 = buf.clone(), src.clone()
    out = get_ext().attn_decode_beam(qkv, k, v, lens_t, H, src, W)
    assert out is not None, "the kernel must take bf16 D in {64, 128}"
    torch.cuda.synchronize()
    return dict(qkv=qkv, lens=lens, lens_t=lens_t, out=out, want=want, e32=e32, before=before, after=buf, k=k, v=v,
                src=src, src0=src0)


@functools.lru_cache(maxsize=4)  # a run holds its buffers: keep the last few (D, W, kind) only
def _ragged(D, W, kind):
    g = torch.Generator(device="cuda").manual_seed(1000 * D + 10 * W + len(kind))
    return [_run(D, W, kind, RAGGED_LENS[i:i + 2], g) for i in range(0, len(RAGGED_LENS), 2)]


@pytest.mark.parametrize("kind", ["random", "zero", "high"])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_matches_float64_on_the_gathered_caches(D, W, kind):
    runs = _ragged(D, W, kind)
    e32 = max(r["e32"] for r in runs)
    worst = 0.0
    for r in runs:
        err = (r["out"].double() - r["want"]).abs()
        tol = 2.0 ** -8 * r["want"].abs() + 4 * e32
        worst = max(worst, (err / tol).max().item())
        if kind == "high":
            assert (r["src"] >= W).any()
    print(f"attn_decode_beam D={D} W={W} {kind}: e32={e32:.3e} worst err/tol={worst:.3f}")
    assert worst <= 1.0, (worst, e32)


@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_append_goes_to_the_rows_own_slot_and_nothing_else_changes(D, W):
    for r in _ragged(D, W, "random"):
        R = 2 * W
        new = r["qkv"].view(R, 3, H, D)
        expect = r["before"].clone()
        for b, m in enumerate(r["lens"]):
            if 0 <= m < LMAX:
                assert torch.equal(bits(r["k"][b, :, m]), bits(new[b, 1]))
                assert torch.equal(bits(r["v"][b, :, m]), bits(new[b, 2]))
                expect[0, b, :, SPARE + m], expect[1, b, :, SPARE + m] = new[b, 1], new[b, 2]
            else:
                assert not bits(r["out"][b]).any()  # a parked row: zeros, bit for bit
        assert torch.equal(bits(r["after"]), bits(expect))
        assert torch.equal(r["src"], r["src0"])  # the table is the caller's
        assert r["lens_t"].tolist() == list(r["lens"])


@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_identity_table_is_the_plain_kernel_bit_for_bit(D, W):
    ext = get_ext()
    for r in _ragged(D, W, "identity"):
        _, k, v = guarded_caches(2 * W, H, LMAX, D, "cuda", spare=SPARE)
        k.copy_(r["before"][0, :, :, SPARE:SPARE + LMAX])
        v.copy_(r["before"][1, :, :, SPARE:SPARE + LMAX])
        plain = ext.attn_decode(r["qkv"], k, v, r["lens_t"], H)
        assert torch.equal(bits(plain), bits(r["out"]))
        assert torch.equal(bits(k), bits(r["k"])) and torch.equal(bits(v), bits(r["v"]))


@pytest.mark.parametrize("D", [64, 128])
def test_nothing_at_or_beyond_lens_is_read(D):
    W, pair = 3, (33, 1000)
    outs = []
    for tail in (0, 0x7FC0, -1):  # zeros, a quiet NaN, all ones (a NaN too); the table bytes 0, 0xC0, 0xFF
        g = torch.Generator(device="cuda").manual_seed(7)
        outs.append(_run(D, W, "random", pair, g, tail=tail)["out"])
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(bits(outs[0]), bits(outs[2]))


def test_two_calls_agree_bitwise():
    for D, W in ((64, 8), (128, 3)):
        outs = []
        for _ in range(2):
            g = torch.Generator(device="cuda").manual_seed(9)
            outs.append(_run(D, W, "random", (129, 1023), g)["out"])
        assert torch.equal(bits(outs[0]), bits(outs[1]))


def test_inactive_rows_and_argument_checks():
    ext = get_ext()
    D = 64
    # W = 1: group 0 parked, group 1 active
    g = torch.Generator(device="cuda").manual_seed(11)
    r = _run(D, 1, "zero", (0, 0), g, lens=[-1, 300])
    assert not bits(r["out"][0]).any()
    assert ((r["out"][1].double() - r["want"][1]).abs() <= 2.0 ** -8 * r["want"][1].abs() + 4 * r["e32"]).all()
    expect = r["before"].clone()
    new = r["qkv"].view(2, 3, H, D)
    expect[0, 1, :, SPARE + 300], expect[1, 1, :, SPARE + 300] = new[1, 1], new[1, 2]
    assert torch.equal(bits(r["after"]), bits(expect))

    W, R = 3, 6
    qkv = torch.randn(R, 3 * H * D, device="cuda").bfloat16()
    _, k, v = guarded_caches(R, H, LMAX, D, "cuda", spare=SPARE)
    lens = torch.full((R,), 5, dtype=torch.int32, device="cuda")
    src = torch.zeros(R, LMAX, dtype=torch.uint8, device="cuda")
    assert ext.attn_decode_beam(qkv, k, v, lens, H, src, W) is not None
    for bad in (src.int(), src[:, :-1], src[:-1], src.view(-1)):
        with pytest.raises(RuntimeError):
            ext.attn_decode_beam(qkv, k, v, lens, H, bad, W)
        with pytest.raises(ValueError):
            attention_decode(qkv, k, v, lens, H, src=bad, beams=W)
    for beams in (4, 0, 256):  # R % W != 0, and W outside 1 .. 255
        with pytest.raises(RuntimeError):
            ext.attn_decode_beam(qkv, k, v, lens, H, src, beams)
        with pytest.raises(ValueError):
            attention_decode(qkv, k, v, lens, H, src=src, beams=beams)
    # what the plain binding does not cover is not covered here either
    assert ext.attn_decode_beam(qkv.float(), k.float(), v.float(), lens, H, src, W) is None
    assert ext.attn_decode_beam(*[t.cpu() for t in (qkv, k, v, lens)], H, src.cpu(), W) is None


def test_head_dim_32_takes_the_torch_path_and_matches():
    D, W, R = 32, 3, 6
    g = torch.Generator(device="cuda").manual_seed(10)
    lens = [64, -1, 64, 500, 500, 500]
    qkv = torch.randn(R, 3 * H * D, device="cuda", generator=g).bfloat16()
    buf, k, v = guarded_caches(R, H, LMAX, D, "cuda", spare=SPARE)
    k.copy_(torch.randn(R, H, LMAX, D, device="cuda", generator=g))
    v.copy_(torch.randn(R, H, LMAX, D, device="cuda", generator=g))
    src = _table("high", W, g)
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    assert get_ext().attn_decode_beam(qkv, k.clone(), v.clone(), lens_t, H, src, W) is None
    ke, ve = _gathered(k, src, W), _gathered(v, src, W)
    want = ref64(qkv, ke, ve, lens_t, H)
    e32 = (attention_decode_ref(qkv.float(), ke.float(), ve.float(), lens_t, H).double() - want).abs().max().item()
    before = buf.clone()
    out = attention_decode(qkv, k, v, lens_t, H, src=src, beams=W)
    assert out.dtype == torch.bfloat16
    assert ((out.double() - want).abs() <= 2.0 ** -8 * want.abs() + 4 * e32).all()
    new = qkv.view(R, 3, H, D)
    for b, m in enumerate(lens):
        if 0 <= m < LMAX:
            before[0, b, :, SPARE + m], before[1, b, :, SPARE + m] = new[b, 1], new[b, 2]
    assert torch.equal(bits(buf), bits(before))
