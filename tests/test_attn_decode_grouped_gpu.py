"""csrc/attn_decode_grouped.hip (K-M28) through its binding against float64 on the same bf16 inputs.  Yardstick:
``attention_extend`` (the same bf16 weights) with T = 1 on a per-row copy of prefix plus suffix; a call's largest error
may be twice the yardstick's in the same call, and no bound is below one bf16 ulp of the reference's largest value.
B = 2 groups (4 at G = 1: two rows stay active beside the parked ones); NaN from ``plens`` / ``slens`` on."""
import math

import pytest
import torch

from decode_helpers import guarded_caches
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import attention_decode_grouped, attention_extend

pytestmark = pytest.mark.gpu
H, LP, LS, SPARE = 2, 160, 40, 3
PLENS = [0, 1, 31, 32, 33, 127, 128, 129, 160]  # both sides of a 32-key tile and of the 128 keys of a 4-wave round
SLENS = [0, 1, 31, 32, 33, 39]


def _inputs(D, G, kind, pl, seed, dtype=torch.bfloat16):
    """Unit normals, or a ``ramp`` of scores climbing by up to 65 to the new key (the maximum moves everywhere)."""
    B, dev, g = len(pl), "cuda", torch.Generator(device="cuda").manual_seed(seed)
    R = B * G
    sl = [SLENS[(5 * r + r // G) % 6] for r in range(R)]
    sl[1], sl[R - 2] = -1, LS
    grp = torch.arange(R, device=dev) // G
    q, d = torch.randn(R, H, D, device=dev, generator=g), torch.randn(B, H, D, device=dev, generator=g)
    kp, vp = (torch.randn(B, H, LP, D, device=dev, generator=g) for _ in range(2))
    ks, vs = (torch.randn(R, H, LS + 1, D, device=dev, generator=g) for _ in range(2))
    if kind == "ramp":
        plt = torch.tensor(pl, device=dev).float()
        tot = (plt + LS).view(B, 1)
        a_p = 65.0 * (torch.arange(LP, device=dev).view(1, LP) - tot) / tot
        a_s = 65.0 * (plt[grp].view(R, 1) + torch.arange(LS + 1, device=dev).view(1, -1) - tot[grp]) / tot[grp]
        along = d * math.sqrt(D) / (d ** 2).sum(-1, keepdim=True)
        q = d[grp] + 0.05 * q
        kp = 0.01 * kp + a_p.view(B, 1, LP, 1) * along.unsqueeze(2)
        ks = 0.01 * ks + a_s.view(R, 1, LS + 1, 1) * along[grp].unsqueeze(2)
    rows, at = torch.arange(R, device=dev), torch.tensor(sl, device=dev).clamp(0, LS)
    qkv = torch.stack([q, ks[rows, :, at], vs[rows, :, at]], 1).reshape(R, 3 * H * D).to(dtype)
    return dict(D=D, G=G, pl=pl, sl=sl, qkv=qkv, kp=kp.to(dtype), vp=vp.to(dtype), ks=ks[:, :, :LS].to(dtype),
                vs=vs[:, :, :LS].to(dtype))


def _call(inp, qs=0, b0=0):
    """The groups from b0 on through the binding, on guarded caches with NaN tails -> out; checks what may change."""
    D, G, dt = inp["D"], inp["G"], inp["qkv"].dtype
    b1 = len(inp["pl"])
    B, r0, r1 = b1 - b0, b0 * G, b1 * G
    pl, sl = inp["pl"][b0:b1], inp["sl"][r0:r1]
    pbuf, kp, vp = guarded_caches(B, H, LP, D, "cuda", dt, spare=SPARE)
    sbuf, ks, vs = guarded_caches(B * G, H, LS, D, "cuda", dt, spare=SPARE)
    kp.copy_(inp["kp"][b0:b1]), vp.copy_(inp["vp"][b0:b1]), ks.copy_(inp["ks"][r0:r1]), vs.copy_(inp["vs"][r0:r1])
    for c, ns in ((kp, pl), (vp, pl), (ks, sl), (vs, sl)):
        for i, n in enumerate(ns):
            c[i, :, max(n, 0):] = float("nan")
    plens, slens = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (pl, sl))
    before, qkv = (pbuf.clone(), sbuf.clone()), inp["qkv"][r0:r1]
    out = get_ext().attn_decode_grouped(qkv, kp, vp, plens, ks, vs, slens, H, G, qs)
    assert out is not None and plens.tolist() == pl and slens.tolist() == sl and torch.isfinite(out.float()).all()
    want = before[1].clone()
    new = qkv.view(B * G, 3, H, D)
    for r, n in enumerate(sl):  # exactly these rows change, to the bits of qkv_new
        if 0 <= n < LS:
            want[0, r, :, SPARE + n], want[1, r, :, SPARE + n] = new[r, 1], new[r, 2]
        else:
            assert not out[r].any()
    raw = torch.int16 if dt == torch.bfloat16 else torch.int32  # bits: the buffers hold NaNs
    assert torch.equal(pbuf.view(raw), before[0].view(raw)) and torch.equal(sbuf.view(raw), want.view(raw))
    return out


def ref64_grouped(qkv, kp, vp, pl, ks, vs, sl, H, G):
    """The definition in float64 -> (out [R, H D], {active row: its keys and values without the new one})."""
    R, D, new = len(sl), kp.shape[3], qkv.view(len(sl), 3, H, -1)
    want, held = torch.zeros(R, H, D, dtype=torch.float64, device=qkv.device), {}
    for r, n in enumerate(sl):
        b = r // G
        if 0 <= n < ks.shape[2] and 0 <= pl[b] <= kp.shape[2]:
            held[r] = K, V = [torch.cat([p[b, :, :pl[b]], s[r, :, :n]], 1) for p, s in ((kp, ks), (vp, vs))]
            Kn, Vn = torch.cat([K, new[r, 1][:, None]], 1).double(), torch.cat([V, new[r, 2][:, None]], 1).double()
            p = torch.softmax(torch.einsum("hd,hld->hl", new[r, 0].double(), Kn) / math.sqrt(D), -1)
            want[r] = torch.einsum("hl,hld->hd", p, Vn)
    return want.view(R, H * D), held


def _check(inp, out):
    D, G, pl, sl, qkv = inp["D"], inp["G"], inp["pl"], inp["sl"], inp["qkv"]
    R, lens = len(sl), [-1] * len(sl)
    want, held = ref64_grouped(qkv, inp["kp"], inp["vp"], pl, inp["ks"], inp["vs"], sl, H, G)
    kc, vc = (torch.zeros(R, H, LP + LS + 1, D, dtype=qkv.dtype, device="cuda") for _ in range(2))
    for r, (K, V) in held.items():
        lens[r] = K.shape[1]
        kc[r, :, :lens[r]], vc[r, :, :lens[r]] = K, V
    yard = attention_extend(qkv.view(R, 1, -1), kc, vc, torch.tensor(lens, dtype=torch.int32, device="cuda"), H)
    e, e_yard = (out.double() - want).abs().max().item(), (yard.view(R, -1).double() - want).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(want.abs().max().item())) - 7)
    print(f"D={D} G={G} plens={pl}: max |err| = {e:.4e}, attention_extend's = {e_yard:.4e}, ratio "
          f"{e / max(e_yard, 1e-30):.3f}, one bf16 ulp = {ulp:.4e}")
    assert e <= max(2 * e_yard, ulp), (e, e_yard, ulp)


@pytest.mark.parametrize("G", [1, 3, 8, 32])
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_against_float64_and_what_it_writes(D, G):
    B = 4 if G == 1 else 2
    for kind in ("normal", "ramp"):
        for i in range(0, len(PLENS), 2):
            inp = _inputs(D, G, kind, [PLENS[(i + b) % len(PLENS)] for b in range(B)], 1000 * D + 10 * G + i)
            _check(inp, _call(inp))


@pytest.mark.parametrize("D", [64, 128])
def test_bits_do_not_depend_on_the_call_the_slice_or_the_other_groups(D):
    inp = _inputs(D, 32, "ramp", [129, 33], D)
    out = _call(inp)
    for qs in (0, 4, 8, 32):
        assert torch.equal(_call(inp, qs=qs), out), qs
    assert torch.equal(_call(inp, b0=1), out[32:])  # group 1 alone


def test_what_is_served_declined_and_rejected():
    ext = get_ext()
    for D, G, dt in ((64, 33, torch.bfloat16), (32, 3, torch.bfloat16), (64, 3, torch.float32)):
        inp = _inputs(D, G, "normal", [129, 33], G, dt)
        pl, sl = (torch.tensor(inp[x], dtype=torch.int32, device="cuda") for x in ("pl", "sl"))
        a = [inp["qkv"], inp["kp"], inp["vp"], pl, inp["ks"].clone(), inp["vs"].clone(), sl, H, G]
        assert ext.attn_decode_grouped(*a) is None
        _check(inp, attention_decode_grouped(*a[:8], group=G))  # the PyTorch path, within the same bound
    for i, bad in ((3, pl.long()), (6, sl[:5]), (0, inp["qkv"][:, :-8]), (8, 4), (8, 0), (7, H + 1)):
        with pytest.raises(RuntimeError):
            ext.attn_decode_grouped(*(a[:i] + [bad] + a[i + 1:]))
