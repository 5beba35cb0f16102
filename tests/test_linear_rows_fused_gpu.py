"""csrc/linear_rows_fused.hip (K-M30) through ``get_ext().linear_rows``, which must not decline, and ``"rows_fused"``
on the tiny GPT-2.  Bounds: prologue half a bf16 ulp + 4 e32, whole op one bf16 ulp + 4 e32 (measured on an MI355X:
worst 1.000 and 0.500; fp32 ``F.layer_norm`` misses a constant row at eps 1e-12, so those are also held to beta)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import beam_search_helpers as bsh
from decode_block_helpers import lookahead_loop
from decode_helpers import PATTERN, TINY, bits, teacher_forced
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import linear_rows
from test_generate_gpu import _models  # (fp32 model, bf16 model with shadows, engine) of the tiny GPT-2
from utils import lm_sampling as lms

pytestmark = pytest.mark.gpu
ACTS = {"none": (0, lambda t: t), "gelu": (1, F.gelu)}


def _inputs(M, N, K, seed=0):
    """x with rows m % 4 == 0: mean 50, std 1 (a one-pass variance fails); 1: unit normal; 2: constant; 3: scaled 2^-20."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x, m = rnd(M, K), torch.arange(M, device="cuda").view(M, 1) % 4
    x = torch.where(m == 0, x + 50, torch.where(m == 2, x[:, :1].expand(M, K), torch.where(m == 3, x * 2.0 ** -20, x)))
    w = (rnd(N, K) * K ** -0.5).bfloat16()
    return x.bfloat16(), w, rnd(N).bfloat16(), (1 + 0.5 * rnd(K)).bfloat16(), rnd(K).bfloat16(), rnd(M, N).bfloat16()


def _ulp(v):  # one bf16 ulp of |v| (0 at 0)
    return torch.where(v == 0, 0.0, torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - 8))


def _a(x, gm, bt, eps):  # the kernel's a: W = identity, no bias, no act, no residual
    return get_ext().linear_rows(x, torch.eye(x.shape[1], device="cuda").bfloat16(), ln_gamma=gm, ln_beta=bt, ln_eps=eps)


def _worst(got, a, w, b, act, res):
    ref = lambda dt: (ACTS[act][1](F.linear(a.to(dt), w.to(dt), None if b is None else b.to(dt)))  # noqa: E731
                      + (0 if res is None else res.to(dt)))
    want = ref(torch.float64)
    e32 = (ref(torch.float32).double() - want).abs().max().item()
    return ((got.double() - want).abs() / (_ulp(want) + 4 * e32)).max().item()


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("K", [64, 320, 768, 3072])
@pytest.mark.parametrize("M", [1, 33, 128])
def test_prologue_matches_float64_layernorm(M, K, eps):
    x, _, _, gm, bt, _ = _inputs(M, 1, K)
    sel = torch.randperm(K, device="cuda")
    w = F.one_hot(sel, K).bfloat16()
    got = get_ext().linear_rows(x, w, ln_gamma=gm, ln_beta=bt, ln_eps=eps)
    assert got is not None and got.shape == (M, K)
    ln = lambda dt: F.layer_norm(x.to(dt), (K,), gm.to(dt), bt.to(dt), eps)  # noqa: E731
    want = ln(torch.float64)
    e32 = (ln(torch.float32).double() - want).abs().max().item()
    worst = ((got.double() - want[:, sel]).abs() / (_ulp(want[:, sel]) / 2 + 4 * e32)).max().item()
    print(f"prologue {M}x{K} eps={eps}: e32={e32:.3e} worst err/tol={worst:.3f}")
    assert worst <= 1.0, (worst, e32)
    assert M < 3 or torch.equal(bits(got[2]), bits(bt[sel]))  # a constant row: d == 0 exactly, a == beta
    assert torch.equal(bits(get_ext().linear_rows(x, w[:40], ln_gamma=gm, ln_beta=bt, ln_eps=eps)), bits(got[:, :40]))


@pytest.mark.parametrize("M,N,K", [(M, N, 256) for M in (1, 32, 33, 65, 128) for N in (1, 31, 33, 100)]
                         + [(33, 100, K) for K in (64, 768, 3072)])
def test_whole_op_matches_float64(M, N, K):
    x, w, b, gm, bt, res = _inputs(M, N, K, seed=1)
    a = _a(x, gm, bt, 1e-5)
    for ln, r in ((True, None), (False, res), (True, res)):
        for act, bias in (("none", None), ("gelu", b), ("none", b)):
            kw = dict(ln_gamma=gm, ln_beta=bt, ln_eps=1e-5) if ln else {}
            got = get_ext().linear_rows(x, w, bias, ACTS[act][0], residual=r, **kw)
            assert got is not None and got.shape == (M, N) and got.dtype == torch.bfloat16
            worst = _worst(got, a if ln else x, w, bias, act, r)
            print(f"fused {M}x{N}x{K} ln={ln} res={r is not None} act={act} bias={bias is not None}: err/tol={worst:.3f}")
            assert worst <= 1.0, worst


@pytest.mark.parametrize("M,N,K", [(5, 33, 256), (65, 100, 192), (128, 31, 64)])
def test_memory_discipline(M, N, K):
    x, w, b, gm, bt, res = _inputs(M, N, K, seed=2)
    wide = ((N + 7) // 8 * 8 + 8) | 8
    xbuf, rbuf, ybuf = (torch.full((M + 2, c), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
                        for c in (K + 24, wide, wide))
    xbuf[M + 1:], rbuf[M + 1:] = float("nan"), float("nan")
    wbuf = torch.full((N + 4, K + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    xv, wv, rv, yv = xbuf[1:M + 1, 8:K + 8], wbuf[2:N + 2, :K], rbuf[1:M + 1, 5:N + 5], ybuf[1:M + 1, 3:N + 3]
    xv.copy_(x), wv.copy_(w), rv.copy_(res)
    assert xv.stride(0) % 16 == 8 and yv.stride(0) % 16 == 8 and rv.stride(0) % 16 == 8 and wv.stride(0) > K
    got = get_ext().linear_rows(xv, wv, b, 1, yv, gm, bt, 1e-5, rv)
    assert got is not None and got.data_ptr() == yv.data_ptr() and not torch.isnan(yv).any()
    assert torch.equal(bits(yv), bits(get_ext().linear_rows(x, w, b, 1, None, gm, bt, 1e-5, res)))
    assert _worst(yv, _a(x, gm, bt, 1e-5), w, b, "gelu", res) <= 1.0
    outside = torch.ones_like(ybuf, dtype=torch.bool)
    outside[1:M + 1, 3:N + 3] = False
    assert (bits(ybuf)[outside] == PATTERN).all()


def test_row_contract():
    x, w, b, gm, bt, res = _inputs(128, 100, 768, seed=3)
    run = lambda t, r: get_ext().linear_rows(t, w, b, 1, None, gm, bt, 1e-5, r)  # noqa: E731
    full, twelve, one = run(x, res), run(x[:12], res[:12]), run(x[7:8], res[7:8])
    assert torch.equal(bits(full), bits(run(x, res))) and torch.equal(bits(twelve), bits(full[:12]))
    assert torch.equal(bits(twelve[5:9]), bits(run(x[5:9], res[5:9])))
    for M in (33, 128):
        rows = torch.cat([torch.randn(M - 1, 768, device="cuda").bfloat16(), x[7:8]])  # the row last, new company
        assert torch.equal(bits(run(rows, torch.cat([res[:M - 1], res[7:8]]))[M - 1:]), bits(one))
    plain = get_ext().linear_rows(x, w, b, 1)
    assert torch.equal(bits(linear_rows(x, w, b, act="gelu", ln=None, residual=None)), bits(plain))
    assert torch.equal(bits(get_ext().linear_rows(x, w, b, 1, ln_gamma=None, ln_beta=None, residual=None)), bits(plain))


def test_declines_and_rejects():
    ext = get_ext()
    for M, K, dtype in ((129, 256, torch.bfloat16), (4, 96, torch.bfloat16), (4, 256, torch.float32)):
        x, w, b, gm, bt, res = (t.to(dtype) for t in _inputs(M, 40, K, seed=4))
        assert ext.linear_rows(x, w, b, 1, None, gm, bt, 1e-5, res) is None
        got = linear_rows(x, w, b, act="gelu", ln=(gm, bt, 1e-5), residual=res)
        a = linear_rows(x, torch.eye(K, device="cuda", dtype=dtype), ln=(gm, bt, 1e-5))  # the serving path's own a
        assert got.dtype == dtype and _worst(got, a, w, b, "gelu", res) <= 1.0
    x, w, b, gm, bt, res = _inputs(4, 40, 256)
    out = torch.empty(8, 40, device="cuda", dtype=torch.bfloat16)
    for bad in (lambda: ext.linear_rows(x, w, b, 0, None, gm[:255], bt, 1e-5), lambda: ext.linear_rows(x, w, residual=res[:3]),
                lambda: ext.linear_rows(x, w, residual=res[:, :39]), lambda: ext.linear_rows(x, w, residual=res.float()),
                lambda: ext.linear_rows(x, w, b, 0, out[:4], residual=out[2:6])):
        with pytest.raises(RuntimeError):
            bad()


class _Fused:
    def __init__(self, model):
        self.init_cache, self.cfg = model.init_cache, model.cfg
        for name in ("prefill", "decode_step", "decode_block"):
            setattr(self, name, functools.partial(getattr(model, name), decode_linears="rows_fused"))


@pytest.mark.parametrize("heads", [4, 2])
def test_teacher_forced_rows_fused_logits_match_the_fp32_forward(heads):
    ref, nat, _ = _models(heads)
    ids = torch.randint(1000, 3000, (4, 96), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with torch.no_grad():
        want, full = ref(ids).float(), nat(ids).float()
    got, _ = teacher_forced(_Fused(nat), ids, [1, 5, 64, 65], 65)
    e_rows = max((got[(b, p)] - want[b, p]).abs().max().item() for (b, p) in got)
    e_full = max((full[b, p] - want[b, p]).abs().max().item() for (b, p) in got)
    print(f"heads={heads}: rows_fused path max |err| = {e_rows:.4e}, native full forward max |err| = {e_full:.4e}")
    assert e_rows <= 2 * e_full, (e_rows, e_full)


@pytest.mark.parametrize("heads", [4, 2])
def test_generation_in_the_mode_equals_the_written_out_loops(heads):
    nat, rows = _models(heads)[1], _Fused(_models(heads)[1])
    ids, lens = bsh.prompts("cuda", TINY["vocab_size"])
    a, na = nat.generate(ids, lens, 24, temperature=0, decode_linears="rows_fused")
    b, nb = nat.generate(ids, lens, 24, temperature=0, decode_linears="rows_fused")
    assert torch.equal(a, b) and torch.equal(na, nb) and na.tolist() == [24] * 3
    cache = nat.init_cache(3, 64)
    toks = [lms.greedy(rows.prefill(ids, lens, cache))]
    for _ in range(23):
        toks.append(lms.greedy(rows.decode_step(toks[-1], cache)))
    assert torch.equal(a, torch.stack(toks, 1))
    if heads == 4:
        want = bsh.reordering_beam_search(rows, ids, lens, 12, 2)
        for a, b in zip(nat.beam_search(ids, lens, 12, num_beams=2, decode_linears="rows_fused"), want):
            assert torch.equal(a, b), (a, b)
        toks, new_lens, stats = nat.generate_lookahead(ids, lens, 24, lookahead=3, ngram=1, return_stats=True,
                                                       decode_linears="rows_fused")
        t2, l2, s2, _ = lookahead_loop(rows, ids, lens, 24, 3, ngram=1)
        assert torch.equal(toks, t2) and new_lens.tolist() == l2 == [24] * 3 and stats == s2
