"""csrc/linear_rows.hip (K-M26) through its binding, which must not decline, and ``decode_linears="rows"`` on the
tiny GPT-2 models.  Allowed error per element (``test_attn_decode_gpu.py``): ``2^-8 |y_ref| + 4 e32``, e32 the error
of fp32 ``F.linear`` (+ act) on the same inputs.  Measured on an MI355X: worst error over bound 0.995, e32 <= 2.8e-06."""
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
SHAPES = ([(M, N, 256) for M in (1, 5, 32, 33, 64, 65, 128) for N in (1, 31, 32, 33, 100, 3000)]
          + [(33, 100, K) for K in (64, 768, 1024, 3072)] + [(3, 50257, 768)])


def _inputs(M, N, K, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
    return x, w, torch.randn(N, device="cuda", generator=g).bfloat16()


def _worst(got, x, w, b, act):
    ref = lambda dt: ACTS[act][1](F.linear(x.to(dt), w.to(dt), None if b is None else b.to(dt)))  # noqa: E731
    want = ref(torch.float64)
    e32 = (ref(torch.float32).double() - want).abs().max().item()
    return ((got.double() - want).abs() / (2.0 ** -8 * want.abs() + 4 * e32)).max().item(), e32


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_matches_float64(M, N, K):
    x, w, b = _inputs(M, N, K)
    for act in ACTS:
        for bias in (None, b):
            got = get_ext().linear_rows(x, w, bias, ACTS[act][0])
            assert got is not None and got.shape == (M, N) and got.dtype == torch.bfloat16
            worst, e32 = _worst(got, x, w, bias, act)
            print(f"linear_rows {M}x{N}x{K} act={act} bias={bias is not None}: e32={e32:.3e} worst err/tol={worst:.3f}")
            assert worst <= 1.0, (worst, e32)


@pytest.mark.parametrize("M,N,K", [(5, 33, 256), (65, 100, 192), (128, 31, 64)])
def test_memory_discipline(M, N, K):
    """x and y inside pattern-filled buffers at odd multiples of 8 elements per row, W a slice of a matrix of NaN."""
    x, w, b = _inputs(M, N, K, seed=1)
    xbuf = torch.full((M + 2, K + 24), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    ybuf = torch.full((M + 2, ((N + 7) // 8 * 8 + 8) | 8), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    wbuf = torch.full((N + 4, K + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    xv, wv, yv = xbuf[1:M + 1, 8:K + 8], wbuf[2:N + 2, :K], ybuf[1:M + 1, 3:N + 3]
    xv.copy_(x), wv.copy_(w)
    assert xv.stride(0) % 16 == 8 and yv.stride(0) % 16 == 8 and wv.stride(0) > K
    got = get_ext().linear_rows(xv, wv, b, 1, yv)
    assert got is not None and got.data_ptr() == yv.data_ptr() and not torch.isnan(yv).any()
    assert torch.equal(bits(yv), bits(get_ext().linear_rows(x, w, b, 1))) and _worst(yv, x, w, b, "gelu")[0] <= 1.0
    outside = torch.ones_like(ybuf, dtype=torch.bool)
    outside[1:M + 1, 3:N + 3] = False
    assert (bits(ybuf)[outside] == PATTERN).all()


def test_row_contract():
    """An output row is a function of its input row alone, across the three instantiations and from call to call."""
    run = functools.partial(get_ext().linear_rows, act=1)
    x, w, b = _inputs(128, 100, 768, seed=2)
    full, twelve, one = run(x, w, b), run(x[:12], w, b), run(x[7:8], w, b)
    assert torch.equal(bits(full), bits(run(x, w, b)))
    assert torch.equal(bits(twelve[5:9]), bits(run(x[5:9], w, b))) and torch.equal(bits(twelve), bits(full[:12]))
    for M in (33, 128):
        other = torch.cat([torch.randn(M - 1, 768, device="cuda").bfloat16(), x[7:8]])  # the row last, new company
        assert torch.equal(bits(run(other, w, b)[M - 1:]), bits(one))


def test_declined_cases_take_the_pytorch_path():
    ext = get_ext()
    for M, K, dtype in ((129, 256, torch.bfloat16), (4, 96, torch.bfloat16), (4, 256, torch.float32)):
        x, w, b = (t.to(dtype) for t in _inputs(M, 40, K, seed=3))
        assert ext.linear_rows(x, w, b, 1) is None
        got = linear_rows(x, w, b, act="gelu")
        assert got.dtype == dtype and _worst(got, x, w, b, "gelu")[0] <= 1.0
    x, w, b = _inputs(4, 40, 256)
    for bad in (lambda: ext.linear_rows(x, w[:, :128], b, 0), lambda: ext.linear_rows(x, w, b[:39], 0),
                lambda: ext.linear_rows(x, w.float(), b, 0), lambda: ext.linear_rows(x, w, b, 7)):
        with pytest.raises(RuntimeError):
            bad()


class _Rows:
    def __init__(self, model):
        self.init_cache, self.cfg = model.init_cache, model.cfg
        for name in ("prefill", "decode_step", "decode_block"):
            setattr(self, name, functools.partial(getattr(model, name), decode_linears="rows"))


@pytest.mark.parametrize("heads", [4, 2])
def test_teacher_forced_rows_logits_match_the_fp32_forward(heads):
    """The bound of ``test_generate_gpu.py``: twice the native full forward's own error over the same positions."""
    ref, nat, _ = _models(heads)
    ids = torch.randint(1000, 3000, (4, 96), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with torch.no_grad():
        want, full = ref(ids).float(), nat(ids).float()
    got, _ = teacher_forced(_Rows(nat), ids, [1, 5, 64, 65], 65)
    e_rows = max((got[(b, p)] - want[b, p]).abs().max().item() for (b, p) in got)
    e_full = max((full[b, p] - want[b, p]).abs().max().item() for (b, p) in got)
    print(f"heads={heads}: rows path max |err| = {e_rows:.4e}, native full forward max |err| = {e_full:.4e}")
    assert e_rows <= 2 * e_full, (e_rows, e_full)


@pytest.mark.parametrize("heads,kv", [(4, "bf16"), (2, "bf16"), (4, "fp8")])
def test_greedy_generate_rows_equals_the_written_out_loop(heads, kv):
    nat, rows = _models(heads)[1], _Rows(_models(heads)[1])
    ids, lens = bsh.prompts("cuda", TINY["vocab_size"])
    a, na = nat.generate(ids, lens, 24, temperature=0, decode_linears="rows", kv_dtype=kv)
    b, nb = nat.generate(ids, lens, 24, temperature=0, decode_linears="rows", kv_dtype=kv)
    assert torch.equal(a, b) and torch.equal(na, nb) and na.tolist() == [24] * 3
    cache = nat.init_cache(3, 64, kv_dtype=kv)
    toks = [lms.greedy(rows.prefill(ids, lens, cache))]
    for _ in range(23):
        toks.append(lms.greedy(rows.decode_step(toks[-1], cache)))
    assert torch.equal(a, torch.stack(toks, 1))


def test_beam_search_and_lookahead_rows_equal_their_written_out_loops():
    """Against the helpers' loops, their ``prefill``, ``decode_step`` and ``decode_block`` in the same mode."""
    nat = _models(4)[1]
    ids, lens = bsh.prompts("cuda", TINY["vocab_size"])
    want = bsh.reordering_beam_search(_Rows(nat), ids, lens, 12, 2)
    for a, b in zip(nat.beam_search(ids, lens, 12, num_beams=2, decode_linears="rows"), want):
        assert torch.equal(a, b), (a, b)
    toks, new_lens, stats = nat.generate_lookahead(ids, lens, 24, lookahead=3, ngram=1, return_stats=True,
                                                   decode_linears="rows")
    t2, l2, s2, _ = lookahead_loop(_Rows(nat), ids, lens, 24, 3, ngram=1)
    assert torch.equal(toks, t2) and new_lens.tolist() == l2 == [24] * 3 and stats == s2
