"""csrc/linear_rows_fp8.hip (K-M29) through its binding, which must not decline, and ``decode_linears="rows_fp8"`` on
the tiny GPT-2 models.  Reference: float64 ``F.linear`` (+ act) on ``kv_dequantize(codes, exp)``.  Allowed error per
element: ``2^-8 |y_ref| + 4 e32[n]``, e32[n] the largest error over m of the fp32 computation on the same dequantized
inputs in output column n, so a weight row at a small scale is held to its own scale.

K: 64 and 256 leave lane halves and waves of the only chunk (512 k, 128 per wave, 64 per lane half) without codes;
576 is the K whose last chunk leaves waves 1 .. 3 without a piece (and wave 0 with one lane half); 2048 is the K with
more chunks (4) than the register ring has sets (3); 3072 runs the ring round twice.  Measured on an MI355X: worst
error over bound 0.996 (the head, gelu)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import beam_search_helpers as bsh
from decode_helpers import PATTERN, TINY, bits, teacher_forced
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import kv_dequantize, kv_quantize_ref, linear_rows_fp8
from distributed_pipeline_amd.parallel.ddp import DDPEngine
from test_generate_gpu import _models  # (fp32 model, bf16 model with shadows, engine) of the tiny GPT-2
from utils import lm_sampling as lms

pytestmark = pytest.mark.gpu

ACTS = {"none": (0, lambda t: t), "gelu": (1, F.gelu)}
SHAPES = ([(M, N, K) for M in (1, 32, 33, 65, 128) for N in (1, 31, 33, 100) for K in (64, 256, 576, 2048)]
          + [(33, 100, 3072), (3, 50257, 768)])


def _inputs(M, N, K, seed=0):
    """x, codes, exponents, bias on the GPU; from N = 31 on with the planted weight rows, each checked on its codes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = torch.randn(N, K, generator=g) * K ** -0.5
    if N >= 31:
        w[0] = 0.0
        w[5, 3] = 2.0 ** 10 * w[5].abs().max()  # the rest of row 5 lands on small, subnormal and zero codes
        w[N - 1] *= 2.0 ** -100
        w[N - 2] *= 2.0 ** 60
    codes, exp = kv_quantize_ref(w)
    if N >= 31:
        assert not codes[0].any() and exp[0] == 0
        rest = codes[5].clone()
        rest[3] = 0
        assert (codes[5, 3] & 0x7F) > 0x70 and ((rest & 0x7F) < 0x30).all()  # the outlier in (224, 448], the rest below 0.5
        assert (((rest & 0x78) == 0) & ((rest & 0x07) != 0)).any()  # subnormal codes among them
        assert exp[N - 1] < -100 and exp[N - 2] > 45
    return x.cuda(), codes.cuda(), exp.cuda(), torch.randn(N, generator=g).bfloat16().cuda()


def _worst(got, x, codes, exp, b, act):
    w = kv_dequantize(codes, exp)
    ref = lambda dt: ACTS[act][1](F.linear(x.to(dt), w.to(dt), None if b is None else b.to(dt)))  # noqa: E731
    want = ref(torch.float64)
    e32 = (ref(torch.float32).double() - want).abs().amax(0, keepdim=True)  # per output column
    err, tol = (got.double() - want).abs(), 2.0 ** -8 * want.abs() + 4 * e32
    # an exact zero (the all-zero weight row without bias) has tol = 0 and must be met exactly; a NaN stays one
    return torch.where(tol > 0, err / tol, torch.where(err == 0, 0.0, float("inf"))).max().item()


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_matches_float64(M, N, K):
    x, codes, exp, b = _inputs(M, N, K)
    for act in ACTS:
        for bias in (None, b):
            got = get_ext().linear_rows_fp8(x, codes, exp, bias, ACTS[act][0])
            assert got is not None and got.shape == (M, N) and got.dtype == torch.bfloat16
            worst = _worst(got, x, codes, exp, bias, act)
            print(f"linear_rows_fp8 {M}x{N}x{K} act={act} bias={bias is not None}: worst err/tol={worst:.3f}")
            assert worst <= 1.0, worst


@pytest.mark.parametrize("M,N,K", [(5, 33, 256), (65, 100, 576), (128, 31, 64)])
def test_memory_discipline(M, N, K):
    """x and y inside pattern-filled buffers at odd multiples of 8 elements per row, the codes a row slice of a matrix of
    the NaN code with a row stride above K, the exponents a slice of a buffer of 127."""
    x, codes, exp, b = _inputs(M, N, K, seed=1)
    xbuf = torch.full((M + 2, K + 24), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    ybuf = torch.full((M + 2, ((N + 7) // 8 * 8 + 8) | 8), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    cbuf = torch.full((N + 4, K + 16), 0x7F, dtype=torch.uint8, device="cuda")
    ebuf = torch.full((N + 4,), 127, dtype=torch.int8, device="cuda")
    xv, cv, ev, yv = xbuf[1:M + 1, 8:K + 8], cbuf[2:N + 2, :K], ebuf[2:N + 2], ybuf[1:M + 1, 3:N + 3]
    xv.copy_(x), cv.copy_(codes), ev.copy_(exp)
    assert xv.stride(0) % 16 == 8 and yv.stride(0) % 16 == 8 and cv.stride(0) > K
    got = get_ext().linear_rows_fp8(xv, cv, ev, b, 1, yv)
    assert got is not None and got.data_ptr() == yv.data_ptr() and not torch.isnan(yv).any()
    assert torch.equal(bits(yv), bits(get_ext().linear_rows_fp8(x, codes, exp, b, 1)))
    assert _worst(yv, x, codes, exp, b, "gelu") <= 1.0
    outside = torch.ones_like(ybuf, dtype=torch.bool)
    outside[1:M + 1, 3:N + 3] = False
    assert (bits(ybuf)[outside] == PATTERN).all()


def test_row_contract():
    """An output row is a function of its input row alone, across the three instantiations and from call to call."""
    x, codes, exp, b = _inputs(128, 100, 768, seed=2)
    run = lambda t: get_ext().linear_rows_fp8(t, codes, exp, b, 1)  # noqa: E731
    full, twelve, one = run(x), run(x[:12]), run(x[7:8])
    assert torch.equal(bits(full), bits(run(x)))
    assert torch.equal(bits(twelve[5:9]), bits(run(x[5:9]))) and torch.equal(bits(twelve), bits(full[:12]))
    for M in (33, 128):
        other = torch.cat([torch.randn(M - 1, 768, device="cuda").bfloat16(), x[7:8]])  # the row last, new company
        assert torch.equal(bits(run(other)[M - 1:]), bits(one))


def test_declined_cases_take_the_pytorch_path():
    ext = get_ext()
    for M, K, dtype in ((129, 256, torch.bfloat16), (4, 96, torch.bfloat16), (4, 256, torch.float32)):
        x, codes, exp, b = _inputs(M, 40, K, seed=3)
        x, b = x.to(dtype), b.to(dtype)
        assert ext.linear_rows_fp8(x, codes, exp, b, 1) is None
        got = linear_rows_fp8(x, codes, exp, b, act="gelu")
        assert got.dtype == dtype and _worst(got, x, codes, exp, b, "gelu") <= 1.0
    x, codes, exp, b = _inputs(4, 40, 256)
    for bad in (lambda: ext.linear_rows_fp8(x, codes[:, :128], exp, b, 0), lambda: ext.linear_rows_fp8(x, codes, exp[:39], b, 0),
                lambda: ext.linear_rows_fp8(x, codes, exp, b[:39], 0), lambda: ext.linear_rows_fp8(x, codes.char(), exp, b, 0),
                lambda: ext.linear_rows_fp8(x, codes, exp.byte(), b, 0), lambda: ext.linear_rows_fp8(x, codes, exp, b, 7)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError):
        linear_rows_fp8(x, codes, exp, b, act="relu")


class _Fp8:
    def __init__(self, model):
        self.init_cache, self.cfg = model.init_cache, model.cfg
        for name in ("prefill", "decode_step"):
            setattr(self, name, functools.partial(getattr(model, name), decode_linears="rows_fp8"))


@functools.lru_cache(maxsize=None)
def _fixed_point_models(heads):
    """``_models`` built afresh (the shared ones stay as they are) with every Linear weight and ``wte`` replaced, in the
    fp32 model and in the bf16 shadows alike, by its own dequantized quantization: a fixed point of the format."""
    torch.manual_seed(0)
    ref = build_model(precision="fp32", num_heads=heads, **TINY).cuda().eval()
    nat = build_model(precision="bf16", num_heads=heads, **TINY).cuda().eval()
    nat.load_state_dict(ref.state_dict())
    eng = DDPEngine(nat, shadow_dtype=torch.bfloat16)
    with torch.no_grad():
        for m in (ref, nat):
            for w in [m.wte.weight] + [lin.weight for blk in m.h
                                       for lin in (blk.attn.qkv, blk.attn_proj, blk.mlp_fc, blk.mlp_proj)]:
                fixed = kv_dequantize(*kv_quantize_ref(w))
                assert torch.equal(kv_dequantize(*kv_quantize_ref(fixed)), fixed)
                w.copy_(fixed)
                if m is nat:
                    w._dpa_shadow.copy_(fixed)
                    assert torch.equal(w._dpa_shadow.float(), fixed)  # the bf16 forward sees the same values
    return ref, nat, eng


@pytest.mark.parametrize("heads", [4, 2])
def test_teacher_forced_rows_fp8_logits_match_the_fp32_forward(heads):
    """On fixed-point weights ``rows_fp8`` computes with exactly the weights of the fp32 forward.  The bound of
    ``test_linear_rows_gpu.py``: twice the native full forward's own error over the same positions."""
    ref, nat, _ = _fixed_point_models(heads)
    ids = torch.randint(1000, 3000, (4, 96), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with torch.no_grad():
        want, full = ref(ids).float(), nat(ids).float()
    got, _ = teacher_forced(_Fp8(nat), ids, [1, 5, 64, 65], 65)
    e_fp8 = max((got[(b, p)] - want[b, p]).abs().max().item() for (b, p) in got)
    e_full = max((full[b, p] - want[b, p]).abs().max().item() for (b, p) in got)
    print(f"heads={heads}: rows_fp8 path max |err| = {e_fp8:.4e}, native full forward max |err| = {e_full:.4e}")
    assert e_fp8 <= 2 * e_full, (e_fp8, e_full)


@pytest.mark.parametrize("heads,kv", [(4, "bf16"), (2, "bf16"), (4, "fp8")])
def test_greedy_generate_rows_fp8_equals_the_written_out_loop(heads, kv):
    nat, rows = _models(heads)[1], _Fp8(_models(heads)[1])
    ids, lens = bsh.prompts("cuda", TINY["vocab_size"])
    a, na = nat.generate(ids, lens, 24, temperature=0, decode_linears="rows_fp8", kv_dtype=kv)
    b, nb = nat.generate(ids, lens, 24, temperature=0, decode_linears="rows_fp8", kv_dtype=kv)
    assert torch.equal(a, b) and torch.equal(na, nb) and na.tolist() == [24] * 3
    cache = nat.init_cache(3, 64, kv_dtype=kv)
    toks = [lms.greedy(rows.prefill(ids, lens, cache))]
    for _ in range(23):
        toks.append(lms.greedy(rows.decode_step(toks[-1], cache)))
    assert torch.equal(a, torch.stack(toks, 1))
