"""The one-byte K/V cache on the GPU: csrc/attn_decode_fp8.hip (the quantizing store, and K-M25: the
quantizing append + single-query attention) against the independent yardstick of kv_fp8_helpers.py -
codes and exponents bit for bit, the attention against the float64 definition on the dequantized
caches - and the model's ``prefill`` / ``decode_step`` / ``generate`` on an fp8 cache.

Allowed attention error per element: ``2^-8 |o_ref| + 4 e32`` (the rule of test_attn_decode_gpu.py): one
bf16 ulp of the float64 reference plus four times ``e32``, the largest absolute error of the fp32 PyTorch
path (``attention_decode_fp8_ref`` on fp32 copies of the same inputs and the same caches) against the
same reference, over the input set.

Every cache is a view into a larger buffer that holds a byte pattern, with spare rows in front of and
behind each (b, h) block, so a stray store changes the pattern instead of faulting.

Measured on one MI355X: worst attention error over bound 0.980 / 0.981 (D = 64, normal / ramp) and 0.991 /
0.986 (D = 128); teacher-forced logits, largest absolute error against the fp32 full forward: E_bf16 =
1.13e-02, E_q = 2.73e-02, E_8 = 3.07e-02 at D = 64 and 1.28e-02, 3.27e-02, 3.25e-02 at D = 128.
"""
import functools
import math

import numpy as np
import pytest
import torch

import kv_fp8_helpers as kv
from decode_helpers import TINY
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops import decode as dec
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import token_stats
from distributed_pipeline_amd.parallel.ddp import DDPEngine
from utils import lm_sampling as lms

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, LMAX = kv.B, kv.H, kv.LMAX
BF = torch.bfloat16


def _kernel(qkv, k8, ke, v8, ve, lens, heads):
    out = get_ext().attn_decode_fp8(qkv, k8, ke, v8, ve, lens, heads)
    assert out is not None, "the kernel must take bf16 D in {64, 128}"
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- the quantizer and the store ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("D", [64, 128])
def test_quantizer_bit_for_bit(D, dtype):
    """bf16: the kernel (v_cvt_pk_fp8_f32); fp32: the PyTorch path on the device."""
    if dtype == BF:
        x = kv.quantizer_rows(D).to(BF).cuda()
        assert get_ext().kv8_quantize(x) is not None
    kv.check_quantizer(DEV, D, dtype)


def test_quantize_declines_and_keeps_shapes():
    ext = get_ext()
    x = torch.randn(4, 5, 64, device=DEV).to(BF)
    codes, exps = dec.kv_quantize(x)
    assert codes.shape == (4, 5, 64) and exps.shape == (4, 5)
    want_c, want_e = kv.yard_quantize(x)
    assert np.array_equal(codes.cpu().numpy(), want_c) and np.array_equal(exps.cpu().numpy(), want_e)
    assert ext.kv8_quantize(torch.randn(4, 32, device=DEV).to(BF)) is None   # D outside {64, 128}
    assert ext.kv8_quantize(torch.randn(4, 64, device=DEV)) is None          # fp32
    assert ext.kv8_quantize(torch.randn(4, 64).to(BF)) is None               # a CPU tensor
    assert ext.kv8_quantize(x[:, 0]) is None                                 # rows that are not packed


@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_store(D, dtype):
    kv.check_kv_store(DEV, D, dtype)


def test_kv_store_takes_the_kernel_and_declines_what_it_cannot():
    ext = get_ext()
    D, L = 64, 70
    qkv = torch.randn(B, L, 3 * H * D, device=DEV).to(BF)
    lens = torch.tensor([1, 64, 70], dtype=torch.int32, device=DEV)
    cbuf, ebuf, *views = kv.guarded_fp8(B, H, LMAX, D, DEV)
    assert ext.kv8_store(qkv, lens, *views) is True
    before_c, before_e = cbuf.clone(), ebuf.clone()
    assert ext.kv8_store(qkv.float(), lens, *views) is False                 # fp32: the PyTorch path's
    _, _, *small = kv.guarded_fp8(B, H, LMAX, 32, DEV)
    assert ext.kv8_store(torch.randn(B, L, 3 * H * 32, device=DEV).to(BF), lens, *small) is False  # D = 32
    k8, ke, v8, ve = views
    loose = torch.zeros(B, H, LMAX, 2 * D, dtype=torch.uint8, device=DEV)[..., :D]  # rows that are not packed
    assert ext.kv8_store(qkv, lens, loose, ke, v8, ve) is False
    assert torch.equal(cbuf, before_c) and torch.equal(ebuf, before_e)          # a declined call writes nothing
    with pytest.raises(RuntimeError):
        ext.kv8_store(qkv, lens, k8.view(torch.int8), ke, v8, ve)                # codes must be uint8
    with pytest.raises(RuntimeError):
        ext.kv8_store(qkv, lens.long(), k8, ke, v8, ve)                          # lens must be int32
    with pytest.raises(RuntimeError):
        ext.kv8_store(torch.zeros(B, LMAX + 1, 3 * H * D, device=DEV, dtype=BF), lens, k8, ke, v8, ve)  # too long


# ---- attention over the cache ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ragged(D, kind):
    g = torch.Generator().manual_seed(1000 * D + len(kind))
    lens = kv.chunk_lens(D)
    return [kv.attn_run(D, kind, lens[i:i + B], g, DEV, BF, _kernel) for i in range(0, len(lens), B)]


@pytest.mark.parametrize("kind", ["normal", "ramp"])
@pytest.mark.parametrize("D", [64, 128])
def test_matches_float64(D, kind):
    runs = _ragged(D, kind)
    e32 = max(r["e32"] for r in runs)
    worst = max(kv.within_tolerance(r, e32) for r in runs)
    if kind == "ramp":  # the set is what it claims: the largest score at the last key, a span over 60
        for r in runs:
            q = r["qkv"].double().cpu().view(B, 3, H, D)[:, 0]
            kc, kx = r["new"][0], r["new"][1]
            for b, m in enumerate(r["lens"]):
                if m >= 64:
                    K = kv.yard_dequantize(r["before_c"][0, b, :, kv.SPARE:kv.SPARE + m].cpu().numpy(),
                                           r["before_e"][0, b, :, kv.SPARE:kv.SPARE + m].cpu().numpy())
                    s = torch.einsum("hd,hld->hl", q[b], torch.from_numpy(K)) / math.sqrt(D)
                    s_new = (q[b] * torch.from_numpy(kv.yard_dequantize(kc[b], kx[b]))).sum(-1) / math.sqrt(D)
                    assert (s_new > s.amax(-1)).all() and (s_new - s.amin(-1) > 60).all()
    print(f"attn_decode_fp8 D={D} {kind}: e32={e32:.3e} worst err/tol={worst:.3f}")
    assert worst <= 1.0, (worst, e32)


@pytest.mark.parametrize("kind", ["normal", "ramp"])
@pytest.mark.parametrize("D", [64, 128])
def test_append_writes_the_quantized_row_and_nothing_else(D, kind):
    for r in _ragged(D, kind):
        want_c, want_e = kv.expected_buffers(r, DEV)
        assert torch.equal(r["cbuf"], want_c), "codes"
        assert torch.equal(r["ebuf"], want_e), "exponents"
        assert r["lens_t"].tolist() == list(r["lens"])  # lens is the caller's to advance


@pytest.mark.parametrize("D", [64, 128])
def test_rows_beyond_lens_are_never_read(D):
    lens = (0, 33, 300)
    outs = []
    for tail in ((0, 0), (0x7F, 127), (0xFF, -128), (0x7F, 0)):  # zeros, NaN codes, wild exponents
        g = torch.Generator().manual_seed(7)
        outs.append(kv.attn_run(D, "normal", lens, g, DEV, BF, _kernel, tail=tail)["out"])
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(bits(o), bits(outs[0]))


@pytest.mark.parametrize("D", [64, 128])
def test_inactive_rows(D):
    lens = (-1, 5, LMAX, 300, LMAX + 5, 0)
    g = torch.Generator().manual_seed(8)
    r = kv.attn_run(D, "normal", lens, g, DEV, BF, _kernel)
    want_c, want_e = kv.expected_buffers(r, DEV)
    assert torch.equal(r["cbuf"], want_c) and torch.equal(r["ebuf"], want_e)  # an inactive row stores nothing
    act = [b for b, m in enumerate(lens) if 0 <= m < LMAX]
    assert kv.within_tolerance(r, r["e32"], rows=act) <= 1.0
    for b, m in enumerate(lens):
        if not 0 <= m < LMAX:
            assert not bits(r["out"][b]).any()  # zeros, bit for bit
    # the active rows do not depend on their inactive neighbours
    g = torch.Generator().manual_seed(8)
    alone = kv.attn_run(D, "normal", lens, g, DEV, BF,
                        lambda qkv, k8, ke, v8, ve, lens_t, heads: _kernel(
                            qkv[act].contiguous(), k8[act], ke[act], v8[act], ve[act], lens_t[act].contiguous(), heads))
    assert torch.equal(bits(alone["out"]), bits(r["out"][act]))


def test_two_calls_agree_bitwise_and_strided_inputs_work():
    D, lens = 64, (129, 7, 319)
    outs = []
    for layout in ("packed", "packed", "wide", "odd"):
        def fn(qkv, *rest, layout=layout):
            if layout == "wide":    # rows 8 elements further apart: the kernel takes the stride
                qkv = torch.cat([qkv, torch.zeros(B, 8, dtype=qkv.dtype, device=DEV)], 1)[:, :3 * H * D]
            elif layout == "odd":   # rows that do not start on 16 bytes: the op copies
                qkv = torch.cat([qkv, torch.zeros(B, 1, dtype=qkv.dtype, device=DEV)], 1)[:, :3 * H * D]
            assert qkv.is_contiguous() == (layout == "packed")
            return dec.attention_decode_fp8(qkv, *rest)
        g = torch.Generator().manual_seed(9)
        r = kv.attn_run(D, "normal", lens, g, DEV, BF, fn)
        outs.append((r["out"], r["cbuf"], r["ebuf"]))
    for o in outs[1:]:
        assert torch.equal(bits(o[0]), bits(outs[0][0])) and torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])


def test_head_dim_32_takes_the_torch_path_and_matches():
    D, lens = 32, (0, 64, 300)
    ext = get_ext()
    g = torch.Generator().manual_seed(10)

    def fn(qkv, k8, ke, v8, ve, lens_t, heads):
        clones = [t.clone() for t in (k8, ke, v8, ve)]
        assert ext.attn_decode_fp8(qkv, *clones, lens_t, heads) is None            # D = 32
        assert all(torch.equal(a, b) for a, b in zip(clones, (k8, ke, v8, ve)))  # and nothing written
        return dec.attention_decode_fp8(qkv, k8, ke, v8, ve, lens_t, heads)

    r = kv.attn_run(D, "normal", lens, g, DEV, BF, fn)
    assert r["out"].dtype == BF and kv.within_tolerance(r, r["e32"]) <= 1.0
    want_c, want_e = kv.expected_buffers(r, DEV)
    assert torch.equal(r["cbuf"], want_c) and torch.equal(r["ebuf"], want_e)


def test_what_the_binding_declines_and_rejects():
    ext = get_ext()
    D = 64
    qkv = torch.randn(B, 3 * H * D, device=DEV).to(BF)
    lens = torch.tensor([3, 0, 9], dtype=torch.int32, device=DEV)
    _, _, k8, ke, v8, ve = kv.guarded_fp8(B, H, LMAX, D, DEV)
    assert ext.attn_decode_fp8(qkv.float(), k8, ke, v8, ve, lens, H) is None                    # fp32 compute
    assert ext.attn_decode_fp8(*(t.cpu() for t in (qkv, k8, ke, v8, ve, lens)), H) is None      # CPU tensors
    loose = torch.zeros(B, H, LMAX, 2 * D, dtype=torch.uint8, device=DEV)[..., :D]              # rows not packed
    assert ext.attn_decode_fp8(qkv, loose, ke, v8, ve, lens, H) is None
    off = torch.zeros(B * H * LMAX * D + 8, dtype=torch.uint8, device=DEV)[8:].view(B, H, LMAX, D)  # base off 16 bytes
    assert ext.attn_decode_fp8(qkv, off, ke, v8, ve, lens, H) is None
    sparse_e = torch.zeros(B, H, LMAX, 2, dtype=torch.int8, device=DEV)[..., 0]                 # exponents not packed
    assert ext.attn_decode_fp8(qkv, k8, sparse_e, v8, ve, lens, H) is None
    with pytest.raises(RuntimeError):
        ext.attn_decode_fp8(qkv, k8.view(torch.int8), ke, v8, ve, lens, H)       # codes must be uint8
    with pytest.raises(RuntimeError):
        ext.attn_decode_fp8(qkv, k8, ke.view(torch.uint8), v8, ve, lens, H)      # exponents must be int8
    with pytest.raises(RuntimeError):
        ext.attn_decode_fp8(qkv, k8, ke[:, :, :-1], v8, ve, lens, H)             # shapes that do not agree
    with pytest.raises(RuntimeError):
        ext.attn_decode_fp8(qkv, k8, ke, v8, ve, lens.long(), H)                 # lens must be int32
    with pytest.raises(RuntimeError):
        ext.attn_decode_fp8(qkv, k8, ke, v8, ve, lens, H + 1)                    # heads
    torch.cuda.synchronize()


# ---- the model ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _models(heads):
    torch.manual_seed(0)
    ref = build_model(precision="fp32", num_heads=heads, **TINY).cuda().eval()
    nat = build_model(precision="bf16", num_heads=heads, **TINY).cuda().eval()
    nat.load_state_dict(ref.state_dict())
    eng = DDPEngine(nat, shadow_dtype=torch.bfloat16)  # attaches the bf16 weight shadows
    return ref, nat, eng


@pytest.mark.parametrize("heads", [4, 2])
def test_teacher_forced_logits_against_the_fp32_forward(heads):
    """E_8 <= 2 (E_q + E_bf16): the native model on the fp8 cache may be off by the format's own error
    (E_q: the fp32 model on the fp8 cache, PyTorch path) plus the native model's on the bf16 cache
    (E_bf16), with the factor 2 this project gives its model-level bounds.  All three are largest
    absolute logit errors against the fp32 model's full forward over the same (row, position) set."""
    ref, nat, _ = _models(heads)
    L, plens = 80, [1, 5, 64, 65]
    ids = torch.randint(1000, 3000, (4, L), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    with torch.no_grad():
        want = ref(ids).float()

    def worst(got):
        assert len(got) == sum(L - p + 1 for p in plens)
        return max((got[(b, p)] - want[b, p]).abs().max().item() for (b, p) in got)

    e_bf16 = worst(kv.teacher_forced_on(nat, ids, plens, 65, nat.init_cache(4, L + 8)))
    e_q = worst(kv.teacher_forced_on(ref, ids, plens, 65, ref.init_cache(4, L + 8, kv_dtype="fp8")))
    cache = nat.init_cache(4, L + 8, kv_dtype="fp8")
    kv.fill_pattern(cache)
    e_8 = worst(kv.teacher_forced_on(nat, ids, plens, 65, cache))
    print(f"heads={heads}: E_bf16 = {e_bf16:.4e}  E_q = {e_q:.4e}  E_8 = {e_8:.4e}")
    # every row ran the L - 1 steps of the shortest one (or until its cache was full): codes and exponents
    # behind that keep their pattern
    for b, p in enumerate(plens):
        n = min(p + L - 1, L + 8)
        assert (cache.buf[:, :, b, :, n:] == kv.PAT).all() and (cache.ebuf[:, :, b, :, n:] == kv.PAT).all()
        assert not (cache.ebuf[:, :, b, :, :n] == kv.PAT).any()
    assert e_8 <= 2 * (e_q + e_bf16), (e_8, e_q, e_bf16)


@pytest.mark.parametrize("heads", [4, 2])
def test_the_native_model_runs_the_kernels(heads, monkeypatch):
    """prefill and decode_step of the bf16 model on an fp8 cache from ``init_cache`` take csrc/attn_decode_fp8.hip
    in every layer - no call is declined and served by the PyTorch path - and a cache whose rows the
    kernels decline (views off 16 bytes) gets the same bytes from the PyTorch path."""
    _, nat, _ = _models(heads)
    ext = get_ext()
    calls = {"store": 0, "step": 0}

    def store(*a):
        calls["store"] += 1
        ok = real_store(*a)
        assert ok is True, "the store kernel declined the model's own cache"
        return ok

    def step(*a):
        calls["step"] += 1
        out = real_step(*a)
        assert out is not None, "the decode kernel declined the model's own cache"
        return out

    real_store, real_step = ext.kv8_store, ext.attn_decode_fp8
    ids = torch.randint(1000, 3000, (3, 70), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    lens = torch.tensor([70, 1, 33], dtype=torch.int32, device=DEV)
    cache = nat.init_cache(3, 80, kv_dtype="fp8")
    kv.fill_pattern(cache)
    monkeypatch.setattr(ext, "kv8_store", store)
    monkeypatch.setattr(ext, "attn_decode_fp8", step)
    nat.prefill(ids, lens, cache)
    for t in range(3):
        nat.decode_step(ids[:, t], cache)
    assert calls == {"store": len(nat.h), "step": 3 * len(nat.h)}
    monkeypatch.undo()
    # the same steps on views the kernels decline: code rows 8 bytes off a 16-byte boundary
    D = cache.head_dim
    off = nat.init_cache(3, 80, kv_dtype="fp8")
    raw = torch.full((off.buf.numel() + 8,), kv.PAT, dtype=torch.uint8, device=DEV)
    off.buf = raw[8:].view(off.buf.shape)
    off.ebuf.fill_(kv.PAT)
    off.k = [off.buf[i, 0] for i in range(len(nat.h))]
    off.v = [off.buf[i, 1] for i in range(len(nat.h))]
    assert ext.kv8_store(torch.zeros(3, 1, 3 * heads * D, device=DEV, dtype=BF), lens, off.k[0], off.ke[0], off.v[0],
                         off.ve[0]) is False
    nat.prefill(ids, lens, off)
    after_prefill = nat.init_cache(3, 80, kv_dtype="fp8")
    kv.fill_pattern(after_prefill)
    nat.prefill(ids, lens, after_prefill)
    assert torch.equal(off.buf, after_prefill.buf) and torch.equal(off.ebuf, after_prefill.ebuf)  # every layer
    for t in range(3):
        nat.decode_step(ids[:, t], off)
    # layer 0's new k and v do not depend on any attention output: the appended bytes are the kernel's.  (A
    # later layer sees the bf16 rounding of sums taken in another order.)
    assert torch.equal(off.buf[0], cache.buf[0]) and torch.equal(off.ebuf[0], cache.ebuf[0])
    assert off.lens.tolist() == cache.lens.tolist()


def _prompts(seed=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ids = torch.randint(1000, 3000, (4, 40), device=DEV, generator=g)
    return ids, torch.tensor([40, 17, 1, 33], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("heads", [4, 2])
def test_greedy_generate_is_reproducible_and_equals_the_written_out_loop(heads):
    _, nat, _ = _models(heads)
    ids, lens = _prompts()
    a, na, lpa = nat.generate(ids, lens, 24, temperature=0, kv_dtype="fp8", return_logprobs=True)
    b, nb, lpb = nat.generate(ids, lens, 24, temperature=0, kv_dtype="fp8", return_logprobs=True)
    assert torch.equal(a, b) and torch.equal(na, nb) and torch.equal(lpa, lpb) and na.tolist() == [24] * 4
    cache = nat.init_cache(4, 64, kv_dtype="fp8")
    logits = nat.prefill(ids, lens, cache)
    for t in range(24):
        tok = lms.greedy(logits)
        assert torch.equal(tok, a[:, t])
        assert torch.equal(lpa[:, t], token_stats(logits, tok)[0])  # bit for bit
        if t < 23:
            logits = nat.decode_step(tok, cache)
    assert cache.lens.tolist() == [int(n) + 23 for n in lens.tolist()]
    # the prefill's store: the yardstick's codes of the layer's own K and V would need the activations;
    # what can be said from outside is that the prompt rows were written and dequantize to finite values
    assert torch.isfinite(dec.kv_dequantize(cache.k[0][0, :, :40], cache.ke[0][0, :, :40])).all()


@pytest.mark.parametrize("heads", [4, 2])
def test_eos_parks_a_row_and_the_keywords_work(heads):
    _, nat, _ = _models(heads)
    ids, lens = _prompts()
    free, _ = nat.generate(ids, lens, 16, temperature=0, kv_dtype="fp8")
    eos = int(free[0, 0])
    cache = nat.init_cache(4, 56, kv_dtype="fp8")
    kv.fill_pattern(cache)
    toks, new_lens = nat.generate(ids, lens, 16, temperature=0, eos_id=eos, cache=cache)
    assert toks[0].tolist() == [eos] * 16 and int(new_lens[0]) == 1 and int(cache.lens[0]) == -1
    # row 0 never ran a decode step: beyond its 40 prompt rows codes and exponents hold the pattern
    assert (cache.buf[:, :, 0, :, 40:] == kv.PAT).all() and (cache.ebuf[:, :, 0, :, 40:] == kv.PAT).all()
    assert not (cache.ebuf[:, :, 0, :, :40] == kv.PAT).any()
    for b in (1, 2, 3):
        row = free[b].tolist()
        if eos in row:
            cut = row.index(eos) + 1
            assert toks[b].tolist() == row[:cut] + [eos] * (16 - cut) and int(new_lens[b]) == cut
        else:
            assert toks[b].tolist() == row and int(new_lens[b]) == 16
            n = int(lens[b]) + 15
            assert int(cache.lens[b]) == n
            assert (cache.buf[:, :, b, :, n:] == kv.PAT).all() and (cache.ebuf[:, :, b, :, n:] == kv.PAT).all()
    kw = dict(temperature=0.8, top_k=20, noise_seed=5, repetition_penalty=1.3, no_repeat_ngram=2, kv_dtype="fp8")
    x, y = nat.generate(ids, lens, 8, **kw), nat.generate(ids, lens, 8, **kw)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def test_beam_search_and_lookahead_refuse_an_fp8_cache():
    _, nat, _ = _models(4)
    ids, lens = _prompts()
    with pytest.raises(ValueError, match="fp8"):
        nat.beam_search(ids, lens, 4, num_beams=2, cache=nat.init_cache(8, 48, kv_dtype="fp8"))
    with pytest.raises(ValueError, match="fp8"):
        nat.generate_lookahead(ids, lens, 4, lookahead=3, cache=nat.init_cache(4, 48, kv_dtype="fp8"))
    with pytest.raises(ValueError, match="fp8"):
        nat.decode_block(ids[:, :2], nat.init_cache(4, 48, kv_dtype="fp8"))
