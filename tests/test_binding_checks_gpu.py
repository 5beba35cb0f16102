"""Refusal and decline paths of the native bindings: every case here is turned away by the
binding's own argument checks, before any kernel is launched (read in csrc/bind_*.cpp), so a
wrong answer is an exception that is missing or a result that is not None / False / [].

raises: RuntimeError.  none / false: the op declines with that value and runs nothing.
The last test is the one "ignored" case: an unusable accumulator is passed over, not refused.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ext():
    from distributed_pipeline_amd.ops._ext import get_ext
    return get_ext(required=True)


def bf(*shape):
    return torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)


def f32(*shape):
    return torch.zeros(*shape, device="cuda", dtype=torch.float32)


def i64(*shape):
    return torch.zeros(*shape, device="cuda", dtype=torch.int64)


def i32(*shape):
    return torch.zeros(*shape, device="cuda", dtype=torch.int32)


def off_by_one(rows, cols):
    """Contiguous bf16 [rows, cols] that starts 2 bytes past a 16-byte boundary."""
    return bf(rows * cols + 8)[1:1 + rows * cols].view(rows, cols)


def _xent_rows_cases():
    cases = []
    for op, tail in (("xent_rows_fwd", lambda: ()), ("xent_rows_fwd_grad_", lambda: ()),
                     ("xent_rows_bwd_", lambda: (f32(8), f32(8)))):
        cases += [
            (op + "-row-not-x8", op, lambda tail=tail: ((bf(8, 100), 50, i64(8)) + tail(), {}), "raises"),
            (op + "-V-gt-row", op, lambda tail=tail: ((bf(8, 128), 129, i64(8)) + tail(), {}), "raises"),
            (op + "-misaligned", op, lambda tail=tail: ((off_by_one(8, 128), 100, i64(8)) + tail(), {}), "raises"),
        ]
    return cases


def _token_group_cases():
    cases = []
    for op in ("ngram_matches", "ngram_distinct", "lcs_lengths"):
        cases += [
            (op + "-i64-lens", op, lambda: ((i32(2, 3, 16), i64(2, 3)), {}), "raises"),
            (op + "-float-tokens", op, lambda: ((f32(2, 3, 16), i32(2, 3)), {}), "raises"),
            (op + "-lens-shape", op, lambda: ((i32(2, 3, 16), i32(2, 4)), {}), "raises"),
        ]
    return cases


def _adamw(n=8, emas=1, rates=1, skip=None, clip=None, shadow=None, ema_list=None):
    ema_list = [f32(n) for _ in range(emas)] if ema_list is None else ema_list
    return ((f32(n), f32(n), f32(n), f32(n), shadow, ema_list, [0.999] * rates,
             1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, clip, skip), {})


def host(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype)


def strided(n, make=f32):
    """n elements at stride 2, starting on an allocation boundary: only contiguity is wrong."""
    return make(2 * n)[::2]


def _flat_optim_cases():
    """One row per device / contiguity / size / alignment check of the flat optimizer ops; every
    other argument of a row is valid, so the named check is the one that refuses it."""
    return [
        ("sqnorm-host-partial", "sqnorm", lambda: ((f32(8), host(4), f32(3), 1.0, 1.0), {}), "raises"),
        ("sqnorm-host-out", "sqnorm", lambda: ((f32(8), f32(4), host(3), 1.0, 1.0), {}), "raises"),
        ("sqnorm-strided-partial", "sqnorm", lambda: ((f32(8), strided(4), f32(3), 1.0, 1.0), {}), "raises"),
        ("sqnorm-strided-out", "sqnorm", lambda: ((f32(8), f32(4), strided(3), 1.0, 1.0), {}), "raises"),
        ("sqnorm-empty-partial", "sqnorm", lambda: ((f32(8), f32(0), f32(3), 1.0, 1.0), {}), "raises"),
        ("adamw_ema-host-clip", "adamw_ema", lambda: _adamw(clip=host(3)), "raises"),
        ("adamw_ema-strided-clip", "adamw_ema", lambda: _adamw(clip=strided(3)), "raises"),
        ("adamw_ema-clip-1-float", "adamw_ema", lambda: _adamw(clip=f32(1)), "raises"),
        ("adamw_ema-host-ema", "adamw_ema", lambda: _adamw(ema_list=[host(8)]), "raises"),
        ("adamw_ema-host-shadow", "adamw_ema", lambda: _adamw(shadow=host(8, torch.bfloat16)), "raises"),
        ("ema_update-host-ema", "ema_update", lambda: ((host(8), f32(8), 0.5), {}), "raises"),
        ("ema_update-host-param", "ema_update", lambda: ((f32(8), host(8), 0.5), {}), "raises"),
        ("ema_update-strided-ema", "ema_update", lambda: ((strided(8), f32(8), 0.5), {}), "raises"),
        ("ema_update-strided-param", "ema_update", lambda: ((f32(8), strided(8), 0.5), {}), "raises"),
        ("cast_bf16-host-src", "cast_bf16", lambda: ((host(8), bf(8)), {}), "raises"),
        ("cast_bf16-host-dst", "cast_bf16", lambda: ((f32(8), host(8, torch.bfloat16)), {}), "raises"),
        ("cast_bf16-strided-src", "cast_bf16", lambda: ((strided(8), bf(8)), {}), "raises"),
        ("cast_bf16-strided-dst", "cast_bf16", lambda: ((f32(8), strided(8, bf)), {}), "raises"),
        # 4 bytes past an 8-byte boundary: the kernel stores 4 bf16 as one 8-byte word
        ("cast_bf16-dst-4B-aligned", "cast_bf16", lambda: ((f32(8), bf(12)[2:10]), {}), "raises"),
    ]


def _reverse(N=4, E=8, **kw):
    return ((f32(1), N, E), kw)


# (id, op, () -> (args, kwargs), expectation)
CASES = [
    ("gemm_nt-fp32-x", "gemm_nt", lambda: ((f32(128, 256), bf(128, 256), None, 0), {}), "raises"),
    ("gemm_nt-W-K", "gemm_nt", lambda: ((bf(128, 256), bf(128, 128), None, 0), {}), "raises"),
    ("gemm_nt-x-transposed", "gemm_nt", lambda: ((bf(256, 128).t(), bf(128, 256), None, 0), {}), "raises"),
    ("gemm_nn_dact-act5-bf16-aux", "gemm_nn_dact",
     lambda: ((bf(128, 128), bf(128, 256), bf(128, 256), 5), {}), "raises"),
    ("gemm_nn_dact-aux-shape", "gemm_nn_dact",
     lambda: ((bf(128, 128), bf(128, 256), bf(128, 128), 1), {}), "raises"),
    ("gemm_wgrad-bf16-dW", "gemm_wgrad", lambda: ((bf(128, 128), bf(128, 256), bf(128, 256), None), {}), "raises"),
    ("gemm_wgrad-db-length", "gemm_wgrad",
     lambda: ((bf(128, 128), bf(128, 256), f32(128, 256), f32(64)), {}), "raises"),
    ("gemm_wgrad_multi-segment-shape", "gemm_wgrad_multi",
     lambda: (([bf(128, 128), bf(64, 128)], [bf(128, 256), bf(64, 256)], f32(128, 256)), {}), "raises"),
    ("transpose-list-lengths", "transpose_bf16_batch", lambda: (([bf(64, 64), bf(64, 64)], [bf(64, 64)]), {}),
     "raises"),
    ("add_ln_fwd-gamma-length", "add_ln_fwd",
     lambda: ((bf(64, 128), None, bf(64), bf(128), 0.0, 1e-5, 1, 0), {}), "raises"),
    ("add_ln_fwd-res-shape", "add_ln_fwd",
     lambda: ((bf(64, 128), bf(32, 128), bf(128), bf(128), 0.0, 1e-5, 1, 0), {}), "raises"),
    ("add_ln_fwd-pos-R-mod-L", "add_ln_fwd",
     lambda: ((bf(100, 128), None, bf(128), bf(128), 0.0, 1e-5, 1, 0), {"pos": bf(64, 128), "L": 64}), "raises"),
    ("add_ln_bwd-beta-no-hcopy", "add_ln_bwd",
     lambda: ((bf(64, 128), bf(64, 128), f32(64), f32(64), bf(128), 0.0, 1, 0, True, True), {"beta": bf(128)}),
     "raises"),
    ("add_ln_bwd-part_buf-size", "add_ln_bwd",
     lambda: ((bf(64, 128), bf(64, 128), f32(64), f32(64), bf(128), 0.0, 1, 0, True, True),
              {"dg_acc": f32(128), "db_acc": f32(128), "part_buf": f32(7)}), "raises"),
    ("attn_fwd-head_dim-32", "attn_fwd", lambda: ((bf(1, 64, 192), 2, 0.0, False, 1, 0), {}), "raises"),
    ("attn_fwd-L-96", "attn_fwd", lambda: ((bf(1, 96, 192), 1, 0.0, False, 1, 0), {}), "raises"),
    ("attn_fwd-head_major-L-64", "attn_fwd",
     lambda: ((bf(1, 64, 192), 1, 0.0, False, 1, 0), {"head_major": True}), "raises"),
    ("attn_bwd-lse-size", "attn_bwd",
     lambda: ((bf(1, 64, 64), bf(1, 64, 192), bf(1, 64, 64), f32(1, 1, 32), 1, 0.0, False, 1, 0), {}), "raises"),
    ("lxent_fwd-E-64", "lxent_fwd", lambda: ((bf(16, 64), bf(32, 64), None, i64(16)), {}), "raises"),
    ("lxent_fwd-i32-targets", "lxent_fwd", lambda: ((bf(16, 128), bf(32, 128), None, i32(16)), {}), "raises"),
    ("lxent_fwd-bias-length", "lxent_fwd", lambda: ((bf(16, 128), bf(32, 128), bf(31), i64(16)), {}), "raises"),
    ("linear_argmax-c-length", "linear_argmax", lambda: ((bf(16, 128), bf(32, 128), f32(31)), {}), "raises"),
    ("linear_argmax-W-no-rows", "linear_argmax", lambda: ((bf(16, 128), bf(0, 128)), {}), "raises"),
    *_xent_rows_cases(),
    ("reverse_step-E-6", "reverse_step", lambda: _reverse(E=6), "raises"),
    ("reverse_step-a-no-source", "reverse_step", lambda: _reverse(a=1.0), "raises"),
    ("reverse_step-mask-no-x_start", "reverse_step", lambda: _reverse(mask=i64(4)), "raises"),
    ("reverse_step-idx-no-W", "reverse_step", lambda: _reverse(idx=i64(4), a=1.0), "raises"),
    *_token_group_cases(),
    ("emb_grad-i32-ids", "emb_grad", lambda: ((i32(16), f32(16, 128), f32(32, 128)), {}), "raises"),
    ("emb_grad-dy-size", "emb_grad", lambda: ((i64(16), f32(15, 128), f32(32, 128)), {}), "raises"),
    ("adamw_ema-length-not-x4", "adamw_ema", lambda: _adamw(n=6), "raises"),
    ("adamw_ema-emas-vs-rates", "adamw_ema", lambda: _adamw(emas=2, rates=1), "raises"),
    ("adamw_ema-i64-skip", "adamw_ema", lambda: _adamw(skip=i64(1)), "raises"),
    ("sqnorm-out-2", "sqnorm", lambda: ((f32(8), f32(4), f32(2), 1.0, 1.0), {}), "raises"),
    *_flat_optim_cases(),
    ("sample_tokens-temperature-0", "sample_tokens", lambda: ((f32(2, 64), 0.0, 0, 1.0, 1, 0, 0), {}), "raises"),
    # declines
    ("attn_decode-head_dim-32", "attn_decode",
     lambda: ((bf(2, 192), bf(2, 2, 16, 32), bf(2, 2, 16, 32), i32(2), 2), {}), "none"),
    ("attn_decode-fp32-caches", "attn_decode",
     lambda: ((bf(2, 384), f32(2, 2, 16, 64), f32(2, 2, 16, 64), i32(2), 2), {}), "none"),
    # one row past the kernel's widest vocabulary: the only case here above [128, 256] elements
    ("sample_tokens-V-65537", "sample_tokens", lambda: ((f32(1, 65537), 1.0, 0, 1.0, 1, 0, 0), {}), "none"),
    ("sample_tokens-fp16", "sample_tokens",
     lambda: ((torch.zeros(2, 64, device="cuda", dtype=torch.float16), 1.0, 0, 1.0, 1, 0, 0), {}), "none"),
    ("transpose-32x64", "transpose_bf16_batch", lambda: (([bf(32, 64)], [bf(64, 32)]), {}), "false"),
    ("gemm_wgrad_multi-9-segments", "gemm_wgrad_multi",
     lambda: (([bf(128, 128) for _ in range(9)], [bf(128, 128) for _ in range(9)], f32(128, 128)), {}), "false"),
    ("gemm_wgrad_grouped-9-segments", "gemm_wgrad_grouped",
     lambda: (([[bf(128, 128) for _ in range(9)]], [[bf(128, 128) for _ in range(9)]], [f32(128, 128)], [None]),
              {}), "false"),
]


@pytest.mark.parametrize("op,make,expect", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_binding_refuses_or_declines(op, make, expect):
    fn = getattr(_ext(), op)
    args, kwargs = make()
    if expect == "raises":
        with pytest.raises(RuntimeError):
            fn(*args, **kwargs)
        return
    got = fn(*args, **kwargs)
    assert got is {"none": None, "false": False}[expect]
    torch.cuda.synchronize()


def test_add_ln_bwd_ignores_unusable_accumulator():
    """A dg_acc of the wrong length is not refused: dgamma comes back as without it and the
    buffer stays as it was.  Shape: the smallest of test_norm_act_kernels.py."""
    ext = _ext()
    R, D = 64, 64
    torch.manual_seed(0)
    y = torch.randn(R, D, device="cuda").bfloat16()
    r = torch.randn(R, D, device="cuda").bfloat16()
    g = (1 + 0.1 * torch.randn(D, device="cuda")).bfloat16()
    b = (0.1 * torch.randn(D, device="cuda")).bfloat16()
    _, hs, mean, rstd = ext.add_ln_fwd(y, r, g, b, 0.0, 1e-12, 1, 0)
    dout = torch.randn(R, D, device="cuda").bfloat16()
    ref = ext.add_ln_bwd(dout, hs, mean, rstd, g, 0.0, 1, 0, True, True, True)
    bad = torch.full((D + 4,), 7.0, device="cuda")
    got = ext.add_ln_bwd(dout, hs, mean, rstd, g, 0.0, 1, 0, True, True, True, dg_acc=bad)
    assert got[2] is not None and got[2].shape == (D,)
    # the column sums of R = 64 fp32 terms may be associated differently from call to call
    # (atomics): R * 2^-24 relative to the largest sum bounds that, far below 1e-5
    torch.testing.assert_close(got[2], ref[2], rtol=1e-5, atol=1e-5 * ref[2].abs().max().item())
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(bad, torch.full((D + 4,), 7.0, device="cuda"))
