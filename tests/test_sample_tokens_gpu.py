"""csrc/sample.hip (``ops.decode.sample_tokens`` / ``sample_uniforms`` on a HIP device) against the
float64 yardstick of ``sample_helpers.py`` and against the op's PyTorch path on a CPU copy, and
``GPT2LMModel.generate(noise_seed=...)`` on the native bf16 model."""
import functools

import numpy as np
import pytest
import torch

import sample_helpers as sh
from decode_helpers import TINY
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.decode import sample_tokens, sample_uniforms, sample_uniforms_ref
from distributed_pipeline_amd.parallel.ddp import DDPEngine

pytestmark = pytest.mark.gpu


def test_the_kernel_runs_and_declines_what_it_does_not_cover():
    ext = get_ext(required=True)
    x = torch.randn(3, 300, device="cuda")
    out = ext.sample_tokens(x, 1.0, 0, 0.0, 7, 0, 0, True)
    assert len(out) == 3 and out[0].shape == (3,) and out[0].is_cuda
    assert len(ext.sample_tokens(x.bfloat16(), 1.0, 0, 0.0, 7, 0, 0, False)) == 1
    assert ext.sample_tokens(x.half(), 1.0, 0, 0.0, 7, 0, 0, False) is None          # dtype
    assert ext.sample_tokens(x.cpu(), 1.0, 0, 0.0, 7, 0, 0, False) is None           # not on the device
    assert ext.sample_tokens(x.t().contiguous().t(), 1.0, 0, 0.0, 7, 0, 0, False) is None  # last stride
    assert ext.sample_tokens(torch.zeros(1, 65537, device="cuda"), 1.0, 0, 0.0, 7, 0, 0, False) is None
    # the op takes those through its PyTorch path, with the same noise
    big = torch.randn(2, 65537, device="cuda")
    tok, thr, kept = sample_tokens(big, temperature=1.0, top_k=5, seed=7, step=0, return_stats=True)
    u = sample_uniforms_ref(7, 0, 0, 2, 65537).numpy().astype(np.float64)
    sh.assert_valid_draw(tok.cpu().numpy(), thr.cpu().numpy(), sh.scaled(big, 1.0), u)
    assert kept.tolist() == [5, 5]
    # V = 65536, the largest row the kernel takes
    full = torch.randn(2, 65536, device="cuda")
    tok, thr, kept = ext.sample_tokens(full, 0.7, 50, 0.9, 7, 0, 0, True)
    u = sample_uniforms(7, 0, 0, 2, 65536, "cuda").cpu().numpy().astype(np.float64)
    sh.assert_valid_draw(tok.cpu().numpy(), thr.cpu().numpy(), sh.scaled(full, 0.7), u)


@pytest.mark.parametrize("seed", [7, 2 ** 40 + 7])
@pytest.mark.parametrize("V", [8, 257, 50257])
def test_uniforms_equal_the_replica(V, seed):
    for row_base in (0, 5, 2 ** 33):
        u = sample_uniforms(seed, 3, row_base, 3, V, "cuda")
        assert u.is_cuda and u.shape == (3, V) and u.dtype == torch.float32
        assert torch.equal(u.cpu(), sample_uniforms_ref(seed, 3, row_base, 3, V))
        n = u.double() * 2 ** 24
        assert (n == n.round()).all() and (n.long() % 2 == 1).all() and (u > 0).all() and (u < 1).all()
    base = sample_uniforms(seed, 3, 5, 3, V, "cuda")
    for other in ((seed, 4, 5), (seed + 2 ** 32, 3, 5), (seed, 3, 6)):
        assert not torch.equal(base, sample_uniforms(*other, 3, V, "cuda"))


@pytest.mark.parametrize("V,B", sh.SHAPES)
def test_top_k_is_exact(V, B):
    sh.check_top_k_exact(V, B, "cuda")


def test_top_k_keeps_ties_with_the_kth():
    sh.check_top_k_ties("cuda")


@pytest.mark.parametrize("V,B", sh.SHAPES)
def test_top_p_sandwich(V, B):
    """tau64(p + d) <= thr <= tau64(p - d) with d = 1e-4, derived: the kernel's masses are fp32 sums of
    at most 64 terms per thread, then a 64-lane tree, then 16 waves in order - within about
    (64 + 6 + 16) * 2^-24 = 5e-6 relative of the true sum, with each exponential good to a few ulp
    where it matters (a term's relative error grows as |s - max| * 2^-24, weighted by a term that
    shrinks as exp(s - max))."""
    sh.check_top_p_sandwich(V, B, "cuda")


def test_top_p_pinned_cases():
    sh.check_top_p_pinned("cuda")


@pytest.mark.parametrize("V,B", sh.SHAPES)
def test_draw_is_the_perturbed_argmax(V, B):
    """eps = 1e-4, derived as in test_sample_tokens_cpu.py.  B = 70 rows of up to 50257 ids: some
    winners have u within 1e-6 of 1, where a fast-math log has no relative accuracy."""
    worst = sh.check_draw(V, B, "cuda")
    print(f"V={V} B={B}: largest float64 score gap of a drawn token = {worst:.3e} (eps {sh.EPS})")


@pytest.mark.parametrize("V,B", [(257, 70), (4099, 3), (50257, 70)])
def test_kernel_against_the_pytorch_path(V, B):
    for dtype, kind, T in sh.CONFIGS:
        x = sh.inputs(V, B, dtype, kind, "cuda")
        s32 = sh.scaled(x, T)
        u = sh.uniforms64(V, B, "cuda")
        for k, p in ((0, 0.0), (50, 0.0), (0, 0.9), (50, 0.9)):
            dev = sh.run(x, T, top_k=k, top_p=p)
            cpu = sh.run(x.cpu(), T, top_k=k, top_p=p)
            sh.assert_valid_draw(dev[0], dev[1], s32, u, ("kernel", dtype, kind, k, p))
            sh.assert_valid_draw(cpu[0], cpu[1], s32, u, ("cpu", dtype, kind, k, p))
            if p == 0.0:
                assert dev[1].tobytes() == cpu[1].tobytes() and np.array_equal(dev[2], cpu[2])
            print(f"V={V} B={B} {dtype} {kind} k={k} p={p}: {(dev[0] == cpu[0]).mean():.3f} of the tokens equal")


def test_batch_independence_and_reproducibility():
    sh.check_batch_independence("cuda")


def test_distribution_chi_squared():
    """The kernel draws the CPU path's bits: see test_sample_tokens_cpu.py for the statistic."""
    stat, bound, n = sh.check_distribution("cuda")
    print(f"chi2 = {stat:.3f} on {n - 1} degrees of freedom, bound {bound}")
    assert n == 4 and stat < bound, (stat, bound)


def test_degenerate_rows():
    sh.check_degenerate("cuda")


# ---- GPT2LMModel.generate(noise_seed=...) on the native model -----------------------------------

@functools.lru_cache(maxsize=None)
def _model(heads):
    torch.manual_seed(0)
    nat = build_model(precision="bf16", num_heads=heads, **TINY).cuda().eval()
    eng = DDPEngine(nat, shadow_dtype=torch.bfloat16)  # attaches the bf16 weight shadows
    return nat, eng


def _prompts(seed=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(1000, 3000, (4, 40), device="cuda", generator=g)
    return ids, torch.tensor([40, 17, 1, 33], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("heads", [4, 2])
def test_generate_with_noise_seed_equals_the_written_out_loop(heads):
    nat, _ = _model(heads)
    ids, lens = _prompts()
    kw = dict(temperature=0.9, top_k=40, top_p=0.95)
    a, na = nat.generate(ids, lens, 24, noise_seed=11, row_base=4, **kw)
    b, nb = nat.generate(ids, lens, 24, noise_seed=11, row_base=4, **kw)
    assert torch.equal(a, b) and torch.equal(na, nb) and na.tolist() == [24] * 4
    assert not torch.equal(a, nat.generate(ids, lens, 24, noise_seed=12, row_base=4, **kw)[0])
    cache = nat.init_cache(4, 64)
    logits = nat.prefill(ids, lens, cache)
    toks = []
    for t in range(24):
        toks.append(sample_tokens(logits, seed=11, step=t, row_base=4, **kw))
        if t < 23:
            logits = nat.decode_step(toks[-1], cache)
    assert torch.equal(a, torch.stack(toks, 1))


@pytest.mark.parametrize("heads", [4, 2])
def test_generate_with_noise_seed_parks_a_row_at_eos(heads):
    nat, _ = _model(heads)
    ids, lens = _prompts()
    kw = dict(temperature=0.9, top_k=40, noise_seed=11)
    free, _ = nat.generate(ids, lens, 16, **kw)
    eos = int(free[0, 2])
    first = free[0].tolist().index(eos)
    toks, new_lens = nat.generate(ids, lens, 16, eos_id=eos, **kw)
    assert toks[0].tolist() == free[0, :first + 1].tolist() + [eos] * (15 - first)
    assert int(new_lens[0]) == first + 1
    for b in (1, 2, 3):
        row = free[b].tolist()
        cut = row.index(eos) + 1 if eos in row else 16
        assert toks[b].tolist() == row[:cut] + [eos] * (16 - cut) and int(new_lens[b]) == cut
