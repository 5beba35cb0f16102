"""GPT-2 generation on the GPU: ``prefill`` / ``decode_step`` (csrc/attn_decode.hip in every layer)
against the fp32 model's full forward, greedy ``generate`` and its EOS parking.

Tiny GPT-2 (hidden 256, 2 layers, vocabulary 3000, 256 positions, no dropout) with 4 heads
(D = 64) and 2 heads (D = 128): bf16 weights on the native kernels next to the same weights in
fp32 stock ops, built as ``test_model_gpu.py::test_gpt2_native_bf16_matches_fp32`` builds them."""
import functools

import pytest
import torch

from decode_helpers import PATTERN, TINY, bits, teacher_forced
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.parallel.ddp import DDPEngine
from utils import lm_sampling as lms

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _models(heads):
    torch.manual_seed(0)
    ref = build_model(precision="fp32", num_heads=heads, **TINY).cuda().eval()
    nat = build_model(precision="bf16", num_heads=heads, **TINY).cuda().eval()
    nat.load_state_dict(ref.state_dict())
    eng = DDPEngine(nat, shadow_dtype=torch.bfloat16)  # attaches the bf16 weight shadows
    return ref, nat, eng


@pytest.mark.parametrize("heads", [4, 2])
def test_teacher_forced_logits_match_the_fp32_forward(heads):
    """Largest absolute logit error of the cached path <= 2 x that of the existing native full
    forward, both against the fp32 model's full forward over the same (row, position) set: the
    factor 2 allows for the summation order of a different attention kernel."""
    ref, nat, _ = _models(heads)
    ids = torch.randint(1000, 3000, (4, 96), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    plens = [1, 5, 64, 65]
    with torch.no_grad():
        want = ref(ids).float()
        full = nat(ids).float()
    got, _ = teacher_forced(nat, ids, plens, 65)
    assert len(got) == sum(96 - p + 1 for p in plens)
    e_cached = max((got[(b, p)] - want[b, p]).abs().max().item() for (b, p) in got)
    e_full = max((full[b, p] - want[b, p]).abs().max().item() for (b, p) in got)
    print(f"heads={heads}: cached path max |err| = {e_cached:.4e}, native full forward max |err| = {e_full:.4e}")
    assert e_cached <= 2 * e_full, (e_cached, e_full)


def _prompts(seed=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(1000, 3000, (4, 40), device="cuda", generator=g)
    return ids, torch.tensor([40, 17, 1, 33], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("heads", [4, 2])
def test_greedy_generate_is_reproducible_and_equals_the_written_out_loop(heads):
    _, nat, _ = _models(heads)
    ids, lens = _prompts()
    a, na = nat.generate(ids, lens, 24, temperature=0)
    b, nb = nat.generate(ids, lens, 24, temperature=0)
    assert torch.equal(a, b) and torch.equal(na, nb) and na.tolist() == [24] * 4
    cache = nat.init_cache(4, 64)
    logits = nat.prefill(ids, lens, cache)
    toks = []
    for t in range(24):
        toks.append(lms.greedy(logits))
        if t < 23:
            logits = nat.decode_step(toks[-1], cache)
    assert torch.equal(a, torch.stack(toks, 1))
    assert cache.lens.tolist() == [int(n) + 23 for n in lens.tolist()]


@pytest.mark.parametrize("heads", [4, 2])
def test_eos_parks_a_row(heads):
    _, nat, _ = _models(heads)
    ids, lens = _prompts()
    free, _ = nat.generate(ids, lens, 16, temperature=0)
    eos = int(free[0, 0])

    cache = nat.init_cache(4, 56)
    cache.buf.view(torch.int16).fill_(PATTERN)
    toks, new_lens = nat.generate(ids, lens, 16, temperature=0, eos_id=eos, cache=cache)
    assert toks[0].tolist() == [eos] * 16 and int(new_lens[0]) == 1
    assert int(cache.lens[0]) == -1
    # row 0 never ran a decode step: beyond its 40 prompt rows the cache holds the pattern
    assert (bits(cache.buf[:, :, 0, :, 40:]) == PATTERN).all()
    assert not (bits(cache.buf[:, :, 0, :, :40]) == PATTERN).all()
    for b in (1, 2, 3):
        row = free[b].tolist()
        if eos in row:  # it stops there too
            cut = row.index(eos) + 1
            assert toks[b].tolist() == row[:cut] + [eos] * (16 - cut) and int(new_lens[b]) == cut
        else:
            assert toks[b].tolist() == row and int(new_lens[b]) == 16
            # 15 decode steps behind its prompt, and nothing behind those
            n = int(lens[b]) + 15
            assert int(cache.lens[b]) == n
            assert (bits(cache.buf[:, :, b, :, n:]) == PATTERN).all()
