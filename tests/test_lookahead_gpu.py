"""Lookahead decoding on the GPU: ``decode_block`` (csrc/attn_decode_block.hip in every layer)
against the fp32 model's full forward, ``generate_lookahead`` against the loop written out row by
row, and every emitted token against the fp32 model.

The tiny GPT-2 models of test_generate_gpu.py.  bf16 logits of a random-init model have arg-max
margins within the rounding of the kernels, so equality with ``generate`` is not asserted here (it
is on the CPU, in fp32): each emitted token must instead be within the native path's own error of
the fp32 model's best."""
import functools

import pytest
import torch

from decode_block_helpers import lookahead_loop, oracle_draft
from decode_helpers import PATTERN, TINY, bits
from distributed_pipeline_amd.models import build_model
from distributed_pipeline_amd.parallel.ddp import DDPEngine

pytestmark = pytest.mark.gpu

N = 24
VOCAB = TINY["vocab_size"]


# A random-init model with a tied head repeats its last token: every guess is right and no id is new
# inside a block.  The second variant has its position embeddings scaled up, so that the arg-max
# moves with the position: guesses get rejected and rows can end in the middle of a block.
WPE_SCALES = (1.0, 50.0)


@functools.lru_cache(maxsize=None)
def _models(heads, wpe_scale=1.0):
    torch.manual_seed(0)
    ref = build_model(precision="fp32", num_heads=heads, **TINY).cuda().eval()
    with torch.no_grad():
        ref.wpe.weight.mul_(wpe_scale)
    nat = build_model(precision="bf16", num_heads=heads, **TINY).cuda().eval()
    nat.load_state_dict(ref.state_dict())
    eng = DDPEngine(nat, shadow_dtype=torch.bfloat16)  # attaches the bf16 weight shadows
    return ref, nat, eng


@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("heads", [4, 2])
def test_teacher_forced_block_logits_match_the_fp32_forward(heads, T):
    """Largest absolute logit error of ``decode_block`` <= 2 x that of the native full forward, both
    against the fp32 model's full forward over the same (row, position) set.  In every block only
    the first a_b tokens (ragged, 1 .. T) are the row's true ones and ``cache.lens`` advances by a_b,
    so a key of a rejected guess that reached a later logit would show."""
    ref, nat, _ = _models(heads)
    L, plens, Lp = 96, [1, 5, 64, 65], 65
    ids = torch.randint(1000, 3000, (4, L), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with torch.no_grad():
        want = ref(ids).float()
        full = nat(ids).float()
    lens = torch.tensor(plens, dtype=torch.int32, device="cuda")
    prompt = ids[:, :Lp].clone()
    prompt[torch.arange(Lp, device="cuda").view(1, Lp) >= lens.view(4, 1)] = 0
    cache = nat.init_cache(4, L, "cuda")
    got = {}
    logits = nat.prefill(prompt, lens, cache)
    for b in range(4):
        got[(b, plens[b] - 1)] = logits[b].float()
    pos, it = list(plens), 0
    while min(pos) < L:
        a = [min(1 + (it + b) % T, L - pos[b]) for b in range(4)]
        block = torch.zeros(4, T, dtype=torch.long, device="cuda")
        for b in range(4):
            for j in range(T):
                true = int(ids[b, min(pos[b] + j, L - 1)])
                block[b, j] = true if j < a[b] else 1000 + (true - 1000 + 7 + j) % 2000
        cache.lens.copy_(torch.tensor(pos, dtype=torch.int32))  # pos == L: an inactive row
        logits = nat.decode_block(block, cache)
        assert logits.shape == (4, T, VOCAB) and cache.lens.tolist() == pos  # not advanced
        for b in range(4):
            for j in range(a[b]):
                got[(b, pos[b] + j)] = logits[b, j].float()
            pos[b] += a[b]
        it += 1
    assert len(got) == sum(L - p + 1 for p in plens)
    e_block = max((got[(b, p)] - want[b, p]).abs().max().item() for (b, p) in got)
    e_full = max((full[b, p] - want[b, p]).abs().max().item() for (b, p) in got)
    print(f"heads={heads} T={T}: decode_block max |err| = {e_block:.4e}, native full forward max |err| = {e_full:.4e}")
    assert e_block <= 2 * e_full, (e_block, e_full)


def _prompts(seed=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(1000, 3000, (4, 40), device="cuda", generator=g)
    return ids, torch.tensor([40, 17, 1, 33], dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def _lookup_run(heads, T, wpe_scale=1.0):
    """``generate_lookahead`` with lookup drafts, once per case -> (tokens, new_lens, stats, cache)."""
    _, nat, _ = _models(heads, wpe_scale)
    ids, lens = _prompts()
    cache = nat.init_cache(4, 40 + N)
    toks, new_lens, stats = nat.generate_lookahead(ids, lens, N, lookahead=T, ngram=1, cache=cache, return_stats=True)
    return toks, new_lens, stats, cache


@pytest.mark.parametrize("wpe_scale", WPE_SCALES)
@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("heads", [4, 2])
def test_lookup_drafts_equal_the_written_out_loop(heads, T, wpe_scale):
    _, nat, _ = _models(heads, wpe_scale)
    ids, lens = _prompts()
    toks, new_lens, stats, cache = _lookup_run(heads, T, wpe_scale)
    t2, l2, s2, c2 = lookahead_loop(nat, ids, lens, N, T, ngram=1)
    print(f"heads={heads} T={T} wpe x{wpe_scale}: {stats}")
    assert torch.equal(toks, t2) and new_lens.tolist() == l2 == [N] * 4 and stats == s2
    assert cache.lens.tolist() == c2.lens.tolist() == [int(p) + N - 1 for p in lens.tolist()]
    # a second run: the same bits
    again, lens_again = nat.generate_lookahead(ids, lens, N, lookahead=T, ngram=1)
    assert torch.equal(again, toks) and torch.equal(lens_again, new_lens)


@pytest.mark.parametrize("wpe_scale", WPE_SCALES)
@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("heads", [4, 2])
def test_oracle_drafts_and_corrupted_ones(heads, T, wpe_scale):
    """The continuation of the lookup run handed back as the guesses: every guess is accepted and
    the call count is exact; with wrong ids at given positions, the accepted counts are the ones the
    corruption dictates.  Both against the written-out loop too."""
    _, nat, _ = _models(heads, wpe_scale)
    ids, lens = _prompts()
    plens = lens.tolist()
    cont = _lookup_run(heads, T, wpe_scale)[0]
    draft = oracle_draft(cont, plens, VOCAB)
    toks, new_lens, stats = nat.generate_lookahead(ids, lens, N, lookahead=T, draft=draft, return_stats=True)
    assert torch.equal(toks, cont) and new_lens.tolist() == [N] * 4
    assert stats["model_calls"] == -(-(N - 1) // T) and stats["accepted"] == stats["proposed"]
    t2, l2, s2, _ = lookahead_loop(nat, ids, lens, N, T, draft=draft)
    assert torch.equal(toks, t2) and new_lens.tolist() == l2 and stats == s2

    corrupt = torch.zeros(4, N, dtype=torch.bool, device="cuda")
    for b, at in enumerate(([3, 17], [1, 2, 20], [N - 1], [10, 11, 12, 13])):
        corrupt[b, at] = True
    draft = oracle_draft(cont, plens, VOCAB, corrupt)
    cache = nat.init_cache(4, 40 + N)
    toks, new_lens, stats = nat.generate_lookahead(ids, lens, N, lookahead=T, draft=draft, cache=cache,
                                                   return_stats=True)
    t2, l2, s2, c2 = lookahead_loop(nat, ids, lens, N, T, draft=draft)
    assert torch.equal(toks, t2) and new_lens.tolist() == l2 and stats == s2
    assert cache.lens.tolist() == c2.lens.tolist()
    assert torch.equal(toks, cont)  # the picks agree with the continuation that was handed in, so:
    acc, bad = 0, corrupt.tolist()
    for b in range(4):
        at = 1
        while at < N:
            c = min(T, N - at)  # the block: output position at - 1 and guesses for at .. at + c - 2
            a = 0
            while a + 1 < c and not bad[b][at + a]:
                a += 1
            acc += a
            at += a + 1
    assert stats["accepted"] == acc


@pytest.mark.parametrize("wpe_scale", WPE_SCALES)
@pytest.mark.parametrize("heads", [4, 2])
def test_every_emitted_token_is_within_the_native_error_of_the_fp32_best(heads, wpe_scale):
    """With F the fp32 model's full forward on prompt + output: max F_t - F_t[y_t] <= 4 e_full, where
    e_full is the native full forward's error against F on those sequences - 2 x the factor 2 of the
    logit test, once for the winner and once for the runner-up."""
    ref, nat, _ = _models(heads, wpe_scale)
    ids, lens = _prompts()
    plain, _ = nat.generate(ids, lens, N, temperature=0)
    for T in (2, 4, 8):
        toks = _lookup_run(heads, T, wpe_scale)[0]
        worst, e_full = 0.0, 0.0
        for b, p in enumerate(lens.tolist()):
            seq = torch.cat([ids[b, :p], toks[b]])[None]
            with torch.no_grad():
                F = ref(seq).float()[0, p - 1:p + N - 1]
                e_full = max(e_full, (nat(torch.nn.functional.pad(seq, (0, -seq.shape[1] % 64))).float()[0, p - 1:p + N - 1]
                                      - F).abs().max().item())
            worst = max(worst, (F.amax(-1) - F.gather(1, toks[b].view(N, 1)).view(N)).max().item())
        same = sum(torch.equal(toks[b], plain[b]) for b in range(4))
        print(f"heads={heads} T={T} wpe x{wpe_scale}: largest fp32 gap of an emitted token {worst:.4e}, e_full {e_full:.4e}; "
              f"{same} of 4 rows equal generate's")
        assert worst <= 4 * e_full, (worst, e_full)


@pytest.mark.parametrize("heads", [4, 2])
def test_eos_inside_an_accepted_block_and_nothing_written_beyond(heads):
    _, nat, _ = _models(heads, WPE_SCALES[1])
    ids, lens = _prompts()
    plens = lens.tolist()
    T = 8
    cont = _lookup_run(heads, T, WPE_SCALES[1])[0]
    # with every guess accepted, output positions 1 .. 8 come from one block: an id that some row
    # emits there for the first time ends that row inside the block
    rows = cont.tolist()
    inside = [(b, i) for i in (3, 2, 4, 5, 1, 6, 7) for b in range(4) if rows[b][i] not in rows[b][:i]]
    assert inside, rows
    eos = rows[inside[0][0]][inside[0][1]]
    cache = nat.init_cache(4, 80)
    cache.buf.view(torch.int16).fill_(PATTERN)
    toks, new_lens = nat.generate_lookahead(ids, lens, N, lookahead=T, eos_id=eos, cache=cache,
                                            draft=oracle_draft(cont, plens, VOCAB))
    for b in range(4):
        row = cont[b].tolist()
        cut = row.index(eos) + 1 if eos in row else N
        assert toks[b].tolist() == row[:cut] + [eos] * (N - cut) and int(new_lens[b]) == cut
        run = plens[b] + cut - 1  # positions run: the last emitted token was not
        assert int(cache.lens[b]) == (-1 if eos in row else run)
        # guesses are stored too, so up to T - 1 rows behind the positions run - and nothing beyond
        assert (bits(cache.buf[:, :, b, :, run + T - 1:]) == PATTERN).all()
        assert not (bits(cache.buf[:, :, b, :, :run]) == PATTERN).all(-1).any()
