"""Teacher-forced scoring on the GPU: ``GPT2LMModel.score`` (native bf16 forward, csrc/token_stats.hip
on the scored rows) against the fp32 model's full forward, ``generate(return_logprobs=True)`` against
the loop written out, and ``beam_search`` scores against ``score``.

The tiny D = 64 and D = 128 models of tests/test_generate_gpu.py (bf16 weights on the native kernels
next to the same weights in fp32 stock ops).  The rank / top1 test needs targets the fp32 model
separates from their neighbours: the variant with scaled position embeddings of
tests/test_lookahead_gpu.py, whose arg-max moves with the position, scored on its own greedy output."""
import functools

import pytest
import torch

import beam_search_helpers as bsh
import penalty_helpers as ph
from decode_helpers import TINY
from distributed_pipeline_amd.ops.decode import sample_tokens, token_stats
from test_generate_gpu import _models
from test_lookahead_gpu import _models as _scaled_models
from utils.lm_sampling import greedy, sample_next

pytestmark = pytest.mark.gpu

VOCAB = TINY["vocab_size"]
LENS = [2, 5, 64, 65]      # in one batch: L = 65 is padded to 128 on the native path
START = [0, 3, 10, 1]      # ragged; 0 and 1 both mean "from the second token on"


@functools.lru_cache(maxsize=None)
def _case(heads):
    """(ref, nat, ids [4, 128]): random 8-token prompts continued greedily by the fp32 model, so that
    most scored tokens are ones it separates from the rest; columns 65 .. 127 are padding for the
    full forwards (the native attention takes L % 64 == 0; causality hides them)."""
    ref, nat, _ = _scaled_models(heads, 50.0)
    g = torch.Generator(device="cuda").manual_seed(1)
    prompt = torch.randint(1000, 3000, (4, 8), device="cuda", generator=g)
    cont, _ = ref.generate(prompt, torch.full((4,), 8, dtype=torch.int32, device="cuda"), 57, temperature=0)
    ids = torch.cat([prompt, cont, torch.zeros(4, 63, dtype=torch.long, device="cuda")], 1)
    return ref, nat, ids


@functools.lru_cache(maxsize=None)
def _scored(heads):
    """-> (score's result on ids[:, :65], the fp32 logits [4, 64, V], the targets, the native model's
    own -CE [4, 64])."""
    ref, nat, ids = _case(heads)
    res = nat.score(ids[:, :65], torch.tensor(LENS, device="cuda"), start=torch.tensor(START, device="cuda"))
    with torch.no_grad():
        F = ref(ids).float()[:, :64]
        own = -nat(ids, labels=ids).float()[:, :64]
    return res, F, ids[:, 1:65], own


def _mask():
    p = torch.arange(1, 65, device="cuda").view(1, 64)
    start, lens = torch.tensor(START, device="cuda").view(4, 1), torch.tensor(LENS, device="cuda").view(4, 1)
    return (p >= start.clamp(min=1)) & (p < lens)


@pytest.mark.parametrize("heads", [4, 2])
def test_logp_matches_the_fp32_forward(heads):
    """Bound: twice the largest error, over the same positions and against the same fp32 reference, of
    the existing native ``-model(input_ids, labels=input_ids)`` (the rule of test_generate_gpu.py: the
    factor 2 allows for another summation order).  Measured on the MI355X: 7.13e-03 against 4.65e-03
    (D = 64) and 6.73e-03 against 3.97e-03 (D = 128)."""
    res, F, tgt, own = _scored(heads)
    mask = _mask()
    assert torch.equal(res["mask"], mask) and mask.sum(1).tolist() == [1, 2, 54, 64]
    want = torch.log_softmax(F, -1).gather(2, tgt.unsqueeze(-1)).squeeze(-1)
    e_score = (res["logp"] - want)[mask].abs().max().item()
    e_own = (own - want)[mask].abs().max().item()
    print(f"heads={heads}: score logp max |err| = {e_score:.4e}, native -CE max |err| = {e_own:.4e}")
    assert e_score <= 2 * e_own, (e_score, e_own)
    ent = -(torch.softmax(F, -1) * torch.log_softmax(F, -1)).sum(-1)
    print(f"heads={heads}: entropy max |err| = {(res['entropy'] - ent)[mask].abs().max().item():.4e}")


@pytest.mark.parametrize("heads", [4, 2])
def test_rank_and_top1_equal_the_fp32_models_where_it_separates_them(heads):
    res, F, tgt, own = _scored(heads)
    mask = _mask()
    want = torch.log_softmax(F, -1).gather(2, tgt.unsqueeze(-1)).squeeze(-1)
    e = (own - want)[mask].abs().max().item()
    top2 = F.topk(2, -1).values
    st = F.gather(2, tgt.unsqueeze(-1))
    around = (F - st).abs().scatter(2, tgt.unsqueeze(-1), float("inf")).amin(-1)
    sure = mask & (top2[..., 0] - top2[..., 1] > 4 * e) & (around > 4 * e)
    print(f"heads={heads}: {int(sure.sum())} of {int(mask.sum())} scored positions are separated by more than 4 x {e:.3e}")
    assert 2 * int(sure.sum()) >= int(mask.sum())  # the precondition
    ids_v = torch.arange(VOCAB, device="cuda").view(1, 1, VOCAB)
    rank = (F > st).sum(-1) + ((F == st) & (ids_v < tgt.unsqueeze(-1))).sum(-1)
    assert torch.equal(res["rank"][sure].long(), rank[sure])
    assert torch.equal(res["top1"][sure], greedy(F)[sure])
    assert len(set(res["top1"][sure].tolist())) > 20  # not one token repeated
    m = res["mask"]
    assert torch.equal(res["rank"][m] == 0, res["top1"][m] == tgt[m])


@pytest.mark.parametrize("heads", [4, 2])
def test_outside_the_mask_nothing_is_looked_at(heads):
    _, nat, ids = _case(heads)
    res = _scored(heads)[0]
    mask = _mask()
    assert (res["logp"][~mask] == 0).all() and (res["rank"][~mask] == -1).all()
    assert (res["entropy"][~mask] == 0).all() and (res["top1"][~mask] == -1).all()
    assert res["logp"].dtype == res["entropy"].dtype == torch.float32 and res["rank"].dtype == torch.int32
    assert res["top1"].dtype == torch.int64 and all(v.shape == (4, 64) for v in res.values())
    poisoned = ids[:, :65].clone()
    for b, n in enumerate(LENS):
        poisoned[b, n:] = -(2 ** 40) if b % 2 else VOCAB + 12345  # no such embedding row
    got = nat.score(poisoned, LENS, start=START)
    again = nat.score(poisoned, LENS, start=START)
    for k in res:
        assert torch.equal(got[k], res[k]) and torch.equal(again[k], res[k]), k  # bit for bit
    # nothing to score: no launch, shaped fill values
    none = nat.score(ids[:, :65], [1, 0, 1, 1])
    assert not none["mask"].any() and (none["rank"] == -1).all() and none["logp"].is_cuda


def _recording(pick, record):
    def run(logits, t):
        tok = pick(logits, t)
        record.append(token_stats(logits, tok)[0])
        return tok
    return run


@pytest.mark.parametrize("heads", [4, 2])
def test_generate_logprobs_are_token_stats_on_the_loops_logits(heads):
    """Tokens and lengths equal those of the call without the keyword; ``logprobs`` equals, bit for
    bit, ``token_stats`` on the processed logits of the loop written out (tests/penalty_helpers.py),
    with zeros behind a finished row."""
    _, nat, _ = _models(heads)
    ids, lens = ph.gen_prompts("cuda", VOCAB)
    N = ph.N_NEW
    free, _ = nat.generate(ids, lens, N, temperature=0, **ph.PENALTIES)
    eos = int(free[0, 8])

    def gen(seed):
        return torch.Generator(device="cuda").manual_seed(seed)

    cases = [
        (dict(temperature=0), lambda: lambda x, t: greedy(x), {}),
        (dict(temperature=0, eos_id=eos, min_new_tokens=3, **ph.PENALTIES), lambda: lambda x, t: greedy(x),
         dict(eos_id=eos, min_new_tokens=3, **ph.PENALTIES)),
        (dict(temperature=0.9, top_k=20, **ph.PENALTIES),
         lambda: (lambda g: lambda x, t: sample_next(x, 0.9, 20, 0.0, g))(gen(5)), dict(**ph.PENALTIES)),
        (dict(temperature=0.8, top_k=50, top_p=0.9, noise_seed=77, row_base=3, eos_id=eos),
         lambda: lambda x, t: sample_tokens(x, temperature=0.8, top_k=50, top_p=0.9, seed=77, step=t, row_base=3),
         dict(eos_id=eos)),
    ]
    stopped_early = False
    for kw, pick, loop_kw in cases:
        extra = {"generator": gen(5)} if "top_k" in kw and "noise_seed" not in kw else {}
        plain = nat.generate(ids, lens, N, **kw, **extra)
        extra = {"generator": gen(5)} if extra else {}
        toks, new_lens, lp = nat.generate(ids, lens, N, return_logprobs=True, **kw, **extra)
        assert len(plain) == 2 and torch.equal(plain[0], toks) and torch.equal(plain[1], new_lens)
        record = []
        w_toks, w_lens = ph.written_out_generate(nat, ids, lens, N, _recording(pick(), record), **loop_kw)
        assert torch.equal(w_toks, toks) and torch.equal(w_lens, new_lens)
        want = torch.stack(record, 1)
        live = torch.arange(N, device="cuda").view(1, N) < new_lens.view(-1, 1)
        want = torch.where(live, want, 0.0)
        assert lp.dtype == torch.float32 and lp.shape == (4, N)
        assert lp.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        assert (lp[live] <= 0).all() and (lp[~live] == 0).all()
        stopped_early = stopped_early or bool((new_lens < N).any())
    assert stopped_early, "eos_id must end some row early"


def _beam_gap(nat, ids, lens, W, eos):
    """Largest |beam_search score - float64 sum of score()'s logp over the beam| over all beams."""
    toks, new_lens, scores = nat.beam_search(ids, lens, bsh.T, num_beams=W, eos_id=eos)
    B, Lp = ids.shape
    seq = torch.zeros(B * W, Lp + bsh.T, dtype=torch.long, device="cuda")
    plen = lens.long().repeat_interleave(W)
    n = new_lens.view(-1)
    for r in range(B * W):
        seq[r, :plen[r]] = ids[r // W, :plen[r]]
        seq[r, plen[r]:plen[r] + n[r]] = toks.view(B * W, -1)[r, :n[r]]
    res = nat.score(seq, plen + n, start=plen)
    assert torch.equal(res["mask"].sum(1), n)
    forced = res["logp"].double().sum(1)
    exists = scores.view(-1) > float("-inf")
    return (scores.view(-1).double() - forced)[exists].abs().max().item(), new_lens


def test_beam_search_scores_are_the_sums_of_score():
    """Without penalties; the bound of the existing teacher-forced beam test: four times the greedy
    path's own difference in the same run (one beam, with and without ``eos_id``).  Measured on the
    MI355X: 3.12e-02 for the beams against 3.13e-02 for the greedy path - here both are the distance
    between the bf16 full forward of ``score`` and the decode path that produced the scores, not
    rounding of the sums."""
    nat = _models(4)[1]
    ids, lens = bsh.prompts("cuda", VOCAB)
    eos = bsh.pick_eos(nat, ids, lens, 2)
    d_greedy = max(_beam_gap(nat, ids, lens, 1, e)[0] for e in (eos, None))
    d_beam, new_lens = _beam_gap(nat, ids, lens, 2, eos)
    print(f"beam_search (W = 2) max |score - score().logp.sum()| = {d_beam:.3e}, greedy path {d_greedy:.3e}")
    assert bool((new_lens < bsh.T).any()) and bool((new_lens == bsh.T).any())
    assert d_beam <= 4 * d_greedy, (d_beam, d_greedy)
