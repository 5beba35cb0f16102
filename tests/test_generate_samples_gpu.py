"""``generate_samples`` and ``decode_step`` over a ``GroupKVCache`` (K-M28 in every layer), test_generate_gpu.py's models."""
import pytest
import torch

from decode_helpers import PATTERN, bits
from distributed_pipeline_amd.ops.decode import sample_tokens
from test_generate_gpu import _models, _prompts

pytestmark = pytest.mark.gpu
G = 3


@pytest.mark.parametrize("heads", [4, 2])
def test_teacher_forced_logits_match_the_fp32_forward(heads):
    """test_generate_gpu.py's rule, for one prefill per prompt and six steps on G = 3 given continuations of each."""
    ref, nat, _ = _models(heads)
    plens, steps, dev = [1, 5, 64, 65], 6, "cuda"
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = torch.tensor(plens, dtype=torch.int32, device=dev)
    prompt = torch.randint(1000, 3000, (4, 65), device=dev, generator=gen)
    prompt[torch.arange(65, device=dev).view(1, 65) >= lens.view(4, 1)] = 0
    cont = torch.randint(1000, 3000, (4 * G, steps), device=dev, generator=gen)
    ids = torch.zeros(4 * G, 128, dtype=torch.long, device=dev)  # row r: its prompt, its continuation, padding
    rows, n = torch.arange(4 * G, device=dev), lens.long().repeat_interleave(G)
    ids[:, :65] = prompt.repeat_interleave(G, 0)
    ids[rows.view(-1, 1), n.view(-1, 1) + torch.arange(steps, device=dev)] = cont
    with torch.no_grad():
        want, full = ref(ids).float(), nat(ids).float()
    cache = nat.init_group_cache(4, G, 65, steps)
    got = [nat.prefill(prompt, lens, cache.prefix).float().repeat_interleave(G, 0)]
    got += [nat.decode_step(cont[:, t], cache).float() for t in range(steps)]
    at = [n - 1 + t for t in range(steps + 1)]
    e_cached = max((g - want[rows, p]).abs().max().item() for g, p in zip(got, at))
    e_full = max((full[rows, p] - want[rows, p]).abs().max().item() for p in at)
    print(f"heads={heads}: grouped path max |err| = {e_cached:.4e}, native full forward max |err| = {e_full:.4e}")
    assert e_cached <= 2 * e_full, (e_cached, e_full)
    assert cache.suffix.lens.tolist() == [steps] * (4 * G) and cache.prefix.lens.tolist() == plens


@pytest.mark.parametrize("heads", [4, 2])
def test_generate_samples_equals_the_written_out_loop_and_parks_rows(heads):
    nat, (ids, lens) = _models(heads)[1], _prompts()
    kw = dict(num_samples=G, temperature=0.9, top_k=40, noise_seed=11, row_base=5)
    a, b = (nat.generate_samples(ids, lens, 12, **kw) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].tolist() == [[12] * G] * 4
    cache = nat.init_group_cache(4, G, 40, 12)
    logits, toks = nat.prefill(ids, lens, cache.prefix).repeat_interleave(G, 0), []
    for t in range(12):
        toks.append(sample_tokens(logits, temperature=0.9, top_k=40, seed=11, step=t, row_base=5))
        logits = nat.decode_step(toks[-1], cache)
    assert torch.equal(a[0].view(-1, 12), torch.stack(toks, 1))

    eos = int(a[0][0, 1, 2])  # sample (0, 1) ends at its third token
    cache = nat.init_group_cache(4, G, 40, 12)
    cache.suffix.buf.view(torch.int16).fill_(PATTERN)
    plain = nat.init_cache(4, 40)
    nat.prefill(ids, lens, plain)
    cut, cut_lens = nat.generate_samples(ids, lens, 12, eos_id=eos, cache=cache, **kw)
    assert torch.equal(bits(cache.prefix.buf), bits(plain.buf))  # the prefix is what prefill left, bit for bit
    for r, (row, free) in enumerate(zip(cut.view(-1, 12).tolist(), a[0].view(-1, 12).tolist())):
        stop = free.index(eos) + 1 if eos in free else 12
        assert row == free[:stop] + [eos] * (12 - stop) and int(cut_lens.view(-1)[r]) == stop
        kept = stop - 1  # decode steps the row ran: one suffix key each, the pattern behind them
        assert int(cache.suffix.lens[r]) == (-1 if eos in free else 11)
        assert (bits(cache.suffix.buf[:, :, r, :, kept:]) == PATTERN).all()
        assert kept == 0 or not (bits(cache.suffix.buf[:, :, r, :, :kept]) == PATTERN).all()
