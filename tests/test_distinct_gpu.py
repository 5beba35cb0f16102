"""The distinct n-gram kernel (csrc/ngram_distinct.hip) through ``ops.text.ngram_distinct`` against
the set oracle of utils/diversity.py, exactly: shapes on both sides of the wave and of the kernel's
limits, planted first occurrences, id dtypes, strides, zero lengths, poisoned tails; and
``dist_n_batch`` / ``div_n_batch`` on the device."""
import pytest
import torch

from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.text import ngram_distinct
from utils.diversity import dist_n, dist_n_batch, distinct_ngrams, div_n, div_n_batch

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (G, K, L, vocabulary); the last: the limits themselves
SHAPES = [(3, 2, 1, 3), (5, 3, 7, 3), (4, 10, 64, 4), (2, 16, 130, 5), (70, 4, 33, 3), (3, 1, 9, 2),
          (1, 16, 256, 2)]
_ORACLE = {}


def set_counts(seqs):
    """[K + 1][4]: the distinct n-gram counts of the id lists ``seqs`` and of their union."""
    rows = [[distinct_ngrams(s, n) for n in range(1, 5)] for s in seqs]
    rows.append([len(set().union(*[{tuple(s[i:i + n]) for i in range(len(s) - n + 1)} for s in seqs]))
                 for n in range(1, 5)])
    return rows


def oracle(tokens, lens):
    """(want int32 [G, K + 1, 4], the id lists) of CPU ``tokens`` / ``lens`` (lens inside [0, L])."""
    G, K, _ = tokens.shape
    seqs = [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(G)]
    want = torch.tensor([set_counts(grp) for grp in seqs], dtype=torch.int32).reshape(G, K + 1, 4)
    return want, seqs


def case(G, K, L, vocab):
    """(tokens int64 [G, K, L], lens [G, K], oracle int32 [G, K + 1, 4], lists) on the CPU, computed
    once.  The lengths 0, 1, 2, 3 and L occur; the tails hold in-range ids that also occur inside."""
    key = (G, K, L, vocab)
    if key not in _ORACLE:
        g = torch.Generator().manual_seed(G * 1000 + K * 100 + L)
        tokens = torch.randint(0, vocab, (G, K, L), generator=g)
        lens = torch.randint(0, L + 1, (G, K), generator=g)
        flat = lens.view(-1)
        for at, n in enumerate((0, 1, 2, 3, L)):
            flat[(at * 7) % flat.numel()] = min(n, L)
        _ORACLE[key] = (tokens, lens) + oracle(tokens, lens)
    return _ORACLE[key]


@pytest.fixture()
def ext_calls(monkeypatch):
    """Records, per ``ext.ngram_distinct`` call, whether the kernel served it (a tensor came back)."""
    ext = get_ext(required=True)
    calls = []
    real = ext.ngram_distinct

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(ext, "ngram_distinct", spy)
    return calls


def check_invariants(d, lens):
    """What holds for every input: d on the CPU [G, K + 1, 4], lens [G, K] inside [0, L]."""
    K = lens.shape[1]
    n = torch.arange(1, 5).view(1, 1, 4)
    per, uni = d[:, :K].long(), d[:, K].long()
    assert bool((per <= (lens.unsqueeze(-1) - n + 1).clamp_min(0)).all())
    assert bool((per.max(1).values <= uni).all()) and bool((uni <= per.sum(1)).all())
    if K == 1:
        assert torch.equal(d[:, 1], d[:, 0])


@pytest.mark.parametrize("G,K,L,vocab", SHAPES)
def test_kernel_against_the_set_oracle(ext_calls, G, K, L, vocab):
    tokens, lens, want, _ = case(G, K, L, vocab)
    d = ngram_distinct(tokens.to(DEV), lens.to(DEV))
    assert d.dtype == torch.int32 and d.shape == (G, K + 1, 4) and d.is_cuda
    assert torch.equal(d.cpu(), want)
    check_invariants(d.cpu(), lens)
    # bitwise reproducible
    assert torch.equal(ngram_distinct(tokens.to(DEV), lens.to(DEV)), d)
    # zero lengths everywhere: nothing counts, whatever the ids
    assert int(ngram_distinct(tokens.to(DEV), torch.zeros_like(lens).to(DEV)).abs().sum()) == 0
    assert ext_calls == [True, True, True]


def test_ids_up_to_the_top_of_the_range(ext_calls):
    g = torch.Generator().manual_seed(31)
    G, K, L = 6, 5, 70
    tokens = torch.randint(0, 2 ** 31, (G, K, L), generator=g)
    tokens[0, 0, :4] = 2 ** 31 - 1
    tokens[0, 1, :3] = torch.tensor([2 ** 31 - 1, 0, 2 ** 31 - 1])
    tokens[1, 2, :40] = tokens[1, 0, 10:50]  # a long shared run among nearly distinct ids
    lens = torch.randint(4, L + 1, (G, K), generator=g)
    lens[1, 0], lens[1, 2] = L, 45
    want, _ = oracle(tokens, lens)
    assert int(want[0, 0, 0]) < int(lens[0, 0]) and int(want[1, K, 3]) < int(want[1, :K, 3].sum())
    for t in (tokens, tokens.to(torch.int32)):
        d = ngram_distinct(t.to(DEV), lens.to(DEV))
        assert torch.equal(d.cpu(), want)
        check_invariants(d.cpu(), lens)
    assert ext_calls == [True, True]


@pytest.mark.parametrize("G,K,L,vocab", [(5, 3, 7, 3), (4, 10, 64, 4), (2, 16, 130, 5), (70, 4, 33, 3)])
def test_order_independence(ext_calls, G, K, L, vocab):
    tokens, lens, want, _ = case(G, K, L, vocab)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    assert not torch.equal(perm, torch.arange(K))
    d = ngram_distinct(tokens[:, perm].to(DEV), lens[:, perm].to(DEV)).cpu()
    assert torch.equal(d[:, :K], want[:, perm]) and torch.equal(d[:, K], want[:, K])
    rev = ngram_distinct(tokens.flip(1).to(DEV), lens.flip(1).to(DEV)).cpu()
    assert torch.equal(rev[:, :K], want[:, :K].flip(1)) and torch.equal(rev[:, K], want[:, K])
    assert ext_calls == [True, True]


def run_planted(tokens, lens):
    want, seqs = oracle(tokens, lens)
    d = ngram_distinct(tokens.to(DEV), lens.to(DEV)).cpu()
    assert torch.equal(d, want)
    check_invariants(d, lens)
    return d, seqs


def test_planted_4gram_across_the_chunk_edge(ext_calls):
    # every id occurs once, so every n-gram is new - except the planted 4-gram of sequence 1, positions
    # start .. start + 3 (across the edge between its position chunks 0 and 1), which sequence 0 holds
    # only at positions start + 64 .. start + 67, in its chunks 1 and 2
    for start in (61, 62, 63, 64):
        L = 140
        tokens = torch.arange(2 * L).view(1, 2, L) + 10
        lens = torch.tensor([[L, 70]])
        tokens[0, 0, start + 64:start + 68] = torch.tensor([1, 2, 3, 4])
        tokens[0, 1, start:start + 4] = torch.tensor([1, 2, 3, 4])
        d, _ = run_planted(tokens, lens)
        assert d[0, 0].tolist() == [L, L - 1, L - 2, L - 3] and d[0, 1].tolist() == [70, 69, 68, 67]
        assert d[0, 2].tolist() == [L + 70 - 4, L - 1 + 69 - 3, L - 2 + 68 - 2, L - 3 + 67 - 1]
    assert ext_calls == [True] * 4


def test_planted_copy_of_sequence_0_adds_nothing(ext_calls):
    tokens, lens, _, _ = case(4, 10, 64, 4)
    tokens, lens = tokens.clone(), lens.clone()
    lens[:, 0] = torch.tensor([64, 30, 5, 3])
    for k in (4, 9):
        tokens[:, k] = 3 - tokens[:, 0]  # other ids beyond the length ...
        for g in range(4):
            tokens[g, k, :int(lens[g, 0])] = tokens[g, 0, :int(lens[g, 0])]  # ... the same inside it
        lens[:, k] = lens[:, 0]
    d, _ = run_planted(tokens, lens)
    assert torch.equal(d[:, 4], d[:, 0]) and torch.equal(d[:, 9], d[:, 0])
    keep = [k for k in range(10) if k not in (4, 9)]
    without, _ = run_planted(tokens[:, keep].contiguous(), lens[:, keep].contiguous())
    assert torch.equal(without[:, 8], d[:, 10])
    assert ext_calls == [True, True]


def test_planted_length_3_has_no_4gram(ext_calls):
    # sequence 0 stops after [1, 2, 3]; its tail goes on with 4, which would make the 4-gram of sequence 1
    tokens = torch.tensor([[[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 9, 9]]])
    lens = torch.tensor([[3, 4]])
    d, _ = run_planted(tokens, lens)
    assert d[0].tolist() == [[3, 2, 1, 0], [4, 3, 2, 1], [4, 3, 2, 1]]
    d, _ = run_planted(tokens.flip(1).contiguous(), lens.flip(1).contiguous())
    assert d[0].tolist() == [[4, 3, 2, 1], [3, 2, 1, 0], [4, 3, 2, 1]]
    assert ext_calls == [True, True]


def test_planted_one_repeated_id(ext_calls):
    for K, L in [(1, 256), (3, 200), (16, 65)]:
        tokens = torch.full((2, K, L), 7)
        lens = torch.full((2, K), L)
        d, _ = run_planted(tokens, lens)
        assert d.tolist() == [[[1, 1, 1, 1]] * (K + 1)] * 2
    assert ext_calls == [True] * 3


@pytest.mark.parametrize("G,K,L,vocab", SHAPES)
def test_input_variants(ext_calls, G, K, L, vocab):
    tokens, lens, want, _ = case(G, K, L, vocab)
    t, n = tokens.to(DEV), lens.to(DEV)
    assert torch.equal(ngram_distinct(t.to(torch.int32), n.to(torch.int32)).cpu(), want)
    # a non-contiguous view
    wide = torch.full((G, K, 2 * L), vocab - 1, dtype=torch.long, device=DEV)
    wide[:, :, ::2] = t
    assert not wide[:, :, ::2].is_contiguous() or L == 1
    assert torch.equal(ngram_distinct(wide[:, :, ::2], n).cpu(), want)
    assert torch.equal(ngram_distinct(t.transpose(0, 1).contiguous().transpose(0, 1), n).cpu(), want)
    # tails poisoned with -1 (int64 and int32), lengths beyond [0, L]
    beyond = (torch.arange(L).view(1, 1, L) >= lens.unsqueeze(-1)).to(DEV)
    assert torch.equal(ngram_distinct(t.masked_fill(beyond, -1), n).cpu(), want)
    assert torch.equal(ngram_distinct(t.masked_fill(beyond, -1).to(torch.int32), n).cpu(), want)
    over = torch.where(n == L, n + 5, torch.where(n == 0, n - 3, n))
    assert torch.equal(ngram_distinct(t, over).cpu(), want)
    assert ext_calls == [True] * 6


def test_shapes_over_the_limits_take_the_fallback(ext_calls):
    for G, K, L, vocab in [(2, 17, 5, 3), (2, 2, 257, 3)]:
        tokens, lens, want, _ = case(G, K, L, vocab)
        d = ngram_distinct(tokens.to(DEV), lens.to(DEV))
        assert d.is_cuda and d.dtype == torch.int32 and torch.equal(d.cpu(), want)
    assert ext_calls == [False, False]


def test_empty_input(ext_calls):
    d = ngram_distinct(torch.zeros(0, 3, 8, dtype=torch.long, device=DEV), torch.zeros(0, 3, dtype=torch.long, device=DEV))
    assert d.shape == (0, 4, 4) and d.dtype == torch.int32 and d.is_cuda
    assert ext_calls == []  # no launch


def test_batch_forms_on_the_device(ext_calls):
    for G, K, L, vocab in [(4, 10, 64, 4), (70, 4, 33, 3), (3, 1, 9, 2)]:
        tokens, lens, _, _ = case(G, K, L, vocab)
        tokens, lens = tokens.clone(), lens.clone()
        if K > 1:  # duplicate candidates (other junk beyond the length) and an empty one
            for g in range(0, G, 2):
                n = int(lens[g, 0])
                tokens[g, K - 1, :n] = tokens[g, 0, :n]
                lens[g, K - 1] = n
            lens[1, 0] = 0
        lists = [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(G)]
        dist, div = dist_n_batch(tokens.to(DEV), lens.to(DEV)), div_n_batch(tokens.to(DEV), lens.to(DEV))
        assert dist.dtype == torch.float64 and div.dtype == torch.float64 and not dist.is_cuda and not div.is_cuda
        assert torch.equal(dist, torch.tensor([[[dist_n(s, n) for n in range(1, 5)] for s in grp] for grp in lists],
                                              dtype=torch.float64))
        assert torch.equal(div, torch.tensor([[div_n(grp, n) for n in range(1, 5)] for grp in lists],
                                             dtype=torch.float64))
    assert ext_calls == [True] * 6
