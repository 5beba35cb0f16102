"""The n-gram match kernel (csrc/ngram_match.hip) through ``ops.text.ngram_matches`` against the
``Counter`` oracle of utils/mbr.py, exactly: shapes on both sides of the wave and of the kernel's
limits, id dtypes, strides, zero lengths, poisoned tails; and ``mbr_select_batch`` on the device."""
import pytest
import torch

from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.text import ngram_matches
from utils import mbr
from utils.mbr import mbr_select, mbr_select_batch

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (G, K, L, vocabulary)
SHAPES = [(3, 2, 1, 3), (5, 3, 7, 3), (4, 10, 64, 4), (2, 16, 130, 5), (70, 4, 33, 3), (3, 1, 9, 2)]
_ORACLE = {}


def _matches(a, b):
    return [sum(min(c, mbr._ngrams(b, n)[g]) for g, c in mbr._ngrams(a, n).items()) for n in range(1, 5)]


def case(G, K, L, vocab):
    """(tokens int64 [G, K, L], lens [G, K], oracle int32 [G, K, K, 4]) on the CPU, computed once.
    The lengths 0, 1, 2, 3 and L occur; the tails hold in-range ids that also occur inside."""
    key = (G, K, L, vocab)
    if key not in _ORACLE:
        g = torch.Generator().manual_seed(G * 1000 + K * 100 + L)
        tokens = torch.randint(0, vocab, (G, K, L), generator=g)
        lens = torch.randint(0, L + 1, (G, K), generator=g)
        flat = lens.view(-1)
        for at, n in enumerate((0, 1, 2, 3, L)):
            flat[(at * 7) % flat.numel()] = min(n, L)
        seqs = [[tokens[i, k, :int(lens[i, k])].tolist() for k in range(K)] for i in range(G)]
        want = torch.tensor([[[_matches(a, b) for b in grp] for a in grp] for grp in seqs],
                            dtype=torch.int32).reshape(G, K, K, 4)
        _ORACLE[key] = (tokens, lens, want, seqs)
    return _ORACLE[key]


@pytest.fixture()
def ext_calls(monkeypatch):
    """Records, per ``ext.ngram_matches`` call, whether the kernel served it (a tensor came back)."""
    ext = get_ext(required=True)
    calls = []
    real = ext.ngram_matches

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(ext, "ngram_matches", spy)
    return calls


@pytest.mark.parametrize("G,K,L,vocab", SHAPES)
def test_kernel_against_the_counter_oracle(ext_calls, G, K, L, vocab):
    tokens, lens, want, _ = case(G, K, L, vocab)
    m = ngram_matches(tokens.to(DEV), lens.to(DEV))
    assert m.dtype == torch.int32 and m.shape == (G, K, K, 4) and m.is_cuda
    assert torch.equal(m.cpu(), want)
    assert torch.equal(m, m.transpose(1, 2))
    n = torch.arange(1, 5).view(1, 1, 4)
    assert torch.equal(torch.diagonal(m.cpu(), dim1=1, dim2=2).permute(0, 2, 1),
                       (lens.unsqueeze(-1) - n + 1).clamp_min(0).to(torch.int32))
    # bitwise reproducible
    assert torch.equal(ngram_matches(tokens.to(DEV), lens.to(DEV)), m)
    assert ext_calls == [True, True]


@pytest.mark.parametrize("G,K,L,vocab", SHAPES)
def test_input_variants(ext_calls, G, K, L, vocab):
    tokens, lens, want, _ = case(G, K, L, vocab)
    t, n = tokens.to(DEV), lens.to(DEV)
    assert torch.equal(ngram_matches(t.to(torch.int32), n.to(torch.int32)).cpu(), want)
    # a non-contiguous view
    wide = torch.full((G, K, 2 * L), vocab - 1, dtype=torch.long, device=DEV)
    wide[:, :, ::2] = t
    assert not wide[:, :, ::2].is_contiguous() or L == 1
    assert torch.equal(ngram_matches(wide[:, :, ::2], n).cpu(), want)
    assert torch.equal(ngram_matches(t.transpose(0, 1).contiguous().transpose(0, 1), n).cpu(), want)
    # tails poisoned with -1 (int64 and int32), lengths beyond [0, L]
    beyond = (torch.arange(L).view(1, 1, L) >= lens.unsqueeze(-1)).to(DEV)
    assert torch.equal(ngram_matches(t.masked_fill(beyond, -1), n).cpu(), want)
    assert torch.equal(ngram_matches(t.masked_fill(beyond, -1).to(torch.int32), n).cpu(), want)
    over = torch.where(n == L, n + 5, torch.where(n == 0, n - 3, n))
    assert torch.equal(ngram_matches(t, over).cpu(), want)
    # zero lengths everywhere: nothing matches, whatever the ids
    assert int(ngram_matches(t, torch.zeros_like(n)).abs().sum()) == 0
    assert ext_calls == [True] * 7


def test_shapes_over_the_limits_take_the_fallback(ext_calls):
    for G, K, L, vocab in [(2, 17, 5, 3), (2, 2, 257, 3)]:
        tokens, lens, want, _ = case(G, K, L, vocab)
        m = ngram_matches(tokens.to(DEV), lens.to(DEV))
        assert m.is_cuda and m.dtype == torch.int32 and torch.equal(m.cpu(), want)
    assert ext_calls == [False, False]
    # the limits themselves are covered
    tokens, lens, want, _ = case(1, 16, 256, 2)
    assert torch.equal(ngram_matches(tokens.to(DEV), lens.to(DEV)).cpu(), want)
    assert ext_calls == [False, False, True]


def test_empty_input(ext_calls):
    m = ngram_matches(torch.zeros(0, 3, 8, dtype=torch.long, device=DEV), torch.zeros(0, 3, dtype=torch.long, device=DEV))
    assert m.shape == (0, 3, 3, 4) and m.dtype == torch.int32 and m.is_cuda


def test_mbr_select_batch_on_the_device(ext_calls):
    for G, K, L, vocab in [(4, 10, 64, 4), (70, 4, 33, 3), (3, 1, 9, 2)]:
        tokens, lens, _, seqs = case(G, K, L, vocab)
        tokens, lens = tokens.clone(), lens.clone()
        if K > 1:  # duplicate candidates (other junk beyond the length) and an empty one
            for g in range(0, G, 2):
                n = int(lens[g, 0])
                tokens[g, K - 1, :n] = tokens[g, 0, :n]
                lens[g, K - 1] = n
            lens[1, 0] = 0
        lists = [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(G)]
        assert mbr_select_batch(tokens.to(DEV), lens.to(DEV)) == [mbr_select(c) for c in lists]
    assert ext_calls == [True] * 3
