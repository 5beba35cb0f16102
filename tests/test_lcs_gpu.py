"""The bit-parallel LCS kernel (csrc/lcs.hip) through ``ops.text.lcs_lengths`` against the textbook
dynamic programme ``utils.rouge.lcs_length``, exactly: shapes on both sides of the wave, of the
64-bit words and of the kernel's limits, planted carries and word boundaries, id dtypes, strides,
zero lengths, poisoned tails; ``mbr_select_batch(metric="rouge_l")`` and ``pairwise_rouge_l`` on the
device."""
import pytest
import torch

from distributed_pipeline_amd.ops._ext import get_ext
from distributed_pipeline_amd.ops.text import lcs_lengths
from utils.mbr import mbr_select, mbr_select_batch
from utils.rouge import lcs_length, pairwise_rouge_l, rouge_l

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (G, K, L, vocabulary)
SHAPES = [(3, 2, 1, 3), (5, 3, 7, 3), (4, 10, 64, 4), (6, 3, 65, 2), (2, 16, 20, 3), (70, 4, 33, 3), (3, 1, 9, 2),
          (2, 3, 130, 5), (2, 3, 256, 2)]
_ORACLE = {}


def oracle(seqs):
    """int32 [G, K, K] LCS lengths of the id lists ``seqs`` [G][K]: the upper triangle by the
    dynamic programme, the rest by symmetry."""
    G, K = len(seqs), len(seqs[0])
    want = torch.zeros(G, K, K, dtype=torch.int32)
    for g, grp in enumerate(seqs):
        for i in range(K):
            for j in range(i, K):
                want[g, i, j] = want[g, j, i] = lcs_length(grp[i], grp[j])
    return want


def case(G, K, L, vocab):
    """(tokens int64 [G, K, L], lens [G, K], oracle int32 [G, K, K], id lists) on the CPU, computed
    once.  The lengths 0, 1, 63, 64, 65 and L occur where L allows them; the tails hold in-range ids
    that also occur inside."""
    key = (G, K, L, vocab)
    if key not in _ORACLE:
        g = torch.Generator().manual_seed(G * 1000 + K * 100 + L)
        tokens = torch.randint(0, vocab, (G, K, L), generator=g)
        lens = torch.randint(0, L + 1, (G, K), generator=g)
        flat = lens.view(-1)
        forced = [n for n in (0, 1, 63, 64, 65, L) if n <= L]
        for at, n in enumerate(forced):
            flat[(at * 5) % flat.numel()] = n
        if flat.numel() >= len(forced):
            assert set(forced) <= set(flat.tolist())
        seqs = [[tokens[i, k, :int(lens[i, k])].tolist() for k in range(K)] for i in range(G)]
        _ORACLE[key] = (tokens, lens, oracle(seqs), seqs)
    return _ORACLE[key]


@pytest.fixture()
def ext_calls(monkeypatch):
    """Records, per ``ext.lcs_lengths`` call, whether the kernel served it (a tensor came back)."""
    ext = get_ext(required=True)
    calls = []
    real = ext.lcs_lengths

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(ext, "lcs_lengths", spy)
    return calls


@pytest.mark.parametrize("G,K,L,vocab", SHAPES)
def test_kernel_against_the_dynamic_programme(ext_calls, G, K, L, vocab):
    tokens, lens, want, _ = case(G, K, L, vocab)
    out = lcs_lengths(tokens.to(DEV), lens.to(DEV))
    assert out.dtype == torch.int32 and out.shape == (G, K, K) and out.is_cuda
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out, out.transpose(1, 2))
    assert torch.equal(torch.diagonal(out.cpu(), dim1=1, dim2=2), lens.to(torch.int32))
    # bitwise reproducible
    assert torch.equal(lcs_lengths(tokens.to(DEV), lens.to(DEV)), out)
    assert ext_calls == [True, True]


def planted():
    """K = 2 groups at L = 256 with known LCS lengths: (tokens [G, 2, 256], lens [G, 2], expected)."""
    L = 256
    rows = []  # (a, b, expected)
    for n in (1, 64, 65, 200, 256):  # one repeated token: every step's carry runs through all the words
        rows.append(([7] * 256, [7] * n, n))
    ident = [(p * 37) % 11 for p in range(256)]
    rows.append((ident, ident, 256))
    rows.append((ident[:130], ident[:130], 130))
    rows.append(([p % 5 for p in range(256)], [5 + p % 6 for p in range(256)], 0))  # disjoint alphabets
    distinct = list(range(100, 356))
    rows.append((distinct, distinct[::-1], 1))
    thinned = [t for p, t in enumerate(ident) if p % 3 != 2]
    rows.append((ident, thinned, len(thinned)))
    # the only common tokens sit at the positions 63 / 64 and 127 / 128 of a: both sides of two word boundaries
    common = [distinct[63], 900, distinct[64], 901, 902, distinct[127], distinct[128], 903]
    rows.append((distinct, common, 4))
    rows.append((common, distinct, 4))
    rows.append((distinct, common[::-1], 1))
    tokens = torch.tensor([[s + [s[0]] * (L - len(s)) for s in (a, b)] for a, b, _ in rows])
    lens = torch.tensor([[len(a), len(b)] for a, b, _ in rows])
    return tokens, lens, [e for _, _, e in rows], [[a, b] for a, b, _ in rows]


def test_planted_carries_and_word_boundaries(ext_calls):
    tokens, lens, expected, seqs = planted()
    want = oracle(seqs)
    assert want[:, 0, 1].tolist() == expected  # the hand values are the dynamic programme's
    out = lcs_lengths(tokens.to(DEV), lens.to(DEV))
    assert out[:, 0, 1].tolist() == expected
    assert torch.equal(out.cpu(), want)
    # five of them as the sequences of one group: every pair of the repeated token, the periodic
    # sequence, its thinned copy, the distinct ids and their reversal
    flat = [seqs[0][0], seqs[5][0], seqs[9][1], seqs[8][0], seqs[8][1]]
    one = torch.tensor([[s + [s[0]] * (256 - len(s)) for s in flat]])
    n = torch.tensor([[len(s) for s in flat]])
    assert torch.equal(lcs_lengths(one.to(DEV), n.to(DEV)).cpu(), oracle([flat]))
    assert ext_calls == [True, True]


@pytest.mark.parametrize("G,K,L,vocab", SHAPES)
def test_input_variants(ext_calls, G, K, L, vocab):
    tokens, lens, want, _ = case(G, K, L, vocab)
    t, n = tokens.to(DEV), lens.to(DEV)
    assert torch.equal(lcs_lengths(t.to(torch.int32), n.to(torch.int32)).cpu(), want)
    # a non-contiguous view
    wide = torch.full((G, K, 2 * L), vocab - 1, dtype=torch.long, device=DEV)
    wide[:, :, ::2] = t
    assert not wide[:, :, ::2].is_contiguous() or L == 1
    assert torch.equal(lcs_lengths(wide[:, :, ::2], n).cpu(), want)
    assert torch.equal(lcs_lengths(t.transpose(0, 1).contiguous().transpose(0, 1), n).cpu(), want)
    # tails poisoned with -1 (int64 and int32), lengths beyond [0, L]
    beyond = (torch.arange(L).view(1, 1, L) >= lens.unsqueeze(-1)).to(DEV)
    assert torch.equal(lcs_lengths(t.masked_fill(beyond, -1), n).cpu(), want)
    assert torch.equal(lcs_lengths(t.masked_fill(beyond, -1).to(torch.int32), n).cpu(), want)
    over = torch.where(n == L, n + 5, torch.where(n == 0, n - 3, n))
    assert torch.equal(lcs_lengths(t, over).cpu(), want)
    # zero lengths everywhere: nothing matches, whatever the ids
    assert int(lcs_lengths(t, torch.zeros_like(n)).abs().sum()) == 0
    assert ext_calls == [True] * 7


def test_shapes_over_the_limits_take_the_fallback(ext_calls):
    for G, K, L, vocab in [(2, 17, 5, 3), (2, 2, 257, 3)]:
        tokens, lens, want, _ = case(G, K, L, vocab)
        out = lcs_lengths(tokens.to(DEV), lens.to(DEV))
        assert out.is_cuda and out.dtype == torch.int32 and torch.equal(out.cpu(), want)
    assert ext_calls == [False, False]


def test_empty_input(ext_calls):
    out = lcs_lengths(torch.zeros(0, 3, 8, dtype=torch.long, device=DEV),
                      torch.zeros(0, 3, dtype=torch.long, device=DEV))
    assert out.shape == (0, 3, 3) and out.dtype == torch.int32 and out.is_cuda


def with_duplicates(G, K, L, vocab):
    """The random case with duplicated candidates (other junk beyond the length) and an empty one."""
    tokens, lens, _, _ = case(G, K, L, vocab)
    tokens, lens = tokens.clone(), lens.clone()
    if K > 1:
        for g in range(0, G, 2):
            n = int(lens[g, 0])
            tokens[g, K - 1, :n] = tokens[g, 0, :n]
            lens[g, K - 1] = n
        lens[1, 0] = 0
    lists = [[tokens[g, k, :int(lens[g, k])].tolist() for k in range(K)] for g in range(G)]
    return tokens, lens, lists


def test_mbr_select_batch_rouge_l_on_the_device(ext_calls):
    for G, K, L, vocab in [(4, 10, 64, 4), (70, 4, 33, 3), (3, 1, 9, 2)]:
        tokens, lens, lists = with_duplicates(G, K, L, vocab)
        picks = mbr_select_batch(tokens.to(DEV), lens.to(DEV), metric="rouge_l")
        assert picks == [mbr_select(c, metric="rouge_l") for c in lists]
    assert ext_calls == [True] * 3


def test_pairwise_rouge_l_on_the_device(ext_calls):
    for G, K, L, vocab in [(5, 3, 7, 3), (6, 3, 65, 2)]:
        tokens, lens, lists = with_duplicates(G, K, L, vocab)
        pr = pairwise_rouge_l(tokens.to(DEV), lens.to(DEV))
        assert pr.dtype == torch.float64 and pr.shape == (G, K, K) and not pr.is_cuda
        assert pr.tolist() == [[[rouge_l(a, b) for b in c] for a in c] for c in lists]
    assert ext_calls == [True] * 2
