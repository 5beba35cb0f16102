"""DPM-Solver++ (2M) sampling on the GPU: the four-term update of csrc/reverse_step.hip
(``a x0 + a_prev x0_prev + b x + s z``) against float64 for every pair of x0 sources, the untouched
three-term arithmetic, batch independence, and the history ``sample_seq2seq`` hands from one update
to the next - replayed in float64 - for both new samplers, across the ``clamp_step`` boundary."""
import numpy as np
import pytest
import torch

from distributed_pipeline_amd.models import TransformerNetModel, create_gaussian_diffusion
from distributed_pipeline_amd.ops import diffusion as dops
from distributed_pipeline_amd.ops._ext import get_ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -24
SAMPLERS = ["dpmpp_2m", "dpmpp_2m_sde"]


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _noise(shape, **kw):
    """z of the kernel: a = b = 0, s = 1 under an all-ones mask."""
    ones = torch.ones(shape[:-1], dtype=torch.long, device=DEV)
    xs = torch.zeros(shape, device=DEV)
    args = dict(seed=7, step=3, row_base=0, top_p=0.0)
    args.update(kw)
    return dops.reverse_step(None, x_start=xs, mask=ones, a=0.0, b=0.0, s=1.0, **args)[0]


@pytest.fixture()
def ext_calls(monkeypatch):
    """The keyword arguments of the extension's reverse_step launches: every case here must take the kernel."""
    ext = get_ext(required=True)
    calls = []
    real = ext.reverse_step
    monkeypatch.setattr(ext, "reverse_step", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    return calls


def _case(B, L, E, seed):
    """Inputs of one update with both kinds of both sources; every id tensor has four ids outside
    [0, V) in row 0, on target positions."""
    g = torch.Generator().manual_seed(seed)
    V = 50
    c = dict(V=V, x=torch.randn(B, L, E, generator=g), xs=torch.randn(B, L, E, generator=g),
             pred=torch.randn(B, L, E, generator=g).to(torch.bfloat16),
             predp=torch.randn(B, L, E, generator=g).to(torch.bfloat16), W=torch.randn(V, E, generator=g),
             idx=torch.randint(0, V, (B, L), generator=g), idxp=torch.randint(0, V, (B, L), generator=g),
             mask=(torch.rand(B, L, generator=g) < 0.6).long())  # boundaries inside a wave
    c["mask"][0, :6] = 1
    c["idx"][0, :4] = torch.tensor([-1, V, V + 7, -(2 ** 40)])
    c["idxp"][0, 2:6] = torch.tensor([V, -(2 ** 40), -1, V + 7])
    return {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in c.items()}


def _x0(c, kind, name):
    """(keyword arguments, float64 value) of the source ``name`` (pred / idx, or their _prev)."""
    p = "p" if name.endswith("_prev") else ""
    if kind == "pred":
        return {name: c["pred" + p]}, c["pred" + p].double()
    i = c["idx" + p]
    ok = ((i >= 0) & (i < c["V"])).unsqueeze(-1)
    return {name: i}, 2.5 * c["W"].double()[i.clamp(0, c["V"] - 1)] * ok


@pytest.mark.parametrize("top_p", [0.0, 0.9])
@pytest.mark.parametrize("prev", ["pred", "idx"])
@pytest.mark.parametrize("cur", ["pred", "idx"])
@pytest.mark.parametrize("B,L,E", [(3, 20, 16), (1, 77, 128)])
def test_four_term_formula_against_float64(ext_calls, B, L, E, cur, prev, top_p):
    c = _case(B, L, E, B * 1000 + E)
    a, b, s, ap = (_f32(v) for v in (1.37, 0.61, 0.23, -0.41))
    src, x0 = _x0(c, cur, cur)
    hist, x0p = _x0(c, prev, prev + "_prev")
    kw = dict(x_start=c["xs"], mask=c["mask"], weight=c["W"], scale=2.5, a=a, b=b, s=s, seed=7, step=3, row_base=5,
              top_p=top_p)
    out, out16 = dops.reverse_step(c["x"], a_prev=ap, want_bf16=True, **src, **hist, **kw)
    z = _noise((B, L, E), row_base=5, top_p=top_p).double()
    assert len(ext_calls) == 2
    k = ext_calls[0]
    assert k["a_prev"] == ap and (k["pred_prev"] is not None) == (prev == "pred")
    assert (k["idx_prev"] is not None) == (prev == "idx") and (k["pred"] is not None) == (cur == "pred")
    assert out.dtype == torch.float32 and out.shape == (B, L, E) and out16.dtype == torch.bfloat16
    terms = [a * x0, ap * x0p, b * c["x"].double(), s * z]
    ref = sum(terms)
    # one multiply and three fused adds, one scale rounding per gathered source: at most six roundings
    bound = 6 * EPS * sum(t.abs() for t in terms)
    tgt = c["mask"].unsqueeze(-1).expand(B, L, E) != 0
    err = (out.double() - ref).abs()
    print(f"max err / bound on the target rows: {float((err / bound.clamp_min(1e-300))[tgt].max()):.3f}")
    assert bool((err <= bound)[tgt].all())
    assert float(terms[1].abs()[tgt].max()) > 0.1  # the previous term is there
    assert torch.equal(out[~tgt], c["xs"][~tgt])         # source rows: x_start, bit for bit
    assert torch.equal(out16, out.to(torch.bfloat16))    # round to nearest even
    if prev == "idx":  # an id outside [0, V): that source contributes a zero row
        bad = torch.zeros(B, L, dtype=torch.bool, device=DEV)
        bad[0, 2:6] = True
        assert bool((x0p[bad] == 0).all()) and bool(tgt[bad].all())
    out_b, none = dops.reverse_step(c["x"], a_prev=ap, **src, **hist, **kw)  # without the bf16 copy; same bits
    assert none is None and torch.equal(out_b, out)


@pytest.mark.parametrize("top_p", [0.0, 0.9])
@pytest.mark.parametrize("cur", ["pred", "idx"])
def test_a_prev_zero_is_the_three_term_update(ext_calls, cur, top_p):
    c = _case(1, 77, 128, 5)
    src, _ = _x0(c, cur, cur)
    kw = dict(x_start=c["xs"], mask=c["mask"], weight=c["W"], scale=2.5, a=0.37, b=0.61, s=0.23, seed=7, step=3,
              row_base=5, top_p=top_p, want_bf16=True)
    base = dops.reverse_step(c["x"], **src, **kw)
    nan = torch.full_like(c["predp"], float("nan"))
    same = dops.reverse_step(c["x"], pred_prev=nan, a_prev=0.0, **src, **kw)
    assert torch.equal(same[0], base[0]) and torch.equal(same[1], base[1])
    assert ext_calls[1].get("pred_prev") is None and ext_calls[1].get("a_prev", 0.0) == 0.0  # not even handed over
    for hist in (dict(pred_prev=c["predp"]), dict(idx_prev=c["idxp"])):
        one = dops.reverse_step(c["x"], a_prev=-0.41, **src, **hist, **kw)
        two = dops.reverse_step(c["x"], a_prev=-0.41, **src, **hist, **kw)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
        assert not torch.equal(one[0], base[0])
    assert len(ext_calls) == 6


def test_previous_source_errors(ext_calls):
    c = _case(1, 8, 16, 1)
    kw = dict(pred=c["pred"], a=1.0, b=1.0, s=0.0, seed=0, step=0)
    with pytest.raises(ValueError):
        dops.reverse_step(c["x"], a_prev=0.5, **kw)
    ext = get_ext(required=True)
    with pytest.raises(RuntimeError):  # the binding refuses a_prev != 0 without a source
        ext.reverse_step(c["x"], 8, 16, x=c["x"].view(8, 16), pred=c["pred"].view(8, 16), a=1.0, b=1.0, a_prev=0.5)


@pytest.mark.parametrize("prev", ["pred", "idx"])
def test_four_term_batch_independence(ext_calls, prev):
    g = torch.Generator().manual_seed(4)
    E, V = 128, 50
    x = torch.randn(64, E, generator=g).to(DEV)
    pred, predp = (torch.randn(64, E, generator=g).to(DEV).to(torch.bfloat16) for _ in range(2))
    W = torch.randn(V, E, generator=g).to(DEV)
    idxp = torch.randint(0, V, (64,), generator=g).to(DEV)

    def run(r0, r1):
        hist = dict(pred_prev=predp[r0:r1]) if prev == "pred" else dict(idx_prev=idxp[r0:r1], weight=W)
        return dops.reverse_step(x[r0:r1], pred=pred[r0:r1], a=1.37, b=0.61, s=0.23, a_prev=-0.41, seed=7, step=3,
                                 row_base=r0, top_p=0.9, **hist)[0]

    full = run(0, 64)
    for r0, r1 in ((0, 7), (7, 40), (40, 64)):
        assert torch.equal(run(r0, r1), full[r0:r1])
    assert len(ext_calls) == 4


# ---- the sampler's history ----------------------------------------------------------------------
class _TinyNet(torch.nn.Module):
    """The decoding helpers ``_reverse_loop`` reads, in plain PyTorch, on a [V, E] table."""

    def __init__(self, V, E, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.word_embedding = torch.nn.Embedding(V, E)
        with torch.no_grad():
            self.word_embedding.weight.copy_(torch.randn(V, E, generator=g))
        self.emb_scale_factor, self.compute_dtype = 1.0, torch.bfloat16

    def get_embeds(self, ids):
        return self.word_embedding.weight.detach()[ids]

    def rounding_offsets(self):
        return -0.5 * self.word_embedding.weight.detach().pow(2).sum(-1)

    def nearest_tokens(self, x, c=None):
        return (x.float() @ self.word_embedding.weight.detach().t() + c).argmax(-1)

    def decode_tokens(self, x):
        return self.nearest_tokens(x, self.rounding_offsets())


class _Fixed(torch.nn.Module):
    """A model that answers its j-th call with the j-th of the given tensors."""

    def __init__(self, net, answers):
        super().__init__()
        self.module, self.answers, self.n = net, answers, 0

    def forward(self, x, t):
        self.n += 1
        return self.answers[self.n - 1]


@pytest.mark.parametrize("clamp_step", [-1, 1200])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_history_wiring_and_float64_replay(monkeypatch, sampler, clamp_step):
    """5 kept steps of T = 2000 are 1999, 1499, 1000, 500, 0: clamp_step = 1200 rounds the last three."""
    B, L, E, V, S = 3, 20, 16, 50, 5
    net = _TinyNet(V, E).to(DEV)
    W = net.word_embedding.weight.detach()
    diff = create_gaussian_diffusion(steps=2000)
    kept = diff.kept_timesteps(S)[::-1]
    assert kept[1] > 1200 > kept[2]
    sched = diff.reverse_schedule(S, sampler)
    g = torch.Generator().manual_seed(6)
    P = [torch.randn(B, L, E, generator=g).to(DEV).to(torch.bfloat16) for _ in range(S)]
    ids = torch.randint(0, V, (B, L), generator=g).to(DEV)
    mask = torch.zeros(B, L, dtype=torch.long, device=DEV)
    mask[:, 7:] = 1
    ext = get_ext(required=True)
    launches = []
    real_ext = ext.reverse_step
    monkeypatch.setattr(ext, "reverse_step", lambda *a, **k: (launches.append(1), real_ext(*a, **k))[1])
    calls = []
    real = dops.reverse_step

    def recorded(x, **k):
        out = real(x, **k)
        z = None
        if k["s"] != 0.0 and x is not None:  # the z of this update, from the kernel itself
            z = real(None, x_start=torch.zeros_like(k["x_start"]), mask=torch.ones_like(k["mask"]), a=0.0, b=0.0,
                     s=1.0, seed=k["seed"], step=k["step"], row_base=k["row_base"], top_p=k["top_p"])[0]
        calls.append(dict(k, x=x, out=out[0], out16=out[1], z=z))
        return out

    monkeypatch.setattr(dops, "reverse_step", recorded)
    top_p = 0.9 if sampler == "dpmpp_2m_sde" else 0.0
    res = diff.sample_seq2seq(_Fixed(net, P), {"input_ids": ids, "input_mask": mask}, steps=S, sampler=sampler,
                              clamp_step=clamp_step, noise_seed=13, row_base=2, top_p=top_p)
    assert len(calls) == S + 1
    n_sde = sum(1 for row in sched if row[3] != 0.0)
    assert len(launches) == S + 1 + n_sde  # every update took the kernel
    rounded = [k <= clamp_step for k in kept]  # -1: no update rounds
    assert rounded == ([False] * 5 if clamp_step < 0 else [False, False, True, True, True])

    def source(k, suffix=""):
        name = "pred" if k.get("pred" + suffix) is not None else "idx"
        return name, k.get(name + suffix)

    for j, (k, row) in enumerate(zip(calls[1:], sched)):
        got = np.float32([k["a"], k["b"], k["s"], k.get("a_prev", 0.0)])
        assert (got == np.float32(row[1:])).all()
        assert k["step"] == S - 1 - j and k["row_base"] == 2 * L and k["noise"] is None
        name, cur = source(k)
        assert name == ("idx" if rounded[j] else "pred")
        assert cur.dtype == (torch.int64 if rounded[j] else torch.bfloat16)
        if not rounded[j]:
            assert cur is P[j]
        if j in (0, S - 1):  # no history yet / the jump to sigma = 0
            assert k.get("a_prev", 0.0) == 0.0 and k.get("pred_prev") is None and k.get("idx_prev") is None
        else:  # the very x0 source of the update before
            pname, prev = source(k, "_prev")
            before = source(calls[j])
            assert (pname, id(prev)) == (before[0], id(before[1]))
            assert (k.get("pred_prev") is None) != (k.get("idx_prev") is None)
    if clamp_step >= 0:
        assert source(calls[3])[0] == "idx" and source(calls[3], "_prev")[0] == "pred"
        assert source(calls[4])[0] == "idx" and source(calls[4], "_prev")[0] == "idx"

    # float64 replay from the recorded start noise up to the state after the penultimate update
    tgt = (mask != 0).unsqueeze(-1).expand(B, L, E)
    xs = W[ids]
    assert torch.equal(calls[0]["out"][~tgt], xs[~tgt])

    def value(name, t):
        return t.double() if name == "pred" else W.double()[t]

    x, err = calls[0]["out"].double(), torch.zeros(B, L, E, dtype=torch.float64, device=DEV)
    for j in range(S - 1):
        k = calls[j + 1]
        a, b, s, ap = (float(v) for v in np.float32([k["a"], k["b"], k["s"], k.get("a_prev", 0.0)]))
        terms = [a * value(*source(k)), b * x]
        if ap != 0.0:
            terms.append(ap * value(*source(k, "_prev")))
        if s != 0.0:
            terms.append(s * k["z"].double())
        x = torch.where(tgt, sum(terms), xs.double())
        err = abs(b) * err + 6 * EPS * (sum(t.abs() for t in terms) + abs(b) * err)
        got = k["out"].double()
        assert torch.equal(k["out"][~tgt], xs[~tgt])
        assert torch.equal(k["out16"], k["out"].to(torch.bfloat16))
        print(f"update {j}: max |difference| {float((got - x).abs()[tgt].max()):.3e}, "
              f"bound there at most {float(err[tgt].max()):.3e}")
    assert bool(((got - x).abs() <= err)[tgt].all())
    assert float(err[tgt].max()) < 1e-4  # the bound says something
    # the last update returns the last prediction (rounded: its nearest embeddings)
    last = calls[S]
    assert torch.equal(res["x0"], last["out"])
    assert torch.equal(res["x0"][tgt], value(*source(last)).float()[tgt])


# ---- a real model's helpers -------------------------------------------------------------------------
V, L, E, T = 30522, 128, 128, 8


def _model(hidden, heads, seed=0):
    torch.manual_seed(seed)
    m = TransformerNetModel(vocab_size=V, input_dims=E, hidden_t_dim=128, seq_len=L, config_name="tiny",
                            hidden_size=hidden, num_layers=2, num_heads=heads, dropout=0.1,
                            compute_dtype=torch.bfloat16)
    with torch.no_grad():  # rows of one norm: a row's own logit beats every other row's clearly
        w = torch.randn(V, E)
        m.word_embedding.weight.copy_(4.0 * w / w.norm(dim=-1, keepdim=True))
        m.lm_head.bias.copy_(0.1 * torch.randn(V))
    return m.to(DEV).eval()


def _batch(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, V, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    mask[:, 48:] = 1
    return {"input_ids": ids.to(DEV), "input_mask": mask.to(DEV)}


@pytest.fixture(scope="module")
def net():
    return _model(64, 2)


class _Stub(torch.nn.Module):
    """A model of the decoding helpers of ``module`` and a given forward."""

    def __init__(self, net, fn):
        super().__init__()
        self.module, self.fn = net, fn

    def forward(self, x, t):
        return self.fn(x)


@pytest.mark.parametrize("clamp_step", [None, -1])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_oracle_model_recovers_the_input_through_the_kernel(ext_calls, net, sampler, clamp_step):
    batch = _batch(2)
    diff = create_gaussian_diffusion(steps=T)
    xs16 = net.get_embeds(batch["input_ids"]).detach().to(torch.bfloat16)
    steps = 4
    out = diff.sample_seq2seq(_Stub(net, lambda x: xs16), batch, steps=steps, sampler=sampler, top_p=0.9,
                              clamp_step=clamp_step, noise_seed=11)
    assert torch.equal(out["tokens"], batch["input_ids"])
    assert torch.equal(out["source_mask"], batch["input_mask"] == 0)
    assert len(ext_calls) == steps + 1
    for j, k in enumerate(ext_calls[1:]):
        assert (k["idx"] is not None and k["pred"] is None) == (clamp_step is None)
        has_prev = j in (1, 2)
        assert (k.get("a_prev", 0.0) != 0.0) == has_prev
        assert (k.get("idx_prev") is not None) == (has_prev and clamp_step is None)
        assert (k.get("pred_prev") is not None) == (has_prev and clamp_step is not None)


def test_a_sample_decodes_the_same_in_any_batch(net):
    """The model halves its input (batch-invariant by construction), so the output is made of the
    noise of every step and of the history of every sample."""
    diff = create_gaussian_diffusion(steps=T)
    batch = _batch(8)
    kw = dict(steps=5, sampler="dpmpp_2m_sde", noise_seed=5, clamp_step=-1)  # no rounding: x0 is made of noise
    half = _Stub(net, lambda x: (0.5 * x).to(torch.bfloat16))

    def run(b, r0):
        return diff.sample_seq2seq(half, b, row_base=r0, **kw)

    whole = run(batch, 0)
    for r0, r1 in ((0, 3), (3, 8)):
        part = run({k: v[r0:r1] for k, v in batch.items()}, r0)
        assert torch.equal(part["x0"], whole["x0"][r0:r1])
        assert torch.equal(part["tokens"], whole["tokens"][r0:r1])
    tgt = batch["input_mask"] != 0
    assert not torch.equal(whole["x0"][0][tgt[0]], whole["x0"][1][tgt[1]])
