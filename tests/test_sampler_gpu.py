"""Respaced / DDIM DiffuSeq sampling on the GPU with ``noise_seed``: every update outside the model
is the fused kernel of csrc/reverse_step.hip, the model reads its bf16 output, and a sample
decodes to the same bits in whatever batch it is placed."""
import pytest
import torch

from distributed_pipeline_amd.models import TransformerNetModel, create_gaussian_diffusion
from distributed_pipeline_amd.ops._ext import get_ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
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
    """A model of the decoding helpers of ``module`` and a given forward; records what it gets."""

    def __init__(self, net, fn):
        super().__init__()
        self.module, self.fn, self.seen = net, fn, []

    def forward(self, x, t):
        self.seen.append((x.dtype, int(t[0])))
        return self.fn(x)


@pytest.mark.parametrize("clamp_step", [None, -1])
@pytest.mark.parametrize("sampler", ["ancestral", "ddim"])
def test_oracle_model_recovers_the_input_through_the_kernel(monkeypatch, net, sampler, clamp_step):
    ext = get_ext(required=True)
    calls = []
    real = ext.reverse_step
    monkeypatch.setattr(ext, "reverse_step", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    batch = _batch(2)
    diff = create_gaussian_diffusion(steps=T)
    xs16 = net.get_embeds(batch["input_ids"]).detach().to(torch.bfloat16)
    oracle = _Stub(net, lambda x: xs16)
    steps = 3
    out = diff.sample_seq2seq(oracle, batch, steps=steps, sampler=sampler, eta=0.5, top_p=0.9, clamp_step=clamp_step,
                              noise_seed=11)
    assert torch.equal(out["tokens"], batch["input_ids"])
    assert torch.equal(out["source_mask"], batch["input_mask"] == 0)
    assert len(calls) == steps + 1
    # rounded steps hand ids + the fp32 table to the kernel, the others the bf16 prediction
    for k in calls[1:]:
        assert (k["idx"] is not None and k["pred"] is None) == (clamp_step is None)
    assert oracle.seen == [(torch.bfloat16, 1000 * 7 // T), (torch.bfloat16, 1000 * 4 // T), (torch.bfloat16, 0)]


def test_a_sample_decodes_the_same_in_any_batch(net):
    """The model halves its input (batch-invariant by construction), so the output is made of
    the noise of every step."""
    diff = create_gaussian_diffusion(steps=T)
    batch = _batch(4)
    kw = dict(steps=4, sampler="ddim", eta=1.0, noise_seed=5, clamp_step=-1)  # no rounding: x0 is made of noise
    run = lambda b, r0: diff.sample_seq2seq(_Stub(net, lambda x: (0.5 * x).to(torch.bfloat16)), b, row_base=r0, **kw)  # noqa: E731
    whole = run(batch, 0)
    for r0 in (0, 2):
        half = run({k: v[r0:r0 + 2] for k, v in batch.items()}, r0)
        assert torch.equal(half["x0"], whole["x0"][r0:r0 + 2])
        assert torch.equal(half["tokens"], whole["tokens"][r0:r0 + 2])
    tgt = batch["input_mask"] != 0
    assert not torch.equal(whole["x0"][0][tgt[0]], whole["x0"][1][tgt[1]])
    other = run({k: v[:2] for k, v in batch.items()}, 2)  # the first two samples placed as rows 2, 3
    assert not torch.equal(other["x0"], whole["x0"][:2])


def test_one_real_respaced_loop():
    """A 2-layer 768-wide DiffuSeq in bf16 ``eval()``: 4 DDIM steps of T = 8 with truncated noise."""
    net, batch = _model(768, 12), _batch(4)
    diff = create_gaussian_diffusion(steps=T)
    a = diff.sample_seq2seq(net, batch, steps=4, sampler="ddim", eta=0.5, top_p=0.9, noise_seed=5)
    assert a["tokens"].shape == (4, L) and a["x0"].shape == (4, L, E) and a["x0"].dtype == torch.float32
    assert bool(torch.isfinite(a["x0"]).all())
    assert int(a["tokens"].min()) >= 0 and int(a["tokens"].max()) < V
    src = batch["input_mask"] == 0
    assert torch.equal(a["tokens"][src], batch["input_ids"][src])
    assert torch.equal(a["x0"][src], net.get_embeds(batch["input_ids"])[src])
