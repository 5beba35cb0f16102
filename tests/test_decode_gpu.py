"""DiffuSeq decoding on the GPU: ``sample_seq2seq`` through the native bf16 path (the
csrc/linear_argmax.hip rounding at every reverse step and for the final tokens, and the model's
hand-written forward kernels in ``eval()`` under ``no_grad``)."""
import pytest
import torch

from distributed_pipeline_amd.models import TransformerNetModel, create_gaussian_diffusion
from distributed_pipeline_amd.ops._ext import get_ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
V, L, E, T = 30522, 128, 128, 4


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


class _Oracle(torch.nn.Module):
    """Predicts the true x_start whatever it is given; decoding helpers come from ``module``."""

    def __init__(self, net, x_start):
        super().__init__()
        self.module, self.x_start = net, x_start

    def forward(self, x, t):
        return self.x_start.to(torch.bfloat16)


@pytest.mark.parametrize("clamp_step", [None, -1])
def test_oracle_model_recovers_the_input_on_the_native_path(monkeypatch, clamp_step):
    ext = get_ext(required=True)
    calls = []
    real = ext.linear_argmax
    monkeypatch.setattr(ext, "linear_argmax", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    net, batch = _model(64, 2), _batch(2)
    diff = create_gaussian_diffusion(steps=T)
    oracle = _Oracle(net, net.get_embeds(batch["input_ids"]).detach())
    gen = torch.Generator(device=DEV).manual_seed(3)
    out = diff.sample_seq2seq(oracle, batch, clamp_step=clamp_step, generator=gen)
    assert torch.equal(out["tokens"], batch["input_ids"])
    assert torch.equal(out["source_mask"], batch["input_mask"] == 0)
    # every rounding and the final decode ran the kernel, on all 2 x 128 tokens
    assert calls == [2 * L] * ((T if clamp_step is None else 0) + 1)


def test_one_real_reverse_loop_in_inference_mode():
    """A 2-layer 768-wide DiffuSeq in bf16 ``eval()`` under ``no_grad``, 4 steps, batch 4."""
    net, batch = _model(768, 12), _batch(4)
    diff = create_gaussian_diffusion(steps=T)
    a = diff.sample_seq2seq(net, batch, generator=torch.Generator(device=DEV).manual_seed(5))
    assert a["tokens"].shape == (4, L) and a["x0"].shape == (4, L, E) and a["x0"].dtype == torch.float32
    assert bool(torch.isfinite(a["x0"]).all())
    assert int(a["tokens"].min()) >= 0 and int(a["tokens"].max()) < V
    src = batch["input_mask"] == 0
    assert torch.equal(a["tokens"][src], batch["input_ids"][src])
    assert torch.equal(a["x0"][src], net.get_embeds(batch["input_ids"])[src])
