"""DPM-Solver++ (2M) sampling on the CPU (fp32 PyTorch path): the 5-tuples of
``GaussianDiffusion.reverse_schedule`` for ``dpmpp_2m`` / ``dpmpp_2m_sde``, their second-order
accuracy on a Gaussian whose denoiser is known, the previous-prediction term of
``ops.diffusion.reverse_step``, the history of ``sample_seq2seq`` and the ``run.sample`` flags.

Tiny model as in test_sampler_cpu.py: vocabulary 100, 16 positions, 8 diffusion steps, fp32."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_pipeline_amd.models import TransformerNetModel, create_gaussian_diffusion
from distributed_pipeline_amd.ops import diffusion as dops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, L, E, T = 100, 16, 16, 8
# sampler -> the DDIM eta whose update it is when both predictions agree
SAMPLERS = {"dpmpp_2m": 0.0, "dpmpp_2m_sde": 1.0}


def _model(seed=0):
    torch.manual_seed(seed)
    m = TransformerNetModel(vocab_size=V, input_dims=E, hidden_t_dim=16, seq_len=L, config_name="tiny",
                            dropout=0.0, compute_dtype=torch.float32)
    with torch.no_grad():  # rows of one norm: a row's own logit beats every other row's clearly
        w = torch.randn(V, E)
        m.word_embedding.weight.copy_(4.0 * w / w.norm(dim=-1, keepdim=True))
        m.lm_head.bias.copy_(0.1 * torch.randn(V))
    return m.eval()


def _batch(B=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    mask[:, 6:] = 1
    return {"input_ids": ids, "input_mask": mask}


class _Oracle(torch.nn.Module):
    """Predicts the true x_start whatever it is given; decoding helpers come from ``module``."""

    def __init__(self, net, x_start):
        super().__init__()
        self.module, self.x_start, self.ts = net, x_start, []

    def forward(self, x, t):
        self.ts.append(float(t[0]))
        return self.x_start.to(x.dtype)


# ---- schedule ------------------------------------------------------------------------------
def _table(d, S, sde):
    """The coefficient table of the samplers, scalar by scalar with ``math``: lambda from
    log / log1p of alphas_cumprod, not from the square roots."""
    kept = d.kept_timesteps(S)
    ab = [float(d.alphas_cumprod[k]) for k in kept]
    lam = [0.5 * (math.log(v) - math.log1p(-v)) for v in ab]
    rows = []
    for i in range(S - 1, 0, -1):
        h = lam[i - 1] - lam[i]
        assert h > 0
        al, sg, sg_i = math.sqrt(ab[i - 1]), math.sqrt(1.0 - ab[i - 1]), math.sqrt(1.0 - ab[i])
        if sde:
            b, A, s = sg / sg_i * math.exp(-h), -al * math.expm1(-2.0 * h), sg * math.sqrt(-math.expm1(-2.0 * h))
        else:
            b, A, s = sg / sg_i, -al * math.expm1(-h), 0.0
        if i <= S - 2:
            r = (lam[i] - lam[i + 1]) / h
            rows.append((kept[i], A * (1.0 + 0.5 / r), b, s, -0.5 * A / r))
        else:
            rows.append((kept[i], A, b, s, 0.0))
    rows.append((kept[0], 1.0, 0.0, 0.0, 0.0))
    return rows


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("S", [2, 5, 20])
@pytest.mark.parametrize("steps_T", [2000, 1000])
def test_schedule_identities(steps_T, S, sampler):
    d = create_gaussian_diffusion(steps=steps_T)  # the sqrt schedule
    sched = d.reverse_schedule(S, sampler)
    assert sched == d.reverse_schedule(S, sampler, 0.0)
    assert len(sched) == S and all(len(row) == 5 for row in sched)
    kept = d.kept_timesteps(S)
    assert [row[0] for row in sched] == kept[::-1]
    assert all(isinstance(row[0], int) and all(isinstance(v, float) for v in row[1:]) for row in sched)
    # with both predictions equal the update is DDIM's: a + a_prev, b, s
    ddim = d.reverse_schedule(S, "ddim", SAMPLERS[sampler])
    worst = 0.0
    for (t, a, b, s, ap), (t2, a2, b2, s2) in zip(sched, ddim):
        assert t == t2
        worst = max(worst, abs(a + ap - a2), abs(b - b2), abs(s - s2))
    print(f"T {steps_T} S {S} {sampler}: max |difference to ddim| {worst:.2e}")
    assert worst <= 1e-10
    # first order without a history and at the jump to sigma = 0, second order in between
    assert sched[0][4] == 0.0 and sched[-1][4] == 0.0
    assert all(row[4] != 0.0 for row in sched[1:-1])
    assert sched[-1] == (kept[0], 1.0, 0.0, 0.0, 0.0)
    if sampler == "dpmpp_2m":
        assert all(row[3] == 0.0 for row in sched)
    else:
        assert all(row[3] > 0.0 for row in sched[:-1])
    # the table itself.  lambda is below 10 in magnitude and known to a few ulps (~ 4e-15); h is
    # above 0.05 here, so r and the coefficients (of magnitude ~ 1) agree to ~ 1e-13: 1e-11
    ref = _table(d, S, sampler == "dpmpp_2m_sde")
    for row, want in zip(sched, ref):
        assert row[0] == want[0]
        np.testing.assert_allclose(row[1:], want[1:], rtol=0, atol=1e-11)
    if S == 2:  # no update has a history: the DDIM chain
        np.testing.assert_allclose(np.array([row[:4] for row in sched]), np.array(ddim), rtol=0, atol=1e-10)


def test_schedule_errors_and_untouched_samplers():
    d = create_gaussian_diffusion(steps=2000)
    for sampler in SAMPLERS:
        for eta in (0.5, 1.0, -0.1):
            with pytest.raises(ValueError):
                d.reverse_schedule(5, sampler, eta)
        for bad in (0, 1, 2001, -3):
            with pytest.raises(ValueError):
                d.reverse_schedule(bad, sampler)
        assert len(d.reverse_schedule(None, sampler)) == 2000  # None: all T steps, as for the others
    with pytest.raises(ValueError):
        d.reverse_schedule(4, "dpmpp_3m")
    assert all(len(row) == 4 for row in d.reverse_schedule(5, "ddim", 0.5) + d.reverse_schedule(5, "ancestral"))


def _gaussian_chain_error(d, S, sampler, mu=0.7, c=0.5):
    """RMS error at k_0 of the chain run in float64 on data N(mu, c^2) with its exact denoiser,
    started on the exact probability-flow trajectory at k_{S-1}; the last update (the jump to
    sigma = 0) is left out."""
    kept = d.kept_timesteps(S)
    ab = d.alphas_cumprod[kept]
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    eps = np.random.default_rng(0).standard_normal(4096)

    def exact(i):
        return al[i] * mu + np.sqrt(al[i] ** 2 * c * c + sg[i] ** 2) * eps

    x, prev = exact(S - 1), None
    for j, row in enumerate(d.reverse_schedule(S, sampler, 0.0)[:-1]):
        i = S - 1 - j
        assert row[0] == kept[i] and row[3] == 0.0
        x0 = mu + al[i] * c * c / (al[i] ** 2 * c * c + sg[i] ** 2) * (x - al[i] * mu)
        a_prev = row[4] if len(row) > 4 else 0.0
        x = row[1] * x0 + row[2] * x + (a_prev * prev if a_prev != 0.0 else 0.0)
        prev = x0
    return float(np.sqrt(np.mean((x - exact(0)) ** 2)))


@pytest.mark.parametrize("S", [5, 10, 20])
def test_second_order_accuracy_on_a_gaussian(S):
    d = create_gaussian_diffusion(steps=2000)
    e1 = _gaussian_chain_error(d, S, "ddim")
    e2 = _gaussian_chain_error(d, S, "dpmpp_2m")
    print(f"S {S}: rms error ddim {e1:.3e} dpmpp_2m {e2:.3e} ratio {e1 / e2:.2f}")
    assert e2 < 0.5 * e1


# ---- op (PyTorch path) ------------------------------------------------------------------------
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@pytest.mark.parametrize("prev", ["pred_prev", "idx_prev"])
@pytest.mark.parametrize("cur", ["pred", "idx"])
def test_reverse_step_pytorch_path_with_a_previous_source(cur, prev):
    g = torch.Generator().manual_seed(0)
    x, xs, pred, predp, z = (torch.randn(2, 5, 8, generator=g) for _ in range(5))
    mask = torch.tensor([[0, 0, 1, 1, 1], [0, 1, 1, 1, 0]])
    W = torch.randn(7, 8, generator=g)
    idx = torch.tensor([[0, 1, 2, 3, 7], [6, -1, 5, 4, 3]])
    idxp = torch.tensor([[3, 2, 7, -(2 ** 40), 1], [0, 9, 4, -1, 6]])  # out of range on target positions too
    a, b, s, ap = (_f32(v) for v in (0.9, 0.6, 0.2, -0.35))

    def gathered(i):
        ok = ((i >= 0) & (i < 7)).unsqueeze(-1)
        return _f32(2.5) * W.double()[i.clamp(0, 6)] * ok

    src = dict(pred=pred) if cur == "pred" else dict(idx=idx)
    hist = dict(pred_prev=predp) if prev == "pred_prev" else dict(idx_prev=idxp)
    x0 = pred.double() if cur == "pred" else gathered(idx)
    x0p = predp.double() if prev == "pred_prev" else gathered(idxp)
    kw = dict(x_start=xs, mask=mask, weight=W, scale=2.5, a=a, b=b, s=s, seed=4, step=2, noise=z)
    out, o16 = dops.reverse_step(x, a_prev=ap, want_bf16=True, **src, **hist, **kw)
    terms = [a * x0, ap * x0p, b * x.double(), s * z.double()]
    ref = torch.where(mask.unsqueeze(-1) == 0, xs.double(), sum(terms))
    # fp32: the two scale roundings, four products and three sums, each below the sum of the
    # terms' magnitudes: at most 9 roundings
    bound = 10 * 2.0 ** -24 * sum(t.abs() for t in terms)
    tgt = (mask != 0).unsqueeze(-1).expand_as(out)
    assert out.dtype == torch.float32
    assert bool(((out.double() - ref).abs() <= bound)[tgt].all())
    assert torch.equal(out[~tgt], xs[~tgt])
    assert torch.equal(o16, out.to(torch.bfloat16))
    assert float((ap * x0p).abs()[tgt].max()) > 0.1  # the term is there
    # a_prev = 0 reads no previous source
    base = dops.reverse_step(x, **src, **kw)[0]
    nan = dict(pred_prev=torch.full_like(predp, float("nan"))) if prev == "pred_prev" else dict(idx_prev=idxp)
    assert torch.equal(dops.reverse_step(x, a_prev=0.0, **src, **nan, **kw)[0], base)
    assert not torch.equal(out, base)


def test_reverse_step_previous_source_errors():
    x = torch.zeros(2, 3, 8)
    kw = dict(pred=x, a=1.0, b=1.0, s=0.0, seed=0, step=0)
    with pytest.raises(ValueError):
        dops.reverse_step(x, a_prev=0.5, **kw)                                      # no source
    with pytest.raises(ValueError):
        dops.reverse_step(x, a_prev=0.5, idx_prev=torch.zeros(2, 3, dtype=torch.long), **kw)  # no weight
    dops.reverse_step(x, a_prev=0.0, **kw)


# ---- sampler ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("noise_seed", [None, 11])
def test_oracle_model_recovers_the_input(sampler, noise_seed):
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    oracle = _Oracle(net, net.get_embeds(batch["input_ids"]).detach())
    out = diff.sample_seq2seq(oracle, batch, steps=4, sampler=sampler, top_p=0.9, noise_seed=noise_seed,
                              generator=torch.Generator().manual_seed(3))
    assert torch.equal(out["tokens"], batch["input_ids"])
    assert torch.equal(out["source_mask"], batch["input_mask"] == 0)
    assert oracle.ts == [k * 1000.0 / T for k in diff.kept_timesteps(4)[::-1]]


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("noise_seed", [None, 5])
def test_history_across_the_clamp_boundary(monkeypatch, sampler, noise_seed):
    """5 kept steps of T = 8 are 7, 5, 4, 2, 0; clamp_step = 4 rounds from the third update on, so
    the third one has ids for this step's prediction and the fp32 tensor for the previous one."""
    net, batch = _model(), _batch()
    diff = create_gaussian_diffusion(steps=T)
    assert diff.kept_timesteps(5) == [0, 2, 4, 5, 7]
    sched = diff.reverse_schedule(5, sampler)
    calls = []
    real = dops.reverse_step
    monkeypatch.setattr(dops, "reverse_step", lambda *a, **k: (calls.append(k), real(*a, **k))[1])

    def run():
        return diff.sample_seq2seq(net, batch, steps=5, sampler=sampler, clamp_step=4, noise_seed=noise_seed,
                                   generator=torch.Generator().manual_seed(9))

    out = run()
    assert len(calls) == 6
    kinds = [("pred" if k.get("pred") is not None else "idx", "pred_prev" if k.get("pred_prev") is not None
              else "idx_prev" if k.get("idx_prev") is not None else None) for k in calls[1:]]
    assert kinds == [("pred", None), ("pred", "pred_prev"), ("idx", "pred_prev"), ("idx", "idx_prev"), ("idx", None)]
    for j, k in enumerate(calls[1:]):
        assert (k["a"], k["b"], k["s"], k.get("a_prev", 0.0)) == sched[j][1:]
        if kinds[j][1] is not None:  # the very tensor the update before used
            assert k[kinds[j][1]] is calls[j][kinds[j - 1][0]]
    assert bool(torch.isfinite(out["x0"]).all())
    again = run()
    assert torch.equal(out["x0"], again["x0"]) and torch.equal(out["tokens"], again["tokens"])


# ---- entry point ----------------------------------------------------------------------------------
def test_sample_settings_take_the_new_samplers(tmp_path):
    from config.sample import SampleSettings
    from run.sample import main
    p = SampleSettings.to_argparse(add_json=True)
    for sampler in SAMPLERS:
        assert SampleSettings.from_argparse(p.parse_args(["--sampler", sampler])).sampler == sampler
        # rejected before anything is loaded: the model path does not exist
        with pytest.raises(ValueError, match="ddim_eta"):
            main({"sampler": sampler, "ddim_eta": 0.5, "model_path": str(tmp_path / "missing")})
        with pytest.raises(FileNotFoundError):
            main({"sampler": sampler, "model_path": str(tmp_path / "missing")})
    with pytest.raises(SystemExit):
        p.parse_args(["--sampler", "dpmpp_3m"])


def test_run_sample_with_the_new_samplers_reproduces(tmp_path):
    """``run.sample --sampler dpmpp_2m | dpmpp_2m_sde --step 4`` on a freshly initialised tiny model (the
    CPU path): a second run with the same seed writes the same file; ``--ddim_eta`` is refused."""
    from config.sample import SampleSettings
    from utils.initialization import create_model_from_config
    cfg = {"model": "diffuseq", "config_name": "tiny", "vocab_size": 1200, "seq_len": 16, "hidden_dim": 16,
           "hidden_t_dim": 16, "dropout": 0.0, "diffusion_steps": 8, "precision": "fp32", "dataset": "jsonl",
           "data_dir": str(tmp_path)}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    words = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu".split()
    with open(tmp_path / "test.jsonl", "w") as f:  # hashed word ids (no vocab.txt): 1000 .. 1199
        for i in range(6):
            f.write(json.dumps({"src": " ".join(words[i:i + 4]), "trg": " ".join(words[i + 3:i + 7])}) + "\n")
    torch.manual_seed(0)
    model = create_model_from_config(**SampleSettings(**cfg).dict())
    torch.save(model.state_dict(), tmp_path / "model_000000.pt")
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    env.pop("LOCAL_RANK", None)

    def sample(out, *extra):
        return subprocess.run([sys.executable, "-m", "run.sample", "--config_json", str(tmp_path / "cfg.json"),
                               "--model_path", str(tmp_path), "--out_path", str(out), "--batch_size", "3",
                               "--num_batches", "2", "--step", "4", *extra],
                              cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)

    files = {}
    for name, extra in (("dpmpp_2m", ["--noise", "philox"]), ("dpmpp_2m_sde", ["--top_p", "0.9"])):
        texts = []
        for rep in range(2):
            out = tmp_path / f"{name}_{rep}.jsonl"
            s = sample(out, "--sampler", name, *extra)
            assert s.returncode == 0, s.stdout[-3000:] + s.stderr[-3000:]
            texts.append(out.read_text())
        assert texts[0] == texts[1]
        rows = [json.loads(line) for line in texts[0].splitlines()]
        assert len(rows) == 6
        for row in rows:
            assert set(row) == {"source", "reference", "recover"}
            assert all(isinstance(i, int) and 0 <= i < 1200 for k in row for i in row[k])
        files[name] = texts[0]
    s = sample(tmp_path / "refused.jsonl", "--sampler", "dpmpp_2m_sde", "--ddim_eta", "0.5")
    assert s.returncode != 0 and "ddim_eta" in s.stderr and "### loading" not in s.stdout
    assert not (tmp_path / "refused.jsonl").exists()
