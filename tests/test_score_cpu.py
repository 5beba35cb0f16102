"""Teacher-forced scoring on the CPU (fp32 PyTorch path): ``GPT2LMModel.score`` against the full
forward, ``generate(return_logprobs=True)`` against ``score``, and ``python -m run.score`` /
``python -m run.generate --logprobs``."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_pipeline_amd.models import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 300


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2,
                       vocab_size=V, seq_len=64, dropout=0.0, precision="fp32").eval()


def _ids(B=4, L=40, seed=1):
    return torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(seed))


def test_score_is_the_log_softmax_of_the_full_forward(model):
    """The same fp32 math in another order (only the scored rows go through the head): 1e-5."""
    ids = _ids()
    lens, start = torch.tensor([40, 2, 17, 33]), torch.tensor([0, 1, 5, 33])
    res = model.score(ids, lens, start=start)
    assert {k: (v.dtype, tuple(v.shape)) for k, v in res.items()} == {
        "logp": (torch.float32, (4, 39)), "rank": (torch.int32, (4, 39)), "entropy": (torch.float32, (4, 39)),
        "top1": (torch.int64, (4, 39)), "mask": (torch.bool, (4, 39))}
    p = torch.arange(1, 40).view(1, 39)
    mask = (p >= start.clamp(min=1).view(4, 1)) & (p < lens.view(4, 1))
    assert torch.equal(res["mask"], mask) and mask.sum(1).tolist() == [39, 1, 12, 0]
    with torch.no_grad():
        logits = model(ids)[:, :-1]
        ce = model(ids, labels=ids)
    lsm = torch.log_softmax(logits, -1)
    tgt = ids[:, 1:]
    want = lsm.gather(2, tgt.unsqueeze(-1)).squeeze(-1)
    # rows 0 and 2 see no padding; a row's prefix does not depend on what follows it (causal)
    assert (res["logp"] - want)[mask].abs().max() <= 1e-5
    assert (res["logp"] + ce)[mask].abs().max() <= 1e-5
    ent = -(lsm.exp() * lsm).sum(-1)
    assert (res["entropy"] - ent)[mask].abs().max() <= 1e-5
    st = logits.gather(2, tgt.unsqueeze(-1))
    ids_v = torch.arange(V).view(1, 1, V)
    rank = (logits > st).sum(-1) + ((logits == st) & (ids_v < tgt.unsqueeze(-1))).sum(-1)
    assert torch.equal(res["rank"][mask].long(), rank[mask]) and torch.equal(res["top1"][mask], logits.argmax(-1)[mask])
    # outside the mask: the fill values
    assert (res["logp"][~mask] == 0).all() and (res["rank"][~mask] == -1).all()
    assert (res["entropy"][~mask] == 0).all() and (res["top1"][~mask] == -1).all()
    again = model.score(ids, lens, start=start)
    assert all(torch.equal(res[k], again[k]) for k in res)


def test_score_ignores_training_mode_and_what_lies_behind_lens():
    torch.manual_seed(0)
    m = build_model(model="gpt2", config_name="tiny", hidden_size=64, num_layers=2, num_heads=2,
                    vocab_size=V, seq_len=64, dropout=0.5, precision="fp32")
    ids = _ids(B=3, L=20)
    lens = torch.tensor([20, 7, 12])
    m.eval()
    want = m.score(ids, lens)
    m.train()
    got = m.score(ids, lens)
    assert m.training and all(torch.equal(want[k], got[k]) for k in want)
    poisoned = ids.clone()
    poisoned[1, 7:] = -12345       # no embedding row: an index error if it were looked at
    poisoned[2, 12:] = V + 999
    got = m.score(poisoned, lens)
    assert all(torch.equal(want[k], got[k]) for k in want)
    # defaults: lens = L, start = 1, and lists are taken
    full = m.score(ids)
    assert full["mask"].all() and torch.equal(full["logp"][0], want["logp"][0])
    assert torch.equal(m.score(ids, [20, 7, 12], start=[1, 1, 1])["logp"], want["logp"])


def test_score_edge_shapes_and_bad_arguments(model):
    one = model.score(_ids(B=3, L=1))
    assert all(v.shape == (3, 0) for v in one.values())
    none = model.score(_ids(B=0, L=9))
    assert all(v.shape == (0, 8) for v in none.values())
    empty = model.score(_ids(B=2, L=9), [1, 0])            # nothing to score: shaped fill values
    assert not empty["mask"].any() and (empty["rank"] == -1).all() and (empty["logp"] == 0).all()
    empty = model.score(_ids(B=2, L=9), start=[9, 9])
    assert not empty["mask"].any()
    ids = _ids(B=2, L=9)
    for kw in (dict(lens=[10, 3]), dict(lens=[-1, 3]), dict(start=[0, 10]), dict(start=[-1, 0]), dict(lens=[3]),
               dict(lens=torch.tensor([3.0, 4.0]))):
        with pytest.raises(ValueError):
            model.score(ids, kw.get("lens"), start=kw.get("start"))
    with pytest.raises(ValueError):
        model.score(ids[0])
    with pytest.raises(ValueError):
        model.score(_ids(B=1, L=model.cfg["max_position_embeddings"] + 1))  # beyond the position table


def test_generate_logprobs_are_the_scores_of_the_continuation(model):
    """No penalties: a log-probability moves at most twice the largest logit change, and cached logits
    are held within 1e-4 of the full forward (test_generate_cpu.py): 2e-4."""
    ids = _ids(B=3, L=10, seed=2)
    lens = torch.tensor([10, 10, 10])
    N = 8
    for kw in (dict(temperature=0), dict(temperature=0.9, top_k=20, generator=torch.Generator().manual_seed(5)),
               dict(temperature=0.8, top_p=0.9, noise_seed=7)):
        plain = model.generate(ids, lens, N, **{**kw, **({"generator": torch.Generator().manual_seed(5)}
                                                       if "generator" in kw else {})})
        toks, new_lens, lp = model.generate(ids, lens, N, return_logprobs=True, **kw)
        assert len(plain) == 2 and torch.equal(plain[0], toks) and torch.equal(plain[1], new_lens)
        assert lp.dtype == torch.float32 and lp.shape == (3, N) and (lp < 0).all()
        sc = model.score(torch.cat([ids, toks], 1), start=[10, 10, 10])
        assert (sc["logp"][:, 9:] - lp).abs().max() <= 2e-4
    # zeros behind a finished row; ragged prompts
    lens = torch.tensor([10, 4, 7])
    free, _ = model.generate(ids, lens, N, temperature=0)
    eos = int(free[1, 2])
    toks, new_lens, lp = model.generate(ids, lens, N, temperature=0, eos_id=eos, return_logprobs=True)
    assert int(new_lens[1]) == free[1].tolist().index(eos) + 1 < N
    for b in range(3):
        n = int(new_lens[b])
        assert (lp[b, n:] == 0).all() and (lp[b, :n] < 0).all()
        seq = torch.cat([ids[b, :lens[b]], toks[b, :n]]).view(1, -1)
        sc = model.score(seq, start=[int(lens[b])])
        assert (sc["logp"][0, int(lens[b]) - 1:] - lp[b, :n]).abs().max() <= 2e-4
    # the other two decoders have scores or stats of their own and do not take the keyword
    with pytest.raises(TypeError):
        model.beam_search(ids, lens, 4, num_beams=2, return_logprobs=True)
    with pytest.raises(TypeError):
        model.generate_lookahead(ids, lens, 4, lookahead=2, return_logprobs=True)


# ---- python -m run.score, python -m run.generate --logprobs ------------------------------------

def test_run_score_entry_point(tmp_path):
    """A 2-step tiny GPT-2 training run on the CPU, then ``python -m run.score`` on its checkpoint
    directory: the split, and a ``run.generate`` file."""
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1", WANDB_MODE="disabled")
    env.pop("LOCAL_RANK", None)
    ck = tmp_path / "ck"
    common = ["--model", "gpt2", "--config_name", "tiny", "--vocab_size", "200", "--seq_len", "32",
              "--dropout", "0.0", "--precision", "fp32", "--dataset", "synthetic", "--data_loader_workers", "0"]
    r = subprocess.run([sys.executable, "-m", "run.train", *common, "--batch_size", "4", "--microbatch", "4",
                        "--learning_steps", "2", "--save_interval", "2", "--log_interval", "1",
                        "--eval_interval", "100", "--ema_rate", "0.9", "--checkpoint_path", str(ck)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def run(module, *extra, ok=True, cfg=ck / "training_args.json"):
        s = subprocess.run([sys.executable, "-m", module, "--config_json", str(cfg), "--model_path", str(ck), *extra],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
        assert (s.returncode == 0) == ok, s.stdout[-3000:] + s.stderr[-3000:]
        return s.stdout + s.stderr

    def summary(log):
        return json.loads([line for line in log.splitlines() if line.startswith("{")][-1])

    def rows(path):
        return [json.loads(line) for line in open(path)]

    def consistent(total, per_row):
        assert total["n_rows"] == len(per_row) and total["n_tokens"] == sum(r_["tokens"] for r_ in per_row)
        nll = sum(r_["nll"] for r_ in per_row)
        assert math.isclose(total["ppl"], math.exp(nll / total["n_tokens"]), rel_tol=1e-9)
        assert math.isclose(total["nll"], nll / total["n_tokens"], rel_tol=1e-9)
        assert math.isclose(total["bits_per_token"], total["nll"] / math.log(2), rel_tol=1e-9)
        assert 0 <= total["top1"] <= total["top5"] <= 1 and total["entropy"] > 0
        for r_ in per_row:
            if r_["tokens"]:
                assert math.isclose(r_["ppl"], math.exp(r_["nll"] / r_["tokens"]), rel_tol=1e-9)
                assert 0 <= r_["top1_acc"] <= 1 and 0 <= r_["mean_rank"] < 200 and r_["mean_entropy"] > 0
            else:
                assert r_["ppl"] is None and r_["nll"] == 0

    # the split: 2 batches of 3 rows, scored from position 8 on
    log = run("run.score", "--batch_size", "3", "--num_batches", "2", "--prompt_len", "8",
              "--out_path", str(tmp_path / "s.jsonl"), "--keep_tokens", "true")
    assert "model_000002.pt" in log
    total, per_row = summary(log), rows(tmp_path / "s.jsonl")
    assert total["n_rows"] == 6 and total["n_tokens"] == 6 * (32 - 8)
    consistent(total, per_row)
    for r_ in per_row:
        assert len(r_["logprobs"]) == len(r_["ranks"]) == 24 and all(x <= 0 for x in r_["logprobs"])
        assert math.isclose(r_["nll"], -sum(r_["logprobs"]), rel_tol=1e-9)
        assert r_["top1_acc"] == sum(k == 0 for k in r_["ranks"]) / 24
    # an untrained-size vocabulary: perplexity near 200 after two steps
    assert 50 < total["ppl"] < 800
    # a --config_json round trip: the settings written out and read back give the same numbers
    from config.score import ScoreSettings
    from run.score import create_parser
    ns = create_parser().parse_args(["--config_json", str(ck / "training_args.json"), "--model_path", str(ck),
                                     "--batch_size", "3", "--num_batches", "2", "--prompt_len", "8"])
    args = ScoreSettings.from_argparse(ns)
    assert args.model == "gpt2" and args.vocab_size == 200 and args.prompt_len == 8 and args.field == "continuation"
    (tmp_path / "score.json").write_text(args.json())
    assert ScoreSettings.parse_file(tmp_path / "score.json") == args
    again = summary(run("run.score", cfg=tmp_path / "score.json"))
    assert again == total

    # a run.generate file, with log-probabilities of its own
    gen = ["--batch_size", "3", "--num_batches", "2", "--prompt_len", "8", "--max_new_tokens", "6", "--temperature", "0"]
    run("run.generate", *gen, "--out_path", str(tmp_path / "g.jsonl"))
    greedy = rows(tmp_path / "g.jsonl")
    eos = greedy[0]["continuation"][2]
    run("run.generate", *gen, "--eos_id", str(eos), "--out_path", str(tmp_path / "a.jsonl"))
    run("run.generate", *gen, "--eos_id", str(eos), "--logprobs", "false", "--out_path", str(tmp_path / "b.jsonl"))  # the default
    run("run.generate", *gen, "--eos_id", str(eos), "--logprobs", "true", "--out_path", str(tmp_path / "c.jsonl"))
    assert open(tmp_path / "a.jsonl", "rb").read() == open(tmp_path / "b.jsonl", "rb").read()
    plain, with_lp = rows(tmp_path / "a.jsonl"), rows(tmp_path / "c.jsonl")
    g0 = greedy[0]["continuation"]
    assert plain[0]["continuation"] == g0[:g0.index(eos)] and set(plain[0]) == {"prompt", "continuation", "reference"}
    assert any(len(a["continuation"]) == 6 for a in plain)  # and some rows run all their tokens
    for a, c in zip(plain, with_lp):
        assert set(c) == set(a) | {"logprobs"} and all(a[k] == c[k] for k in a)
        assert len(c["logprobs"]) == len(c["continuation"]) and all(x < 0 for x in c["logprobs"])
    for field in ("continuation", "reference"):
        log = run("run.score", "--path", str(tmp_path / "c.jsonl"), "--field", field, "--batch_size", "4",
                  "--out_path", str(tmp_path / f"{field}.jsonl"), "--keep_tokens", "true")
        total, per_row = summary(log), rows(tmp_path / f"{field}.jsonl")
        consistent(total, per_row)
        assert [r_["tokens"] for r_ in per_row] == [len(c[field]) for c in with_lp]
        if field == "continuation":  # the scores of the tokens generate chose are generate's own
            for r_, c in zip(per_row, with_lp):
                assert all(abs(x - y) <= 2e-4 for x, y in zip(r_["logprobs"], c["logprobs"]))
    # an empty field is a row of 0 tokens
    lines = open(tmp_path / "c.jsonl").read().splitlines()
    first = json.loads(lines[0])
    first["continuation"] = []
    (tmp_path / "e.jsonl").write_text("\n".join([json.dumps(first)] + lines[1:]) + "\n")
    log = run("run.score", "--path", str(tmp_path / "e.jsonl"), "--out_path", str(tmp_path / "e_out.jsonl"))
    per_row = rows(tmp_path / "e_out.jsonl")
    assert per_row[0]["tokens"] == 0 and per_row[0]["ppl"] is None
    consistent(summary(log), per_row)

    # rejected before any checkpoint is read: nothing is loaded, so no "### loading" line
    first["continuation"] = list(range(30))
    (tmp_path / "long.jsonl").write_text("\n".join(lines[:1] + [json.dumps(first)]) + "\n")
    log = run("run.score", "--path", str(tmp_path / "long.jsonl"), ok=False)
    assert "line 2" in log and "### loading" not in log
    for extra, word in ((["--prompt_len", "0"], "prompt_len"), (["--prompt_len", "32"], "prompt_len"),
                        (["--field", "prompt"], "field"),
                        (["--path", str(tmp_path / "c.jsonl"), "--split", "valid"], "--split"),
                        (["--path", str(tmp_path / "c.jsonl"), "--prompt_len", "4"], "--prompt_len")):
        log = run("run.score", *extra, ok=False)
        assert word in log and "### loading" not in log, (extra, log[-500:])
    bad = tmp_path / "diffuseq.json"
    cfg = json.load(open(ck / "training_args.json"))
    cfg["model"] = "diffuseq"
    bad.write_text(json.dumps(cfg))
    log = run("run.score", ok=False, cfg=bad)
    assert "gpt2" in log and "### loading" not in log
    for extra in (["--num_beams", "2"], ["--lookahead", "2"]):
        log = run("run.generate", *gen, "--logprobs", "true", *extra, "--out_path", str(tmp_path / "x.jsonl"), ok=False)
        assert "--logprobs" in log and "### loading" not in log
