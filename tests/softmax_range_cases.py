"""Inputs with a controlled score range for the softmax-family kernels, float64 references,
PyTorch emulations of the kernels' rounding points and a replay of the lazy-rescale rule.

Used by test_softmax_range_gpu.py; everything here is plain PyTorch and runs on any device.

Inputs are a rank-one term plus noise, so every row gets its own regime from one tensor:

    q_i = amp a_i u + 0.5 randn      k_j = amp c_j u + 0.5 randn      (u a unit vector)

so score(i, j) = S a_i c_j + noise with S = amp^2 * scale.  `a` cycles per row through A_CYCLE
(flat, ascending, descending, slow and fast rows mixed inside every 32-row wave), `c` is a
pattern over the key / vocabulary position (key_pattern)."""
import math

import torch

A_CYCLE = (0.0, 1.0, -1.0, 0.5, 2.0, -2.0, 0.25, 1.5)
LOG2E = 1.4426950408889634
LAZY_THRESHOLD = 8.0  # log2 units: the kernels rescale when a tile max exceeds the stale max by 2^8


# ---------------------------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------------------------
def key_pattern(kind, n, spikes, device="cpu"):
    """c[n] in [-1, 1].  Background on [-0.2, 1]: 'ramp' is linear over the position, 'saw' is
    half that ramp plus half a sawtooth that restarts every 192 positions (the max moves inside
    tiles and across tile edges, and keeps climbing from tooth to tooth), 'knee' climbs 11/12 of
    the range over the first 256 positions and the rest over the remainder (causal rows, which
    see only a prefix, still meet a moving max in each of their first tiles).  Every position in
    `spikes` is a single spike key at c = -1: the one dominant key of every descending row (all
    other keys >= 0.8 |a| S below it) and an exact-zero probability for every ascending row."""
    pos = torch.arange(n, dtype=torch.float64, device=device)
    ramp = 2.0 * pos / max(n - 1, 1) - 1.0
    if kind == "ramp":
        bg = ramp
    elif kind == "saw":
        bg = 0.5 * ramp + 0.5 * (2.0 * torch.remainder(pos, 192) / 191.0 - 1.0)
    elif kind == "knee":
        bg = 2.0 * ((11.0 / 12.0) * (pos / 256).clamp(max=1.0) + (pos - 256).clamp(min=0.0) / (12.0 * max(n - 256, 1))) - 1.0
    else:
        raise ValueError(kind)
    c = 0.4 + 0.6 * bg
    for s in spikes:
        if 0 <= s < n:
            c[s] = -1.0
    return c


def row_amplitudes(n, device="cpu"):
    return torch.tensor(A_CYCLE, dtype=torch.float64, device=device).repeat((n + 7) // 8)[:n]


def _unit(d, gen, device):
    u = torch.randn(d, generator=gen, dtype=torch.float64).to(device)
    return u / u.norm()


def attention_inputs(B, L, H, D, patterns, spikes, S=45.0, seed=0, device="cpu"):
    """Token-major packed qkv [B, L, 3 H D] bf16.  Item (b, h) uses patterns[i % len] and the
    spike keys spikes[i % len] with i = b H + h.  S = 45: scores within about +-100 nats."""
    gen = torch.Generator().manual_seed(seed)
    amp = math.sqrt(S * math.sqrt(D))
    a = row_amplitudes(L, device)
    qkv = torch.empty(B, L, 3, H, D, dtype=torch.float64, device=device)
    for b in range(B):
        for h in range(H):
            i = b * H + h
            c = key_pattern(patterns[i % len(patterns)], L, spikes[i % len(spikes)], device)
            u = _unit(D, gen, device)
            n = torch.randn(3, L, D, generator=gen, dtype=torch.float64).to(device)
            qkv[b, :, 0, h] = amp * a[:, None] * u + 0.5 * n[0]
            qkv[b, :, 1, h] = amp * c[:, None] * u + 0.5 * n[1]
            qkv[b, :, 2, h] = 0.7 * n[2]
    return qkv.view(B, L, 3 * H * D).bfloat16()


def ce_inputs(N, V, E, pattern, spikes, with_bias, S=100.0, seed=0, device="cpu"):
    """x [N, E], W [V, E] (bf16) and an optional bf16 bias: tokens take the role of the queries,
    vocabulary rows that of the keys.  S = 100: logits within about +-250 nats."""
    gen = torch.Generator().manual_seed(seed)  # host generator: the same draw on every device
    amp = math.sqrt(S)
    u = _unit(E, gen, device)
    a = row_amplitudes(N, device)
    c = key_pattern(pattern, V, spikes, device)
    x = amp * a[:, None] * u + 0.5 * torch.randn(N, E, generator=gen).to(device).double()
    W = amp * c[:, None] * u + 0.5 * torch.randn(V, E, generator=gen).to(device).double()
    b = torch.randn(V, generator=gen).to(device).bfloat16() if with_bias else None
    return x.bfloat16(), W.bfloat16(), b


# the host plan of csrc/vocab_sweep.h (sweep_plan), restated
def sweep_plan(N, V, target_wgs, xcd_always=False):
    tb, vchunks = (N + 127) // 128, (V + 63) // 64
    S = max(1, min(vchunks, (target_wgs + tb - 1) // tb)) if target_wgs else 1
    if xcd_always and vchunks >= 8:
        S = (S + 7) // 8 * 8
    vps = ((vchunks + S - 1) // S) * 64
    return tb, (V + vps - 1) // vps, vps


def fwd_dx_plan(N, V):
    return sweep_plan(N, V, 768)


def fwd_plan(N, V):
    return sweep_plan(N, V, 1024, xcd_always=True)


# ---------------------------------------------------------------------------------------------
# replay of the lazy-rescale rule on reference scores
# ---------------------------------------------------------------------------------------------
def lazy_replay(s2, tile):
    """s2 [R, K]: reference scores in log2 units, -inf where masked.  Replays, per row,
    `if (tile_max > m + 8) m = max(m, tile_max)` from m0 = -1e30 over tiles of `tile` columns.
    Returns (events after the first tile [R], later tiles with a visible column [R],
    underflow [R]: the row max lies in the first tile and every later visible tile is at least
    60 nats below it)."""
    R, K = s2.shape
    m = torch.full((R,), -1e30, dtype=s2.dtype, device=s2.device)
    events = torch.zeros(R, dtype=torch.long, device=s2.device)
    later = torch.zeros(R, dtype=torch.long, device=s2.device)
    later_max = torch.full((R,), -math.inf, dtype=s2.dtype, device=s2.device)
    first_max = None
    for t, k0 in enumerate(range(0, K, tile)):
        tm = s2[:, k0:k0 + tile].max(1).values
        fire = tm > m + LAZY_THRESHOLD
        m = torch.where(fire, torch.maximum(m, tm), m)
        if t == 0:
            first_max = tm
        else:
            events += fire.long()
            later += torch.isfinite(tm).long()
            later_max = torch.maximum(later_max, tm)
    underflow = (later > 0) & (later_max <= first_max - 60.0 * LOG2E)
    return events, later, underflow


def check_lazy_preconditions(sweeps, short=False, group=32):
    """sweeps: list of (s2 [R, K], tile) - one per accumulator sweep (one for attention, one per
    vocabulary split for the fused CE), all over the same R rows.  Asserts, on reference scores
    only, the conditions under which the lazy rescale is really exercised:
      1. at least a quarter of the rows rescale 3 times after the first tile in one sweep.
         short = True is for shapes where that cannot happen (a 64-row vocabulary split has one
         later subtile, a causal L = 256 row at most three later tiles): there a row with
         fewer than 3 later tiles counts when every one of them fires, and the quarter is taken
         of the rows that sweep more than one tile;
      2. every 32-row group has a row that never rescales after the first tile of any sweep
         (the wave-wide __any branch stays mixed);
      3. some row has its max in the first tile and every later tile >= 60 nats below it."""
    R = sweeps[0][0].shape[0]
    dev = sweeps[0][0].device
    qualifies = torch.zeros(R, dtype=torch.bool, device=dev)
    never = torch.ones(R, dtype=torch.bool, device=dev)
    under = torch.zeros(R, dtype=torch.bool, device=dev)
    most = torch.zeros(R, dtype=torch.long, device=dev)
    multi = torch.zeros(R, dtype=torch.bool, device=dev)
    for s2, tile in sweeps:
        events, later, uf = lazy_replay(s2, tile)
        need = later.clamp(max=3) if short else torch.full_like(later, 3)
        qualifies |= (later > 0) & (events >= need)
        never &= events == 0
        multi |= later > 0
        under |= uf
        most = torch.maximum(most, events)
    frac = qualifies.double().sum().item() / (multi.sum().item() if short else R)
    assert frac >= 0.25, f"precondition 1: only {frac:.3f} of the rows rescale often enough"
    assert R % group == 0 or R > group
    full = (R // group) * group
    per_group = never[:full].view(-1, group).any(1)
    assert bool(per_group.all()), f"precondition 2: {int((~per_group).sum())} 32-row groups have no quiet row"
    if full < R:
        assert bool(never[full:].any()), "precondition 2: the ragged last group has no quiet row"
    assert bool(under.any()), "precondition 3: no row underflows every later tile"
    return {"frac_rescaling": frac, "max_events": int(most.max()), "underflow_rows": int(under.sum())}


# ---------------------------------------------------------------------------------------------
# attention: float64 reference and emulation of the kernels' rounding points
# ---------------------------------------------------------------------------------------------
def split_heads(qkv, H, dtype):
    B, L, W = qkv.shape
    D = W // (3 * H)
    return qkv.to(dtype).view(B, L, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)  # each [B, H, L, D]


def attention_scores(qkv, H, causal, dtype=torch.float64):
    """[B, H, L, L] scores in nats (masked: -inf)."""
    q, k, _ = split_heads(qkv, H, dtype)
    L, D = q.shape[-2], q.shape[-1]
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(L, L, dtype=torch.bool, device=s.device), 1), -math.inf)
    return s


def _pack(dq, dk, dv):
    # three [B, H, L, D] -> [B, L, 3 H D]
    B, H, L, D = dq.shape
    return torch.stack((dq, dk, dv), 0).permute(1, 3, 0, 2, 4).reshape(B, L, 3 * H * D)


def attention_reference(qkv, dout, H, causal, keep=None, p=0.0):
    """float64 on the bf16-rounded inputs -> dict(out, lse, dqkv, dbias, probs)."""
    q, k, v = split_heads(qkv, H, torch.float64)
    B, _, L, D = q.shape
    s = attention_scores(qkv, H, causal)
    lse = torch.logsumexp(s, -1)
    pr = torch.exp(s - lse[..., None])
    kp = torch.ones_like(pr) if keep is None else keep.double() / (1.0 - p)
    pd = pr * kp
    o = pd @ v
    do = dout.double().view(B, L, H, D).permute(0, 2, 1, 3)
    dv = pd.transpose(-1, -2) @ do
    dpd = (do @ v.transpose(-1, -2)) * kp
    delta = (do * o).sum(-1, keepdim=True)
    ds = pr * (dpd - delta)
    dq = ds @ k / math.sqrt(D)
    dk = ds.transpose(-1, -2) @ q / math.sqrt(D)
    dqkv = _pack(dq, dk, dv)
    return {"out": o.permute(0, 2, 1, 3).reshape(B, L, H * D), "lse": lse, "dqkv": dqkv,
            "dbias": dqkv.sum((0, 1)), "probs": pr}


def attention_emulation(qkv, dout, H, causal, keep=None, p=0.0):
    """The same operation with the kernels' rounding points: fp32 scores and statistics, bf16
    probabilities and dS as matrix-core operands, fp32 accumulation, bf16 outputs, delta from
    the bf16 output.  Accumulation order is not reproduced (the factor 2 on its error is)."""
    q, k, v = split_heads(qkv, H, torch.float32)
    B, _, L, D = q.shape
    s = attention_scores(qkv, H, causal).float()
    lse = torch.logsumexp(s, -1)
    pr = torch.exp(s - lse[..., None])
    kp = torch.ones_like(pr) if keep is None else keep.float() / (1.0 - p)
    pb = (pr * kp).bfloat16().float()
    o = (pb @ v).bfloat16().float()
    do = dout.float().view(B, L, H, D).permute(0, 2, 1, 3)
    dv = (pb.transpose(-1, -2) @ do).bfloat16()
    dpd = (do @ v.transpose(-1, -2)) * kp
    delta = (do * o).sum(-1, keepdim=True)
    ds = (pr * (dpd - delta)).bfloat16().float()
    dq = ((ds @ k) / math.sqrt(D)).bfloat16()
    dk = ((ds.transpose(-1, -2) @ q) / math.sqrt(D)).bfloat16()
    dqkv = _pack(dq, dk, dv)
    return {"out": o.permute(0, 2, 1, 3).reshape(B, L, H * D), "lse": lse, "dqkv": dqkv.float(),
            "dbias": dqkv.float().sum((0, 1))}


# ---------------------------------------------------------------------------------------------
# fused linear + cross-entropy: float64 reference and emulation
# ---------------------------------------------------------------------------------------------
def ce_logits(x, W, b, dtype=torch.float64):
    lg = x.to(dtype) @ W.to(dtype).t()
    if b is not None:
        lg += b.to(dtype)
    return lg


def ce_reference(x, W, b, tgt, g):
    """float64 on the bf16-rounded inputs.  Targets outside [0, V) are ignored."""
    V = W.shape[0]
    valid = (tgt >= 0) & (tgt < V)
    tc = tgt.clamp(0, V - 1)
    lg = ce_logits(x, W, b)
    lse = torch.logsumexp(lg, -1)
    loss = torch.where(valid, lse - lg.gather(1, tc[:, None])[:, 0], torch.zeros_like(lse))
    pr = lg.sub_(lse[:, None]).exp_()  # in place: [N, V] float64 is the large tensor here
    Wd, xd = W.double(), x.double()
    dxu = (pr @ Wd - Wd[tc]) * valid[:, None]
    gv = g.double() * valid
    pr.mul_(gv[:, None])
    pr[torch.arange(len(tc), device=tc.device), tc] -= gv
    return {"loss": loss, "lse": lse, "dxu": dxu, "dx": dxu * gv[:, None], "dW": pr.t() @ xd, "db": pr.sum(0)}


def ce_emulation(x, W, b, tgt, g):
    """fp32 logits and statistics, bf16 probabilities / dS as matrix-core operands, fp32
    accumulation, bf16 dx (fp32 dxu, dW, db)."""
    V = W.shape[0]
    valid = (tgt >= 0) & (tgt < V)
    tc = tgt.clamp(0, V - 1)
    Wf, xf = W.float(), x.float()
    lg = ce_logits(x, W, b, torch.float32)
    mx = lg.max(-1).values
    un = (lg - mx[:, None]).exp_()
    l = un.sum(-1)
    lse = mx + l.log()
    loss = torch.where(valid, lse - lg.gather(1, tc[:, None])[:, 0], torch.zeros_like(lse))
    dxu = ((un.bfloat16().float() @ Wf) / l[:, None] - Wf[tc]) * valid[:, None]
    gv = g.float() * valid
    ds = (lg - lse[:, None]).exp_().mul_(gv[:, None])
    ds[torch.arange(len(tc), device=tc.device), tc] -= gv
    db = ds.sum(0)
    dsb = ds.bfloat16().float()
    return {"loss": loss, "lse": lse, "dxu": dxu, "dxu_g": dxu * gv[:, None], "dx": (dsb @ Wf).bfloat16().float(),
            "dW": dsb.t() @ xf, "db": db}


# ---------------------------------------------------------------------------------------------
# comparison: assert_close semantics with an emulation-derived fallback tolerance
# ---------------------------------------------------------------------------------------------
def excess(actual, ref, rtol):
    """max(|actual - ref| - rtol |ref|): the smallest atol with which assert_close would pass."""
    a, r = actual.double(), ref.double()
    return ((a - r).abs() - rtol * r.abs()).max().item()
