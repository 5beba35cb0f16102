"""GPT-2 small causal LM (BASELINE config #4: the generic-model path).

Trained through the *generic* ``TrainLoop`` hooks (``compute_losses`` /
``backward_from_losses``) rather than the diffusion loop.  Weight tying
``lm_head.weight is wte.weight``; the LM loss uses the fused
linear-cross-entropy op so the [tokens, 50257] logits never exist in memory.
"""
import torch
from torch import nn

from ..ops import nn as ops
from . import presets
from .layers import Embedding, GPT2Block, LayerNorm


def _logit_processors(repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram, min_new_tokens,
                      eos_id):
    """-> (the scalar keywords of ``ops.decode.penalize_logits_``, or None with all four at their
    defaults; ``min_new_tokens`` as an int), checked."""
    kw = dict(repetition_penalty=float(repetition_penalty), presence_penalty=float(presence_penalty),
              frequency_penalty=float(frequency_penalty), no_repeat_ngram=int(no_repeat_ngram))
    if not kw["repetition_penalty"] > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
    if kw["no_repeat_ngram"] < 0:
        raise ValueError(f"no_repeat_ngram must be >= 0, got {no_repeat_ngram}")
    M = int(min_new_tokens)
    if M < 0:
        raise ValueError(f"min_new_tokens must be >= 0, got {min_new_tokens}")
    if M > 0 and eos_id is None:
        raise ValueError("min_new_tokens holds off eos_id: it needs one")
    if kw == dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0):
        kw = None
    return kw, M


class GPT2LMModel(nn.Module):
    def __init__(self, *, config_name="gpt2", vocab_size=0, seq_len=1024, hidden_size=0,
                 num_layers=0, num_heads=0, dropout=0.1, compute_dtype=torch.bfloat16, **_):
        super().__init__()
        cfg = presets.resolve(config_name, hidden_size=hidden_size, num_layers=num_layers,
                              num_heads=num_heads, vocab_size=vocab_size)
        H = cfg["hidden_size"]
        self.cfg, self.compute_dtype, self.dropout = cfg, compute_dtype, dropout
        assert seq_len <= cfg["max_position_embeddings"]
        self.wte = Embedding(cfg["vocab_size"], H, init_std=0.02)
        self.wpe = Embedding(cfg["max_position_embeddings"], H, init_std=0.01)
        self.h = nn.ModuleList(GPT2Block(H, cfg["num_heads"], dropout, eps=cfg["layer_norm_eps"],
                                         n_layers=cfg["num_layers"]) for _ in range(cfg["num_layers"]))
        self.ln_f = LayerNorm(H, eps=cfg["layer_norm_eps"])
        self.register_buffer("position_ids", torch.arange(cfg["max_position_embeddings"]).unsqueeze(0),
                             persistent=False)

    def hidden_states(self, input_ids):
        dt = self.compute_dtype
        B, L = input_ids.shape
        # every residual add (and the embedding sum + dropout) runs fused with the
        # LayerNorm that reads it: x = x + dropout(branch), a = LN_next(x) in one kernel
        lns = [blk.ln_1 for blk in self.h] + [self.ln_f]
        x, a = ops.residual_layernorm(self.wte(input_ids, dt), None, lns[0].weight, lns[0].bias,
                                      self.dropout, lns[0].eps, self.training,
                                      pos=self.wpe(self.position_ids[:, :L], dt))
        for i, blk in enumerate(self.h):
            x, h = blk(x, a)
            x, a = ops.residual_layernorm(h, x, lns[i + 1].weight, lns[i + 1].bias, self.dropout,
                                          lns[i + 1].eps, self.training)
        return a

    def forward(self, input_ids, labels=None):
        """Returns per-token CE [B, L-1] when ``labels`` (shifted internally) are given."""
        h = self.hidden_states(input_ids)
        if labels is None:
            return ops.linear(h, self.wte.weight)
        B, L, H = h.shape
        x = h[:, :-1].reshape(-1, H)
        tgt = labels[:, 1:].reshape(-1)
        return ops.linear_cross_entropy(x, self.wte.weight, None, tgt).view(B, L - 1)

    # ---- generation: K/V cache, prefill, one-token decode steps (inference only) ----------

    def init_cache(self, batch, max_len, device=None, dtype=None, kv_dtype="bf16"):
        """An empty cache for ``batch`` rows of up to ``max_len`` tokens (prompt + continuation).
        ``kv_dtype="fp8"``: the one-byte cache of ``ops.decode`` - e4m3fn codes and one int8 exponent per
        cached row - for :meth:`prefill`, :meth:`decode_step` and :meth:`generate`; ``"bf16"`` (the
        default) stores the values in ``dtype`` (the compute dtype)."""
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        cfg = self.cfg
        if not 1 <= max_len <= cfg["max_position_embeddings"]:
            raise ValueError(f"max_len {max_len} outside 1 .. max_position_embeddings "
                             f"{cfg['max_position_embeddings']}")
        device = self.wte.weight.device if device is None else device
        dtype = self.compute_dtype if dtype is None else dtype
        return KVCache(len(self.h), batch, cfg["num_heads"], max_len, cfg["hidden_size"] // cfg["num_heads"],
                       device, dtype, kv_dtype=kv_dtype)

    def _blocks(self, x, a, attend):
        """The block stack of ``hidden_states`` in eval mode with ``attend(i, qkv)`` as layer i's
        attention over its packed projection -> ln_f of the last residual stream."""
        lns = [blk.ln_1 for blk in self.h] + [self.ln_f]
        for i, blk in enumerate(self.h):
            h = blk.attn_proj(attend(i, blk.attn.qkv(a)))
            x, a = ops.residual_layernorm(h, x, blk.ln_2.weight, blk.ln_2.bias, 0.0, blk.ln_2.eps, False)
            x, a = ops.residual_layernorm(ops.mlp(a, blk.mlp_fc, blk.mlp_proj), x, lns[i + 1].weight,
                                          lns[i + 1].bias, 0.0, lns[i + 1].eps, False)
        return a

    @torch.no_grad()
    def prefill(self, input_ids, lens, cache):
        """Right-padded prompts ``input_ids`` [B, Lp] of ``1 <= lens[b] <= Lp`` tokens: one causal
        forward (what stands behind a row's prompt never reaches it), each layer's K and V of the
        prompt positions copied into ``cache`` (quantized into an fp8 cache; the prompt's own forward
        attends over the unquantized values), ``cache.lens = lens`` -> the logits [B, V] at each row's
        last prompt position."""
        dt = self.compute_dtype
        B, Lp = input_ids.shape
        if Lp > cache.max_len or B != cache.batch:
            raise ValueError(f"prompts [{B}, {Lp}] do not fit a cache of {cache.batch} rows x {cache.max_len}")
        lens = lens.to(device=input_ids.device, dtype=torch.int32)
        L = Lp
        if input_ids.is_cuda and dt == torch.bfloat16 and Lp % 64:
            # ops.attention's kernels take L % 64 == 0: pad on the right, which causality hides
            L = min(-(-Lp // 64) * 64, self.cfg["max_position_embeddings"])
            input_ids = torch.nn.functional.pad(input_ids, (0, L - Lp))
        heads, D = cache.heads, cache.head_dim
        inside = (torch.arange(Lp, device=input_ids.device).view(1, Lp) < lens.view(B, 1)).view(B, 1, Lp, 1)
        if cache.fp8:
            from ..ops.decode import kv_store

        def attend(i, qkv):
            if cache.fp8:  # one quantizing store per layer; positions at or beyond lens stay untouched
                kv_store(qkv.view(B, L, -1)[:, :Lp], lens, cache.k[i], cache.ke[i], cache.v[i], cache.ve[i])
                return ops.attention(qkv, heads, 0.0, True, False)
            kv = qkv.view(B, L, 3, heads, D)[:, :Lp].permute(2, 0, 3, 1, 4)  # [3, B, H, Lp, D]
            for dst, src in ((cache.k[i], kv[1]), (cache.v[i], kv[2])):
                dst[:, :, :Lp] = torch.where(inside, src.to(dst.dtype), dst[:, :, :Lp])
            return ops.attention(qkv, heads, 0.0, True, False)

        ln0 = self.h[0].ln_1
        x, a = ops.residual_layernorm(self.wte(input_ids, dt), None, ln0.weight, ln0.bias, 0.0, ln0.eps, False,
                                      pos=self.wpe(self.position_ids[:, :L], dt))
        a = self._blocks(x, a, attend)
        cache.lens = lens.clone()
        last = a[torch.arange(B, device=a.device), (lens.long() - 1).clamp(0, Lp - 1)]
        return ops.linear(last, self.wte.weight)

    @torch.no_grad()
    def decode_step(self, tokens, cache, table=None):
        """One token per row at position ``cache.lens[b]`` -> the next-token logits [B, V];
        ``cache.lens`` advances on the device.  A parked row (``lens`` outside 0 .. max_len - 1)
        does no cache work, keeps its ``lens``, and its logits mean nothing.  ``table``: a pair
        ``(src uint8 [B, max_len], beams)`` handed to ``attention_decode`` - the rows are groups
        of ``beams`` slots that read their cached keys through ``src`` (beam search; not over an
        fp8 cache).  Over an fp8 cache the step is ``ops.decode.attention_decode_fp8``."""
        from ..ops.decode import attention_decode, attention_decode_fp8
        if cache.fp8 and table is not None:
            raise ValueError("an fp8 cache has no indirection-table variant: beam search needs kv_dtype='bf16'")
        dt = self.compute_dtype
        B = tokens.shape[0]
        heads = cache.heads
        pos = cache.lens.long().clamp(0, self.cfg["max_position_embeddings"] - 1)
        # the B rows stand where hidden_states has the L positions of one sequence, so the
        # embedding sum and every LayerNorm run in the kernels (and roundings) of the full forward
        ln0 = self.h[0].ln_1
        x, a = ops.residual_layernorm(self.wte(tokens.view(1, B), dt), None, ln0.weight, ln0.bias, 0.0, ln0.eps,
                                      False, pos=self.wpe(pos, dt))

        kw = {} if table is None else {"src": table[0], "beams": table[1]}

        def attend(i, qkv):
            if cache.fp8:
                return attention_decode_fp8(qkv.view(B, -1), cache.k[i], cache.ke[i], cache.v[i], cache.ve[i],
                                            cache.lens, heads).view(1, B, -1)
            return attention_decode(qkv.view(B, -1), cache.k[i], cache.v[i], cache.lens, heads, **kw).view(1, B, -1)

        a = self._blocks(x, a, attend)
        cache.lens += ((cache.lens >= 0) & (cache.lens < cache.max_len)).to(cache.lens.dtype)
        return ops.linear(a.view(B, -1), self.wte.weight)

    @torch.no_grad()
    def generate(self, input_ids, lens, max_new_tokens, *, temperature=1.0, top_k=0, top_p=0.0, eos_id=None,
                 generator=None, cache=None, check_every=16, noise_seed=None, row_base=0, repetition_penalty=1.0,
                 presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0, min_new_tokens=0,
                 penalize_prompt=True, return_logprobs=False, kv_dtype=None):
        """Continue right-padded prompts -> (tokens [B, max_new_tokens], new_lens [B]).

        ``temperature == 0`` is greedy (ties to the lowest id); otherwise ``logits / temperature``,
        ``top_k``, ``top_p``, one draw with ``generator`` (utils/lm_sampling.py) - or, with an
        integer ``noise_seed``, step t draws with ``ops.decode.sample_tokens(..., seed=noise_seed,
        step=t, row_base=row_base)``: counter-based noise keyed by (seed, step, ``row_base`` + b, id),
        the same for a row in whatever batch it stands, and ``generator`` is not touched.  A row stops when
        it has emitted ``eos_id`` or its cache is full: it is parked (``cache.lens[b] = -1``, no
        further cache work) and the rest of its output row is ``eos_id`` (0 without one).
        ``new_lens[b]`` counts the tokens the row really produced, a closing ``eos_id`` included.
        ``cache``: one from :meth:`init_cache` to use (default: a new one of just the size needed).
        ``kv_dtype``: "bf16" or "fp8" - the one-byte cache, half the bytes per cached token - for
        the new cache (default "bf16"); given together with a ``cache`` of the other kind it is an
        error.
        The loop runs on the device; the host looks at it once every ``check_every`` steps (0:
        never), to stop early when every row has finished.

        Logit processors.  With any of ``repetition_penalty``, ``presence_penalty``,
        ``frequency_penalty`` and ``no_repeat_ngram`` off its default, the loop keeps each row's
        prompt and output so far on the device and every step's logits, the prefill's included, go
        through ``ops.decode.penalize_logits_`` before the token is chosen; ``penalize_prompt=False``
        leaves the prompt out of the window (``start = lens``).  ``min_new_tokens = M`` sets the
        ``eos_id`` logit of a row that has produced fewer than M tokens to -inf first.  With all at
        their defaults the loop is, call for call, the one without them.

        ``return_logprobs=True`` adds a third result, ``logprobs`` fp32 [B, max_new_tokens]: entry t is
        the log-probability of the token chosen at step t under the step's processed logits - after
        ``min_new_tokens`` and the penalties, before temperature, ``top_k`` and ``top_p`` - as
        ``ops.decode.token_stats`` gives it, and 0 from the step a row is done.  Tokens and lengths are
        those of the call without it."""
        from utils.lm_sampling import sample_next
        from ..ops.decode import penalize_logits_, sample_tokens, token_stats
        penalties, min_new = _logit_processors(repetition_penalty, presence_penalty, frequency_penalty,
                                               no_repeat_ngram, min_new_tokens, eos_id)
        philox = noise_seed is not None and temperature > 0
        B, Lp = input_ids.shape
        dev = input_ids.device
        if kv_dtype not in (None, "bf16", "fp8"):
            raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        if cache is None:
            cache = self.init_cache(B, min(Lp + max_new_tokens, self.cfg["max_position_embeddings"]), dev,
                                    **({"kv_dtype": "fp8"} if kv_dtype == "fp8" else {}))
        elif kv_dtype is not None and (kv_dtype == "fp8") != cache.fp8:
            raise ValueError(f"kv_dtype={kv_dtype!r} contradicts the given cache, which is "
                             f"{'fp8' if cache.fp8 else 'bf16'}")
        fill = 0 if eos_id is None else int(eos_id)
        out = torch.full((B, max_new_tokens), fill, dtype=torch.long, device=dev)
        new_lens = torch.zeros(B, dtype=torch.long, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        logprobs = torch.zeros(B, max_new_tokens, dtype=torch.float32, device=dev) if return_logprobs else None
        if penalties is not None:
            # a row's prompt and output so far: hist[b, :n[b]]; a new token lands on the padding
            hist = torch.zeros(B, Lp + max_new_tokens, dtype=torch.int32, device=dev)
            hist[:, :Lp] = input_ids
            n = lens.to(device=dev, dtype=torch.int32).clone()
            start = None if penalize_prompt else n.clone()
        logits = self.prefill(input_ids, lens, cache)
        for t in range(max_new_tokens):
            if t < min_new:
                logits[:, fill] = float("-inf")  # every live row has produced t tokens
            if penalties is not None:
                penalize_logits_(logits, hist, n, start=start, **penalties)
            if philox:
                tok = sample_tokens(logits, temperature=temperature, top_k=top_k, top_p=top_p, seed=int(noise_seed),
                                    step=t, row_base=row_base)
            else:
                tok = sample_next(logits, temperature, top_k, top_p, generator)
            if return_logprobs:
                logprobs[:, t] = token_stats(logits, torch.where(done, -1, tok))[0]  # a done row: "ignore", 0
            tok = torch.where(done, fill, tok)
            out[:, t] = tok
            if penalties is not None:
                hist.scatter_(1, n.long().view(B, 1), tok.to(torch.int32).view(B, 1))
                n += 1
            new_lens += (~done).to(new_lens.dtype)
            if eos_id is not None:
                done = done | (tok == fill)
            done = done | (cache.lens >= cache.max_len)  # no room to run this token
            if t + 1 == max_new_tokens:
                break
            cache.lens.masked_fill_(done, -1)
            if check_every and (t + 1) % check_every == 0 and bool(done.all()):
                break
            logits = self.decode_step(tok, cache)
        cache.lens.masked_fill_(done, -1)
        return (out, new_lens, logprobs) if return_logprobs else (out, new_lens)

    # ---- teacher-forced scoring (inference only) -----------------------------------------

    @torch.no_grad()
    def score(self, input_ids, lens=None, *, start=None):
        """Teacher-forced statistics of every scored token of right-padded ``input_ids`` [B, L] -> a
        dict of [B, L - 1] tensors whose column j speaks of token ``input_ids[b, j + 1]`` given the
        tokens in front of it: ``logp`` fp32 (its log-probability, nats), ``rank`` int32 (its 0-based
        place among the V ids, ties by id), ``entropy`` fp32 (of the model's distribution there),
        ``top1`` int64 (the model's arg-max) and ``mask`` bool.

        Position ``p = j + 1`` is scored iff ``max(start[b], 1) <= p < lens[b]``; ``start`` defaults to
        1 (everything but the first token) and ``lens`` to L, and a value outside ``[0, L]`` raises.
        Outside the mask ``logp = 0``, ``rank = -1``, ``entropy = 0`` and ``top1 = -1``, and ids at or
        behind ``lens[b]`` are never looked at.

        One causal forward in eval behaviour whatever ``self.training`` is (the stack of
        :meth:`prefill`; on the native bf16 path L is padded to a multiple of 64, which causality
        hides), then only the hidden rows inside the mask go through the head: chunks of at most
        256 MiB of logits, ``ops.linear`` and ``ops.decode.token_stats`` each.  The positions are
        gathered with one ``nonzero`` (a host synchronisation)."""
        from ..ops.decode import token_stats
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B, L], got {tuple(input_ids.shape)}")
        B, L = input_ids.shape
        dev = input_ids.device
        if L > self.cfg["max_position_embeddings"]:
            raise ValueError(f"L = {L} exceeds max_position_embeddings {self.cfg['max_position_embeddings']}")

        def bound(x, default, name):
            if x is None:
                return torch.full((B,), default, dtype=torch.long, device=dev)
            x = torch.as_tensor(x, device=dev)
            if x.is_floating_point() or x.dtype == torch.bool or tuple(x.shape) != (B,):
                raise ValueError(f"{name} must hold {B} integers, got {x.dtype} {tuple(x.shape)}")
            x = x.long()
            if B and bool(((x < 0) | (x > L)).any()):
                raise ValueError(f"{name} must lie in 0 .. L = {L}")
            return x

        lens, start = bound(lens, L, "lens"), bound(start, 1, "start")
        n = max(L - 1, 0)
        res = {"logp": torch.zeros(B, n, dtype=torch.float32, device=dev),
               "rank": torch.full((B, n), -1, dtype=torch.int32, device=dev),
               "entropy": torch.zeros(B, n, dtype=torch.float32, device=dev),
               "top1": torch.full((B, n), -1, dtype=torch.long, device=dev),
               "mask": torch.zeros(B, n, dtype=torch.bool, device=dev)}
        if B == 0 or n == 0:
            return res
        p = torch.arange(1, L, device=dev).view(1, n)
        mask = (p >= start.clamp(min=1).view(B, 1)) & (p < lens.view(B, 1))
        res["mask"] = mask
        bi, ji = mask.nonzero(as_tuple=True)
        if bi.numel() == 0:
            return res

        dt = self.compute_dtype
        # what stands at or behind lens[b] is padding of any content: it never reaches the embedding
        ids = torch.where(torch.arange(L, device=dev).view(1, L) < lens.view(B, 1), input_ids, 0)
        Lr = L
        if ids.is_cuda and dt == torch.bfloat16 and L % 64:
            # ops.attention's kernels take L % 64 == 0: pad on the right, which causality hides
            Lr = min(-(-L // 64) * 64, self.cfg["max_position_embeddings"])
            ids = torch.nn.functional.pad(ids, (0, Lr - L))
        heads = self.cfg["num_heads"]
        ln0 = self.h[0].ln_1
        x, a = ops.residual_layernorm(self.wte(ids, dt), None, ln0.weight, ln0.bias, 0.0, ln0.eps, False,
                                      pos=self.wpe(self.position_ids[:, :Lr], dt))
        a = self._blocks(x, a, lambda i, qkv: ops.attention(qkv, heads, 0.0, True, False))

        rows = a[bi, ji]                 # [N, H]: the hidden state in front of each scored token
        tgt = input_ids[bi, ji + 1]
        V = self.wte.weight.shape[0]
        step = max(1, (256 << 20) // (V * rows.element_size()))
        for r0 in range(0, rows.shape[0], step):
            logits = ops.linear(rows[r0:r0 + step], self.wte.weight)
            lp, rk, en, t1 = token_stats(logits, tgt[r0:r0 + step])
            at = (bi[r0:r0 + step], ji[r0:r0 + step])
            res["logp"][at], res["rank"][at], res["entropy"][at], res["top1"][at] = lp, rk, en, t1.long()
        return res

    @torch.no_grad()
    def decode_block(self, tokens, cache, counts=None):
        """T tokens per row, token j of row b at position ``cache.lens[b] + j`` -> logits [B, T, V],
        the logits at j saying what follows token j.  ``counts`` (int [B], default T): how many of a
        row's tokens are real - ``ops.decode.attention_decode_block`` has the exact rule; the logits of
        the others mean nothing and their keys are not stored.  ``cache.lens`` is NOT advanced: the
        caller commits as many positions as it accepted, and what was stored beyond them is
        overwritten or never read."""
        from ..ops.decode import attention_decode_block
        if cache.fp8:
            raise ValueError("decode_block has no fp8 variant: lookahead decoding needs kv_dtype='bf16'")
        dt = self.compute_dtype
        B, T = tokens.shape
        heads = cache.heads
        pos = cache.lens.long().view(B, 1) + torch.arange(T, device=tokens.device).view(1, T)
        pos = pos.clamp(0, self.cfg["max_position_embeddings"] - 1).view(-1)
        if counts is not None:
            counts = counts.to(torch.int32)
        # the B T tokens stand where decode_step has its B rows: the same kernels around the attention
        ln0 = self.h[0].ln_1
        x, a = ops.residual_layernorm(self.wte(tokens.reshape(1, B * T), dt), None, ln0.weight, ln0.bias, 0.0,
                                      ln0.eps, False, pos=self.wpe(pos, dt))

        def attend(i, qkv):
            return attention_decode_block(qkv.view(B, T, -1), cache.k[i], cache.v[i], cache.lens, heads,
                                          counts=counts).view(1, B * T, -1)

        a = self._blocks(x, a, attend)
        return ops.linear(a.view(B * T, -1), self.wte.weight).view(B, T, -1)

    @torch.no_grad()
    def generate_lookahead(self, input_ids, lens, max_new_tokens, *, lookahead, ngram=2, eos_id=None, cache=None,
                           check_every=4, draft=None, return_stats=False, repetition_penalty=1.0,
                           presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0, min_new_tokens=0,
                           penalize_prompt=True):
        """Greedy continuation by lookahead decoding -> (tokens [B, max_new_tokens], new_lens [B]),
        with the meanings of :meth:`generate`: its ``temperature=0`` result wherever every arg-max on
        the way is the same in both, in fewer model calls.

        One iteration runs ``T = lookahead`` tokens per row through :meth:`decode_block`: the row's
        last committed token and T - 1 guesses, by default copied from the row's own history
        (``ops.decode.lookup_draft`` with ``ngram``).  The logits at block position j say what follows
        token j, so the longest prefix of guesses that equal the arg-max in front of them is accepted
        and the arg-max behind it comes free: a row emits 1 .. T tokens per call, cut behind the first
        ``eos_id``.  A row's block is cut to what its cache and ``max_new_tokens`` leave room for.
        Keys stored for rejected guesses lie at or beyond ``cache.lens`` and are overwritten or never
        read.  Rows finish and are parked as in :meth:`generate` (a row that used up
        ``max_new_tokens`` has not run its last token); there are at most ``max_new_tokens - 1``
        iterations, all on the device, and the host looks once every ``check_every`` iterations (0:
        never) to stop when every row has finished.

        ``draft``: a callable with ``lookup_draft``'s signature ``(history [B, Lh], n [B], *, ngram,
        max_draft) -> (draft [B, max_draft], k [B])`` to use instead - ``history[b, :n[b]]`` is the
        row's prompt and output so far.  ``return_stats`` adds a dict: ``model_calls`` (iterations with
        a live row), ``proposed`` and ``accepted`` guesses, read back once at the end.

        The logit processors of :meth:`generate` are not available here: the guesses continue
        repeated n-grams, which is what those penalties forbid, and the queries of a block would
        each need a history of their own.  Any non-default value raises ``ValueError``."""
        from utils.lm_sampling import greedy
        from ..ops.decode import lookup_draft
        if ((repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram, min_new_tokens) != (1.0, 0.0, 0.0, 0, 0)
                or penalize_prompt is not True):
            raise ValueError("lookahead decoding does not take logit penalties, no_repeat_ngram, min_new_tokens or "
                             "penalize_prompt: use generate")
        T, g, N = int(lookahead), int(ngram), int(max_new_tokens)
        if not 2 <= T <= 8:
            raise ValueError(f"lookahead must be in 2 .. 8, got {lookahead}")
        if g < 1:
            raise ValueError(f"ngram must be >= 1, got {ngram}")
        draft = lookup_draft if draft is None else draft
        B, Lp = input_ids.shape
        dev = input_ids.device
        if cache is None:
            cache = self.init_cache(B, min(Lp + N, self.cfg["max_position_embeddings"]), dev)
        elif cache.fp8:
            raise ValueError("generate_lookahead needs a bf16 cache: the block decode kernel has no fp8 variant")
        max_len = cache.max_len
        fill = 0 if eos_id is None else int(eos_id)
        # T spare columns behind both: where the masked-out slots of a block are written
        out = torch.full((B, N + T), fill, dtype=torch.long, device=dev)
        Lh = Lp + N
        hist = torch.zeros(B, Lh + T, dtype=torch.long, device=dev)
        n = lens.to(device=dev, dtype=torch.long).clone()  # tokens of the row's history
        hist[:, :Lp] = torch.where(torch.arange(Lp, device=dev).view(1, Lp) < n.view(B, 1), input_ids, 0)
        new_lens = torch.zeros(B, dtype=torch.long, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        stats = torch.zeros(3, dtype=torch.long, device=dev)  # model calls, proposed, accepted
        logits = self.prefill(input_ids, lens, cache)
        if N == 0:
            res = (out[:, :0], new_lens)
            return res + ({"model_calls": 0, "proposed": 0, "accepted": 0},) if return_stats else res
        last = greedy(logits)
        out[:, 0] = last
        hist.scatter_(1, n.view(B, 1), last.view(B, 1))
        n += 1
        new_lens += 1
        if eos_id is not None:
            done = done | (last == fill)
        pos = cache.lens.clone()  # a row's cached tokens, while cache.lens parks the rows with nothing to run
        done = done | (pos >= max_len)
        idle = done | (new_lens >= N)
        cols = torch.arange(T, device=dev).view(1, T)
        for it in range(N - 1):
            cache.lens.copy_(torch.where(idle, -1, pos))
            if check_every and it and it % check_every == 0 and bool(idle.all()):
                break
            guess, k = draft(hist[:, :Lh], n, ngram=g, max_draft=T - 1)
            counts = torch.minimum(torch.minimum(1 + k.long(), max_len - pos.long()), N - new_lens)
            counts = torch.where(idle, 0, counts).clamp(min=0)
            block = torch.cat([last.view(B, 1), guess], 1)
            logits = self.decode_block(block, cache, counts)
            picks = greedy(logits.view(B * T, -1)).view(B, T)
            # a: the guesses accepted - the longest prefix with block[j + 1] == picks[j], j + 1 < counts
            match = (block[:, 1:] == picks[:, :-1]) & (cols[:, 1:] < counts.view(B, 1))
            a = match.long().cumprod(1).sum(1)
            keep = (cols <= a.view(B, 1)) & ~idle.view(B, 1)
            if eos_id is not None:  # nothing behind the first eos_id
                is_eos = keep & (picks == fill)
                keep = keep & (is_eos.long().cumsum(1) - is_eos.long() == 0)
            e = keep.long().sum(1)  # tokens emitted: 1 .. a + 1 for a live row
            out.scatter_(1, torch.where(keep, new_lens.view(B, 1) + cols, N + cols), picks)
            hist.scatter_(1, torch.where(keep, n.view(B, 1) + cols, Lh + cols), picks)
            last = torch.where(idle, last, picks.gather(1, (e - 1).clamp(min=0).view(B, 1)).view(B))
            stats += torch.stack([(~idle).any().long(), (counts - 1).clamp(min=0).sum(),
                                  torch.where(idle, 0, a).sum()])
            new_lens += e
            n += e
            pos += e.to(pos.dtype)
            if eos_id is not None:
                done = done | (keep & (picks == fill)).any(1)
            done = done | (pos >= max_len)  # no room to run the last token emitted
            idle = done | (new_lens >= N)
        cache.lens.copy_(torch.where(done, -1, pos))
        res = (out[:, :N].contiguous(), new_lens)
        if return_stats:
            calls, proposed, accepted = stats.tolist()
            res += ({"model_calls": calls, "proposed": proposed, "accepted": accepted},)
        return res

    @torch.no_grad()
    def beam_search(self, input_ids, lens, max_new_tokens, *, num_beams, eos_id=None, length_penalty=0.0,
                    cache=None, check_every=16, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                    no_repeat_ngram=0, min_new_tokens=0, penalize_prompt=True):
        """Continue right-padded prompts with beam search -> (tokens [B, W, max_new_tokens], new_lens
        [B, W], scores fp32 [B, W]), ``W = num_beams``, the beams of a prompt best first.

        The cache has ``B W`` rows, row ``b W + w`` being slot w of prompt b.  The prompts are
        prefilled once, into slot 0 of each group; a uint8 table [B, W, max_len] names, per slot and
        position, the slot that holds the key (``ops.decode.attention_decode``'s ``src``), starts as
        zeros - every beam reads the one copy of the prompt - and is what a step re-parents instead
        of the cache.  Step t: ``ops.decode.beam_step`` on the current logits; the next table is the
        parents' rows with the position of the last append pointing at the parent; finished and
        non-existent slots are parked; one ``decode_step`` through the table.

        The search ranks by the cumulative log-probability alone, ``beam_step``'s fp32 sums (a
        finished beam keeps its score and its place).  The returned ``scores`` are the raw sums of
        the hypotheses' log-probabilities - ``beam_step``'s ``logp`` terms added up in float64 and
        rounded to fp32 once, so they do not carry the rounding of every fp32 addition - and the
        returned order is by ``scores / max(new_lens, 1) ** length_penalty`` (0: the raw sum), ties
        to the lower slot.  As in
        :meth:`generate`, a beam stops at ``eos_id`` or when the cache is full, the rest of its row
        is ``eos_id`` (0 without one), ``new_lens`` counts a closing ``eos_id``, and the host looks
        at the loop once every ``check_every`` steps (0: never).  A slot that never held a
        hypothesis (fewer than W candidates) has score -inf, length 0 and a row of fill.

        The logit processors of :meth:`generate`, with the same keywords: every beam has a history
        row of its own, re-ordered by ``parent`` with one gather per step and extended at the group's
        common position, and ``ops.decode.penalize_logits_`` runs on every step's logits before
        ``beam_step`` (finished and non-existent slots are passed as parked rows).  The first step's
        logits are one row per prompt repeated for every beam, so they are penalised once, before
        they are expanded.  The scores are sums of the log-softmax of the processed logits."""
        from ..ops.decode import beam_step, penalize_logits_
        penalties, min_new = _logit_processors(repetition_penalty, presence_penalty, frequency_penalty,
                                               no_repeat_ngram, min_new_tokens, eos_id)
        W = int(num_beams)
        if not 1 <= W <= 255:
            raise ValueError(f"num_beams must be in 1 .. 255, got {num_beams}")
        B, Lp = input_ids.shape
        dev = input_ids.device
        T = int(max_new_tokens)
        if cache is None:
            cache = self.init_cache(B * W, min(Lp + T, self.cfg["max_position_embeddings"]), dev)
        elif cache.fp8:
            raise ValueError("beam_search needs a bf16 cache: the table decode kernel has no fp8 variant")
        elif cache.batch != B * W:
            raise ValueError(f"beam search over {B} prompts x {W} beams needs a cache of {B * W} rows, "
                             f"got {cache.batch}")
        Lmax = cache.max_len
        fill = 0 if eos_id is None else int(eos_id)
        eos = -1 if eos_id is None else int(eos_id)
        ninf = float("-inf")

        logits = self.prefill(input_ids, lens, cache.slot_view(W, 0))  # the prompts, once, into slot 0
        if min_new > 0:
            logits[:, fill] = ninf
        if penalties is not None:
            Lh = Lp + T
            plen = lens.to(device=dev, dtype=torch.int32).clone()
            hist = torch.zeros(B, W, Lh, dtype=torch.int32, device=dev)  # a beam's prompt and output so far
            hist[:, :, :Lp] = input_ids.unsqueeze(1)
            start = None if penalize_prompt else plen.view(B, 1).expand(B, W).reshape(-1)
            penalize_logits_(logits, hist[:, 0], plen, start=None if penalize_prompt else plen, **penalties)
        logits = logits.unsqueeze(1).expand(B, W, logits.shape[-1])    # beam stride 0
        glen = lens.to(device=dev, dtype=torch.int32).clone()          # the group's common length
        scores = torch.full((B, W), ninf, dtype=torch.float32, device=dev)
        scores[:, 0] = 0.0
        finished = torch.zeros(B, W, dtype=torch.bool, device=dev)
        total = torch.zeros(B, W, dtype=torch.float64, device=dev)  # the hypotheses' summed log-probabilities
        new_lens = torch.zeros(B, W, dtype=torch.long, device=dev)
        tok_hist = torch.full((T, B, W), fill, dtype=torch.long, device=dev)
        par_hist = torch.arange(W, device=dev).expand(T, B, W).contiguous()
        tables = [torch.zeros(B, W, Lmax, dtype=torch.uint8, device=dev) for _ in range(2)]
        cur = 0
        cache.table = tables[cur]  # the table of the last decode step (zeros before the first)
        exists = scores > ninf
        active = exists
        for t in range(T):
            scores, parent, token, nfin, logp = beam_step(logits, scores, finished, eos_id=eos, fill=fill,
                                                          return_logp=True)
            par = parent.long()
            total = total.gather(1, par) + logp.double()  # logp is 0 behind a finished beam
            tok_hist[t], par_hist[t] = token, par
            exists = scores > ninf
            new_lens = torch.where(exists, new_lens.gather(1, par) + (~finished.gather(1, par)).long(), 0)
            finished = nfin | (exists & (glen >= Lmax).view(B, 1))  # no room to run this token
            active = exists & ~finished
            if t + 1 == T:
                break
            if check_every and (t + 1) % check_every == 0 and not bool(active.any()):
                break
            # src'[b, j, :n] = src[b, parent[j], :n]; src'[b, j, n] = parent[j], n = the last appended position
            nxt = tables[cur ^ 1]
            torch.gather(tables[cur], 1, par.view(B, W, 1).expand(B, W, Lmax), out=nxt)
            if t > 0:
                at = (glen.long() - 1).clamp(0, Lmax - 1).view(B, 1, 1).expand(B, W, 1)
                nxt.scatter_(2, at, parent.to(torch.uint8).view(B, W, 1))
            cur ^= 1
            cache.table = nxt
            cache.lens.copy_(torch.where(active, glen.view(B, 1), -1).view(-1))
            logits = self.decode_step(token.view(-1), cache, table=(nxt.view(B * W, Lmax), W)).view(B, W, -1)
            glen = glen + (glen < Lmax).to(glen.dtype)
            if t + 1 < min_new:
                logits[:, :, fill] = ninf  # every live beam has produced t + 1 tokens
            if penalties is not None:
                # the parents' histories, then this step's tokens at the group's common position
                hist = hist.gather(1, par.view(B, W, 1).expand(B, W, Lh))
                hist.scatter_(2, (plen.long() + t).view(B, 1, 1).expand(B, W, 1), token.to(torch.int32).view(B, W, 1))
                n = torch.where(active, (plen + (t + 1)).view(B, 1), -1).to(torch.int32).view(-1)
                penalize_logits_(logits.view(B * W, -1), hist.view(B * W, Lh), n, start=start, **penalties)
        cache.lens.copy_(torch.where(active, glen.view(B, 1), -1).view(-1))

        # the token rows: walk the recorded parents backwards
        out = torch.full((B, W, T), fill, dtype=torch.long, device=dev)
        idx = torch.arange(W, device=dev).expand(B, W)
        for t in range(T - 1, -1, -1):
            out[:, :, t] = tok_hist[t].gather(1, idx)
            idx = par_hist[t].gather(1, idx)
        out = torch.where(exists.unsqueeze(-1), out, fill)
        scores = torch.where(exists, total.to(torch.float32), ninf)
        key = scores / new_lens.clamp(min=1).to(torch.float32) ** float(length_penalty) if length_penalty else scores
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        out = out.gather(1, order.unsqueeze(-1).expand(B, W, T))
        return out, new_lens.gather(1, order), scores.gather(1, order)


class KVCache:
    """Per-layer K / V of shape [B, H, max_len, D] - views into one buffer - and ``lens`` int32
    [B], the tokens cached per row (outside 0 .. max_len - 1: a parked row).  ``table``: after a
    beam search, the uint8 [B / W, W, max_len] indirection table of its last decode step.

    ``kv_dtype="fp8"`` (``fp8`` is then True): ``buf`` holds uint8 e4m3fn codes [layers, 2, B, H,
    max_len, D] and ``ebuf`` int8 exponents [layers, 2, B, H, max_len], one per cached row
    (``ops.decode`` has the format); ``k`` / ``v`` are the code views and ``ke`` / ``ve`` the exponent
    views.  Half the bytes per cached token, plus one per row."""

    def __init__(self, layers, batch, heads, max_len, head_dim, device, dtype, kv_dtype="bf16"):
        self.batch, self.heads, self.max_len, self.head_dim = batch, heads, max_len, head_dim
        self.fp8 = kv_dtype == "fp8"
        if self.fp8:
            self.buf = torch.zeros(layers, 2, batch, heads, max_len, head_dim, device=device, dtype=torch.uint8)
            self.ebuf = torch.zeros(layers, 2, batch, heads, max_len, device=device, dtype=torch.int8)
            self.ke = [self.ebuf[i, 0] for i in range(layers)]
            self.ve = [self.ebuf[i, 1] for i in range(layers)]
        else:
            self.buf = torch.zeros(layers, 2, batch, heads, max_len, head_dim, device=device, dtype=dtype)
        self.k = [self.buf[i, 0] for i in range(layers)]
        self.v = [self.buf[i, 1] for i in range(layers)]
        self.lens = torch.zeros(batch, dtype=torch.int32, device=device)
        self.table = None

    def slot_view(self, beams, slot):
        """The rows ``slot, slot + beams, ...`` as a cache of ``batch / beams`` rows over the same
        storage (strided views; ``lens`` is the view's own): where ``prefill`` writes the prompts
        of a beam search."""
        if self.batch % beams:
            raise ValueError(f"{self.batch} cache rows are not whole groups of {beams}")
        view = KVCache.__new__(KVCache)
        view.batch, view.heads, view.max_len, view.head_dim = self.batch // beams, self.heads, self.max_len, self.head_dim
        view.fp8 = self.fp8
        view.buf = self.buf[:, :, slot::beams]
        view.k = [k[slot::beams] for k in self.k]
        view.v = [v[slot::beams] for v in self.v]
        if self.fp8:
            view.ebuf = self.ebuf[:, :, slot::beams]
            view.ke = [e[slot::beams] for e in self.ke]
            view.ve = [e[slot::beams] for e in self.ve]
        view.lens = self.lens[slot::beams]
        view.table = None
        return view


def _gpt2_train_flops_per_sample(self, seq_len):
    """6*P_lin + causal attention (~6*L*H per layer, half of the full 12*L*H) per
    token, plus the tied LM head (6*H*V), times seq_len."""
    cfg = self.cfg
    H, V, n = cfg["hidden_size"], cfg["vocab_size"], cfg["num_layers"]
    F_ = cfg.get("intermediate_size") or 4 * H
    per_tok = 6 * n * (4 * H * H + 2 * H * F_) + 6 * seq_len * H * n + 6 * H * V
    return per_tok * seq_len


GPT2LMModel.train_flops_per_sample = _gpt2_train_flops_per_sample

