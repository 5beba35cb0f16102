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

    def _rows(self, decode_linears, n_rows, ref):
        """How a call of ``n_rows`` rows on ``ref``'s device runs its Linears: "rows" (through
        ``ops.decode.linear_rows``: asked for, at most 128 rows, bf16 compute on a HIP device), "rows_fused" (the
        same op with each block's LayerNorms and residual adds inside it, under the same conditions), "rows_fp8"
        (through ``ops.decode.linear_rows_fp8`` on the quantized snapshot: wherever it is asked for) or False
        (``ops.linear``)."""
        if decode_linears not in ("tile", "rows", "rows_fp8", "rows_fused"):
            raise ValueError(f"decode_linears must be 'tile', 'rows', 'rows_fp8' or 'rows_fused', got {decode_linears!r}")
        if decode_linears == "rows_fp8":
            return "rows_fp8"
        from ..ops.decode import ROWS_MAX_M
        return (decode_linears != "tile" and n_rows <= ROWS_MAX_M and ref.is_cuda
                and self.compute_dtype == torch.bfloat16) and decode_linears

    @torch.no_grad()
    def quantize_decode_weights(self):
        """Build (or rebuild) the one-byte snapshot that ``decode_linears="rows_fp8"`` computes with: for the
        weight of every block's qkv, attn_proj, mlp_fc and mlp_proj and for the tied ``wte``,
        ``ops.decode.kv_quantize_ref`` of the compute-dtype values - e4m3fn codes uint8 [N, K] and one int8
        power-of-two exponent per weight row.  A one-time PyTorch op.  The snapshot is kept on the module,
        is not part of ``state_dict`` and does NOT follow later weight updates (an optimizer step, a loaded
        checkpoint, a move to another device): call this again after one.  The ``rows_fp8`` paths build it on
        first use if it is absent.  Biases, LayerNorms and the embedding lookup are not quantized."""
        from ..ops.decode import kv_quantize_ref
        dt = self.compute_dtype
        weights = [self.wte.weight] + [lin.weight for blk in self.h
                                       for lin in (blk.attn.qkv, blk.attn_proj, blk.mlp_fc, blk.mlp_proj)]
        self._decode_w8 = {id(w): kv_quantize_ref(ops.shadow(w, dt)) for w in weights}
        return self

    def _w8(self, weight):
        """(codes, exponents) of ``weight`` from the snapshot, built on first use."""
        if getattr(self, "_decode_w8", None) is None:
            self.quantize_decode_weights()
        return self._decode_w8[id(weight)]

    def _lin_rows(self, lin, t, rows="rows", ln=None, residual=None):
        """``lin(t)`` for a ``layers.Linear`` through ``ops.decode.linear_rows`` on the bf16 shadows, or with
        ``rows="rows_fp8"`` through ``ops.decode.linear_rows_fp8`` on the snapshot (the bias stays as it is).
        ``ln``: a ``layers.LayerNorm`` applied to ``t`` inside the call; ``residual``: added to the result inside it
        (``linear_rows``'s keywords, "rows_fused")."""
        from ..ops.decode import linear_rows, linear_rows_fp8
        dt = self.compute_dtype
        t2 = t.reshape(-1, t.shape[-1])
        if rows == "rows_fp8":
            y = linear_rows_fp8(t2, *self._w8(lin.weight), ops.shadow(lin.bias, dt), act=lin.act)
        elif ln is None and residual is None:
            y = linear_rows(t2, ops.shadow(lin.weight, dt), ops.shadow(lin.bias, dt), act=lin.act)
        else:
            y = linear_rows(t2, ops.shadow(lin.weight, dt), ops.shadow(lin.bias, dt), act=lin.act,
                            ln=None if ln is None else (ops.shadow(ln.weight, dt), ops.shadow(ln.bias, dt), ln.eps),
                            residual=None if residual is None else residual.reshape(-1, residual.shape[-1]))
        return y.view(*t.shape[:-1], -1)

    def _head(self, a, rows):
        """The tied head on ``a`` [R, H] -> logits [R, V]."""
        if rows == "rows_fp8":
            from ..ops.decode import linear_rows_fp8
            return linear_rows_fp8(a, *self._w8(self.wte.weight))
        if rows:
            from ..ops.decode import linear_rows
            return linear_rows(a, ops.shadow(self.wte.weight, self.compute_dtype))
        return ops.linear(a, self.wte.weight)

    def _blocks(self, x, a, attend, rows=False):
        """The block stack of ``hidden_states`` in eval mode with ``attend(i, qkv)`` as layer i's
        attention over its packed projection -> ln_f of the last residual stream.  ``rows``: the four
        Linears of every block run through ``ops.decode.linear_rows`` or, for "rows_fp8",
        ``ops.decode.linear_rows_fp8`` (:meth:`_rows` says which).  "rows_fused": ``a`` is not used - ln_1 and ln_2
        run inside qkv and mlp_fc and the two residual adds inside attn_proj and mlp_proj (five launches per block
        instead of seven); ln_f is ``ops.layer_norm``, one launch per call."""
        if rows == "rows_fused":
            # five launches per block: only the residual stream x is carried, each LayerNorm runs in the prologue
            # of the Linear that reads it and each residual add in the epilogue of the Linear in front of it
            for i, blk in enumerate(self.h):
                qkv = self._lin_rows(blk.attn.qkv, x, rows, ln=blk.ln_1)
                x = self._lin_rows(blk.attn_proj, attend(i, qkv), rows, residual=x)
                x = self._lin_rows(blk.mlp_proj, self._lin_rows(blk.mlp_fc, x, rows, ln=blk.ln_2), rows, residual=x)
            return ops.layer_norm(x, self.ln_f.weight, self.ln_f.bias, self.ln_f.eps)
        lns = [blk.ln_1 for blk in self.h] + [self.ln_f]
        for i, blk in enumerate(self.h):
            if rows:
                h = self._lin_rows(blk.attn_proj, attend(i, self._lin_rows(blk.attn.qkv, a, rows)), rows)
            else:
                h = blk.attn_proj(attend(i, blk.attn.qkv(a)))
            x, a = ops.residual_layernorm(h, x, blk.ln_2.weight, blk.ln_2.bias, 0.0, blk.ln_2.eps, False)
            if rows:
                h = self._lin_rows(blk.mlp_proj, self._lin_rows(blk.mlp_fc, a, rows), rows)
            else:
                h = ops.mlp(a, blk.mlp_fc, blk.mlp_proj)
            x, a = ops.residual_layernorm(h, x, lns[i + 1].weight, lns[i + 1].bias, 0.0, lns[i + 1].eps, False)
        return a

    @torch.no_grad()
    def prefill(self, input_ids, lens, cache, decode_linears="tile", chunk=0):
        """Right-padded prompts ``input_ids`` [B, Lp] of ``1 <= lens[b] <= Lp`` tokens: one causal
        forward (what stands behind a row's prompt never reaches it), each layer's K and V of the
        prompt positions copied into ``cache`` (quantized into an fp8 cache; the prompt's own forward
        attends over the unquantized values), ``cache.lens = lens`` -> the logits [B, V] at each row's
        last prompt position.  ``decode_linears="rows"``: the head on those B rows runs through
        ``ops.decode.linear_rows`` (see :meth:`decode_step`), with "rows_fp8" through
        ``ops.decode.linear_rows_fp8``; the prompt's forward is unchanged and keeps its unquantized weights.

        ``chunk = C >= 1``: the prompt goes through :meth:`extend` in pieces of C columns instead,
        starting from an empty cache - piece ``p0`` with ``counts = clamp(lens - p0, 0, C)``, so nothing is
        padded to the longest prompt's next multiple of 64 and K and V reach the cache inside the
        attention kernel.  Each row's hidden state at position ``lens - 1`` is taken from the piece that
        holds it and the head runs once on those B rows.  Not over an fp8 cache.  0: the single forward."""
        dt = self.compute_dtype
        B, Lp = input_ids.shape
        head_rows = self._rows(decode_linears, B, input_ids)
        if Lp > cache.max_len or B != cache.batch:
            raise ValueError(f"prompts [{B}, {Lp}] do not fit a cache of {cache.batch} rows x {cache.max_len}")
        lens = lens.to(device=input_ids.device, dtype=torch.int32)
        C = int(chunk)
        if C < 0:
            raise ValueError(f"chunk must be >= 0, got {chunk}")
        if C:
            if cache.fp8:
                raise ValueError("a chunked prefill has no fp8 variant: it needs kv_dtype='bf16'")
            cache.lens = torch.zeros_like(lens)
            rows = torch.arange(B, device=input_ids.device)
            last = None
            for p0 in range(0, Lp, C):
                ids = input_ids[:, p0:p0 + C]
                hid = self.extend(ids, cache, (lens - p0).clamp(0, ids.shape[1]), decode_linears)
                at = lens.long() - 1 - p0  # where the row's last prompt token stands in this piece
                mine = hid[rows, at.clamp(0, ids.shape[1] - 1)]
                last = mine if last is None else torch.where((at >= 0).view(B, 1), mine, last)
            return self._head(last, head_rows)
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
        return self._head(last, head_rows)

    @torch.no_grad()
    def extend(self, tokens, cache, counts=None, decode_linears="tile"):
        """Append T tokens per row to a cache that may already hold something, token j of row b at
        position ``cache.lens[b] + j`` -> the hidden states [B, T, H] after ``ln_f``; the head is the
        caller's (a chunked prefill needs one row of them).  ``counts`` (int [B], default T): how many
        of a row's tokens are real - ``c_b`` of ``ops.decode.attention_extend``; the hidden states of
        the others mean nothing and their keys are not stored.  ``cache.lens`` advances by ``c_b`` on
        the device; a parked row does no cache work and keeps its ``lens``.  Runs longer than the
        kernel's 128 tokens go through the stack in pieces of 128.  ``decode_linears``: as in
        :meth:`decode_step`, for the rows of a piece.  Not over an fp8 cache."""
        from ..ops.decode import EXTEND_MAX, attention_extend
        if cache.fp8:
            raise ValueError("extend has no fp8 variant: it needs kv_dtype='bf16'")
        dt = self.compute_dtype
        B, T = tokens.shape
        if T < 1 or B != cache.batch:
            raise ValueError(f"tokens [{B}, {T}] do not fit a cache of {cache.batch} rows")
        heads = cache.heads
        lens = cache.lens
        counts = torch.full_like(lens, T) if counts is None else counts.to(device=lens.device, dtype=torch.int32)
        ln0 = self.h[0].ln_1
        outs = []
        for t0 in range(0, T, EXTEND_MAX):
            Tc = min(EXTEND_MAX, T - t0)
            rows = self._rows(decode_linears, B * Tc, tokens)
            cnt = (counts - t0).clamp(0, Tc)
            pos = lens.long().view(B, 1) + torch.arange(Tc, device=tokens.device).view(1, Tc)
            pos = pos.clamp(0, self.cfg["max_position_embeddings"] - 1).view(-1)
            # the B Tc tokens stand where decode_step has its B rows: the same kernels around the attention
            x, a = ops.residual_layernorm(self.wte(tokens[:, t0:t0 + Tc].reshape(1, B * Tc), dt), None, ln0.weight,
                                          ln0.bias, 0.0, ln0.eps, False, pos=self.wpe(pos, dt))

            def attend(i, qkv):
                return attention_extend(qkv.view(B, Tc, -1), cache.k[i], cache.v[i], lens, heads,
                                        counts=cnt).view(1, B * Tc, -1)

            outs.append(self._blocks(x, a, attend, rows).view(B, Tc, -1))
            active = (lens >= 0) & (lens < cache.max_len)
            lens += torch.where(active, torch.minimum(cnt, cache.max_len - lens), 0).to(lens.dtype)
        return outs[0] if len(outs) == 1 else torch.cat(outs, 1)

    @torch.no_grad()
    def decode_step(self, tokens, cache, table=None, decode_linears="tile"):
        """One token per row at position ``cache.lens[b]`` -> the next-token logits [B, V];
        ``cache.lens`` advances on the device.  A parked row (``lens`` outside 0 .. max_len - 1)
        does no cache work, keeps its ``lens``, and its logits mean nothing.  ``table``: a pair
        ``(src uint8 [B, max_len], beams)`` handed to ``attention_decode`` - the rows are groups
        of ``beams`` slots that read their cached keys through ``src`` (beam search; not over an
        fp8 cache).  Over an fp8 cache the step is ``ops.decode.attention_decode_fp8``.  Over a
        :class:`GroupKVCache` (several continuations per prompt) it is :meth:`_decode_step_grouped`.

        ``decode_linears``: "tile" (the default) runs the Linears through ``ops.linear``, the B rows
        padded into the training GEMM's tiles.  "rows" runs qkv, attn_proj, mlp_fc with its GELU,
        mlp_proj and the tied head through ``ops.decode.linear_rows`` on the bf16 shadows - one launch
        each, an output row a function of its input row alone - where the call has at most 128 rows and
        computes in bf16 on a HIP device; anywhere else it is "tile".  "rows_fp8" runs the same five through
        ``ops.decode.linear_rows_fp8`` on the one-byte snapshot of :meth:`quantize_decode_weights` (built on
        first use; it does not follow later weight updates) - on any device and at any row count, the op's
        PyTorch definition serving what its kernel does not, so the mode means the same numbers everywhere.
        The embedding lookup reads ``wte`` unquantized and the biases stay as they are.  The residual adds,
        the LayerNorms and the attention are the same in all three.  "rows_fused" is "rows" (same conditions, "tile"
        anywhere else) with each block's two LayerNorms and two residual adds inside ``linear_rows`` (its ``ln`` and
        ``residual`` keywords): LN1 + qkv, attention, attn_proj + residual, LN2 + mlp_fc + GELU, mlp_proj + residual -
        five launches per block instead of seven; ln_f is one ``ops.layer_norm`` launch and the head is
        ``linear_rows``.  There the residual stream is rounded to bf16 once per sublayer (the sum, not the branch and
        then the sum).  The modes round differently."""
        from ..ops.decode import attention_decode, attention_decode_fp8
        if isinstance(cache, GroupKVCache):
            if table is not None:
                raise ValueError("a GroupKVCache has no indirection-table variant")
            return self._decode_step_grouped(tokens, cache, decode_linears)
        if cache.fp8 and table is not None:
            raise ValueError("an fp8 cache has no indirection-table variant: beam search needs kv_dtype='bf16'")
        dt = self.compute_dtype
        B = tokens.shape[0]
        rows = self._rows(decode_linears, B, tokens)
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

        a = self._blocks(x, a, attend, rows)
        cache.lens += ((cache.lens >= 0) & (cache.lens < cache.max_len)).to(cache.lens.dtype)
        return self._head(a.view(B, -1), rows)

    @torch.no_grad()
    def generate(self, input_ids, lens, max_new_tokens, *, temperature=1.0, top_k=0, top_p=0.0, eos_id=None,
                 generator=None, cache=None, check_every=16, noise_seed=None, row_base=0, repetition_penalty=1.0,
                 presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0, min_new_tokens=0,
                 penalize_prompt=True, return_logprobs=False, kv_dtype=None, decode_linears="tile",
                 prefill_chunk=0):
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
        error.  ``decode_linears``: "tile", "rows", "rows_fp8" or "rows_fused", handed to :meth:`prefill` and every
        :meth:`decode_step`.  ``prefill_chunk``: :meth:`prefill`'s ``chunk`` (0: the single forward).
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
        self._rows(decode_linears, B, input_ids)  # an unknown value raises here
        dl = {} if decode_linears == "tile" else {"decode_linears": decode_linears}
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
        logits = self.prefill(input_ids, lens, cache, **dl, **({"chunk": prefill_chunk} if prefill_chunk else {}))
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
            logits = self.decode_step(tok, cache, **dl)
        cache.lens.masked_fill_(done, -1)
        return (out, new_lens, logprobs) if return_logprobs else (out, new_lens)

    # ---- several samples per prompt over a shared prompt cache (inference only) ---------------

    def init_group_cache(self, batch, group, prompt_len, max_new, device=None, dtype=None, kv_dtype="bf16"):
        """An empty :class:`GroupKVCache` for ``batch`` prompts of up to ``prompt_len`` tokens with ``group``
        continuations each of up to ``max_new`` tokens: a ``prefix`` cache of ``batch`` rows, which
        :meth:`prefill` fills once per prompt, and a ``suffix`` cache of ``batch * group`` rows (row
        ``b * group + g``), which :meth:`decode_step` appends to.  Values in ``dtype`` (the compute dtype);
        there is no fp8 variant."""
        if kv_dtype != "bf16":
            raise ValueError(f"a group cache has no fp8 variant: it needs kv_dtype='bf16', got {kv_dtype!r}")
        if group < 1 or max_new < 1:
            raise ValueError(f"group and max_new must be >= 1, got {group}, {max_new}")
        room = self.cfg["max_position_embeddings"] - prompt_len  # a continuation ends with the model's positions
        return GroupKVCache(self.init_cache(batch, prompt_len, device, dtype),
                            self.init_cache(batch * group, max(1, min(max_new, room)), device, dtype), group)

    def _decode_step_grouped(self, tokens, cache, decode_linears):
        """:meth:`decode_step` over a :class:`GroupKVCache`: row ``r = b G + g`` stands at position
        ``prefix.lens[b] + suffix.lens[r]``, every layer's attention is
        ``ops.decode.attention_decode_grouped`` and ``suffix.lens`` advances on the device.  A parked row
        (``suffix.lens`` outside 0 .. its max_len - 1) does no cache work and keeps its ``lens``."""
        from ..ops.decode import attention_decode_grouped
        dt = self.compute_dtype
        pre, suf, G = cache.prefix, cache.suffix, cache.group
        R = tokens.shape[0]
        if R != suf.batch:
            raise ValueError(f"{R} tokens do not fit a group cache of {pre.batch} x {G} rows")
        rows = self._rows(decode_linears, R, tokens)
        heads = suf.heads
        plens = pre.lens.view(-1, 1)  # against [B, G] views of the rows: no repeated copy
        pos = (plens + suf.lens.view(-1, G)).view(R).long().clamp(0, self.cfg["max_position_embeddings"] - 1)
        ln0 = self.h[0].ln_1
        x, a = ops.residual_layernorm(self.wte(tokens.view(1, R), dt), None, ln0.weight, ln0.bias, 0.0, ln0.eps,
                                      False, pos=self.wpe(pos, dt))

        def attend(i, qkv):
            return attention_decode_grouped(qkv.view(R, -1), pre.k[i], pre.v[i], pre.lens, suf.k[i], suf.v[i],
                                            suf.lens, heads, group=G).view(1, R, -1)

        a = self._blocks(x, a, attend, rows)
        slens = suf.lens.view(-1, G)
        slens += ((slens >= 0) & (slens < suf.max_len) & ((plens >= 0) & (plens <= pre.max_len))).to(slens.dtype)
        return self._head(a.view(R, -1), rows)

    @torch.no_grad()
    def generate_samples(self, input_ids, lens, max_new_tokens, *, num_samples, temperature=1.0, top_k=0, top_p=0.0,
                         eos_id=None, generator=None, noise_seed=None, row_base=0, decode_linears="tile",
                         cache=None, check_every=16):
        """``num_samples = G`` continuations of every right-padded prompt -> (tokens [B, G, max_new_tokens],
        new_lens [B, G]), with :meth:`generate`'s loop and meanings over a :class:`GroupKVCache`: the prompt's
        forward runs once per prompt, its keys are cached once, and every decode step reads them once per
        group (``ops.decode.attention_decode_grouped``).

        The first token of all G samples is drawn from the one prefill logits row of the prompt.  With an
        integer ``noise_seed`` sample (b, g) draws with the global row ``row_base + b G + g`` - the row it
        would have in :meth:`generate` on the prompts repeated G times each, so the noise is the same.  A row
        stops when it has emitted ``eos_id``, its suffix cache is full or the model's positions end: it is
        parked (``cache.suffix.lens[r] = -1``) and the rest of its output is ``eos_id`` (0 without one).
        ``cache``: one from :meth:`init_group_cache` to use.  Penalties, log-probabilities, beams and
        lookahead are :meth:`generate`'s, :meth:`beam_search`'s and :meth:`generate_lookahead`'s alone."""
        from utils.lm_sampling import sample_next
        from ..ops.decode import sample_tokens
        G = int(num_samples)
        if G < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        philox = noise_seed is not None and temperature > 0
        B, Lp = input_ids.shape
        R = B * G
        dev = input_ids.device
        self._rows(decode_linears, R, input_ids)  # an unknown value raises here
        dl = {} if decode_linears == "tile" else {"decode_linears": decode_linears}
        if cache is None:
            cache = self.init_group_cache(B, G, Lp, max_new_tokens, dev)
        elif cache.group != G or cache.prefix.batch != B:
            raise ValueError(f"the given cache holds {cache.prefix.batch} groups of {cache.group}, not {B} of {G}")
        pre, suf = cache.prefix, cache.suffix
        fill = 0 if eos_id is None else int(eos_id)
        out = torch.full((R, max_new_tokens), fill, dtype=torch.long, device=dev)
        new_lens = torch.zeros(R, dtype=torch.long, device=dev)
        done = torch.zeros(R, dtype=torch.bool, device=dev)
        suf.lens.zero_()
        logits = self.prefill(input_ids, lens, pre, **dl).repeat_interleave(G, 0)
        last_pos = self.cfg["max_position_embeddings"] - pre.lens.repeat_interleave(G)  # suffix keys the positions allow
        for t in range(max_new_tokens):
            if philox:
                tok = sample_tokens(logits, temperature=temperature, top_k=top_k, top_p=top_p, seed=int(noise_seed),
                                    step=t, row_base=row_base)
            else:
                tok = sample_next(logits, temperature, top_k, top_p, generator)
            tok = torch.where(done, fill, tok)
            out[:, t] = tok
            new_lens += (~done).to(new_lens.dtype)
            if eos_id is not None:
                done = done | (tok == fill)
            done = done | (suf.lens >= suf.max_len) | (suf.lens >= last_pos)  # no room to run this token
            if t + 1 == max_new_tokens:
                break
            suf.lens.masked_fill_(done, -1)
            if check_every and (t + 1) % check_every == 0 and bool(done.all()):
                break
            logits = self.decode_step(tok, cache, **dl)
        suf.lens.masked_fill_(done, -1)
        return out.view(B, G, max_new_tokens), new_lens.view(B, G)

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
    def decode_block(self, tokens, cache, counts=None, decode_linears="tile"):
        """T tokens per row, token j of row b at position ``cache.lens[b] + j`` -> logits [B, T, V],
        the logits at j saying what follows token j.  ``counts`` (int [B], default T): how many of a
        row's tokens are real - ``ops.decode.attention_decode_block`` has the exact rule; the logits of
        the others mean nothing and their keys are not stored.  ``cache.lens`` is NOT advanced: the
        caller commits as many positions as it accepted, and what was stored beyond them is
        overwritten or never read.  ``decode_linears``: as in :meth:`decode_step`, for the B T rows."""
        from ..ops.decode import attention_decode_block
        if cache.fp8:
            raise ValueError("decode_block has no fp8 variant: lookahead decoding needs kv_dtype='bf16'")
        dt = self.compute_dtype
        B, T = tokens.shape
        rows = self._rows(decode_linears, B * T, tokens)
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

        a = self._blocks(x, a, attend, rows)
        return self._head(a.view(B * T, -1), rows).view(B, T, -1)

    @torch.no_grad()
    def generate_lookahead(self, input_ids, lens, max_new_tokens, *, lookahead, ngram=2, eos_id=None, cache=None,
                           check_every=4, draft=None, return_stats=False, repetition_penalty=1.0,
                           presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0, min_new_tokens=0,
                           penalize_prompt=True, decode_linears="tile"):
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
        ``decode_linears``: "tile", "rows", "rows_fp8" or "rows_fused", handed to :meth:`prefill` and every :meth:`decode_block`.

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
        self._rows(decode_linears, B, input_ids)  # an unknown value raises here
        dl = {} if decode_linears == "tile" else {"decode_linears": decode_linears}
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
        logits = self.prefill(input_ids, lens, cache, **dl)
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
            logits = self.decode_block(block, cache, counts, **dl)
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
                    no_repeat_ngram=0, min_new_tokens=0, penalize_prompt=True, decode_linears="tile"):
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
        they are expanded.  The scores are sums of the log-softmax of the processed logits.

        ``decode_linears``: "tile", "rows", "rows_fp8" or "rows_fused", handed to :meth:`prefill` and every :meth:`decode_step`
        (``B W`` rows)."""
        from ..ops.decode import beam_step, penalize_logits_
        penalties, min_new = _logit_processors(repetition_penalty, presence_penalty, frequency_penalty,
                                               no_repeat_ngram, min_new_tokens, eos_id)
        W = int(num_beams)
        if not 1 <= W <= 255:
            raise ValueError(f"num_beams must be in 1 .. 255, got {num_beams}")
        B, Lp = input_ids.shape
        dev = input_ids.device
        T = int(max_new_tokens)
        self._rows(decode_linears, B * W, input_ids)  # an unknown value raises here
        dl = {} if decode_linears == "tile" else {"decode_linears": decode_linears}
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

        logits = self.prefill(input_ids, lens, cache.slot_view(W, 0), **dl)  # the prompts, once, into slot 0
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
            logits = self.decode_step(token.view(-1), cache, table=(nxt.view(B * W, Lmax), W), **dl).view(B, W, -1)
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


class GroupKVCache:
    """The cache of ``GPT2LMModel.generate_samples``: ``prefix``, a :class:`KVCache` of B rows that holds each
    prompt's keys and values once, and ``suffix``, one of ``B * group`` rows (row ``b * group + g``) for what
    each of the prompt's ``group`` continuations has produced since.  Row r's tokens are
    ``prefix.lens[r // group] + suffix.lens[r]``; ``suffix.lens[r]`` outside 0 .. ``suffix.max_len - 1`` parks
    the row."""

    def __init__(self, prefix, suffix, group):
        if prefix.fp8 or suffix.fp8:
            raise ValueError("a group cache has no fp8 variant")
        if suffix.batch != prefix.batch * group:
            raise ValueError(f"{suffix.batch} suffix rows are not {prefix.batch} groups of {group}")
        self.prefix, self.suffix, self.group = prefix, suffix, int(group)


def _gpt2_train_flops_per_sample(self, seq_len):
    """6*P_lin + causal attention (~6*L*H per layer, half of the full 12*L*H) per
    token, plus the tied LM head (6*H*V), times seq_len."""
    cfg = self.cfg
    H, V, n = cfg["hidden_size"], cfg["vocab_size"], cfg["num_layers"]
    F_ = cfg.get("intermediate_size") or 4 * H
    per_tok = 6 * n * (4 * H * H + 2 * H * F_) + 6 * seq_len * H * n + 6 * H * V
    return per_tok * seq_len


GPT2LMModel.train_flops_per_sample = _gpt2_train_flops_per_sample

