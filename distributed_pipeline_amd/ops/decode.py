"""
The per-token ops of GPT-2 generation: single-query attention over a K/V cache (directly, or through
the indirection table of a beam search), the same for a block of new tokens with the guesses that
fill it (lookahead decoding), one beam-search step, the choice of the next token, the logit
processors in front of it (repetition, presence and frequency penalty, no-repeat-n-gram ban), and
the statistics of a logits row against a given token (teacher-forced scoring).

Attention of one decode step
----------------------------
``attention_decode(qkv_new, k_cache, v_cache, lens, n_heads)`` appends the new token's key and
value to the caches (in place) and attends its query over everything cached so far:

* ``qkv_new`` [B, 3*H*D]: the token's packed projection, order [3][H][D] (the order of
  ``ops.nn.attention``'s ``qkv.view(B, L, 3, H, D)``);
* ``k_cache`` / ``v_cache`` [B, H, Lmax, D], possibly views into a larger buffer;
* ``lens`` int32 [B]: keys already cached per row.  It is NOT modified - the caller advances it
  with a device op, so a generation loop never synchronises with the host.

A row with ``0 <= lens[b] < Lmax`` stores the new k and v (bit for bit) at ``cache[b, :, lens[b]]``
and returns ``softmax(q K^T / sqrt(D)) V`` over the keys ``0 .. lens[b]``.  Any other ``lens[b]``
marks the row inactive (a finished, parked row): nothing is stored and its output is zeros.  Cache
rows beyond ``lens[b]`` never contribute, whatever they hold.

bf16 on a HIP device with D in {64, 128}: one kernel (csrc/attn_decode.hip).  Anything else (CPU,
fp32, other D, a cache whose rows are not packed): the same definition in fp32 PyTorch,
:func:`attention_decode_ref`.  Inference only: no autograd.

The cache indirection table (beam search).  With ``src`` (uint8 [R, Lmax]) and ``beams = W``
(``R % W == 0``) the R rows are groups of W slots: row ``r = b W + w`` is slot w of prompt b.  An
active row r reads its cached key and value ``t < lens[r]`` from cache row
``(r // W) W + min(src[r, t], W - 1)`` - the clamp keeps any table content inside the row's own
group, so a bad table gives wrong numbers and never an out-of-range read - while the new k and v are
stored at ``(r, lens[r])``, the row's own slot.  ``src`` is not modified and ``src[r, t]`` for
``t >= lens[r]`` is never read.  Inactive rows behave as without a table.  The fold order is the
plain kernel's: with ``src[r, t] == r % W`` everywhere the output and the caches are the plain
call's bit for bit.  Caller's contract: no active row may read a (slot, position) that another active
row of the same call appends to; this holds whenever the active rows of a group have equal ``lens``,
which is what beam search guarantees.  Re-parenting W hypotheses then rewrites ``W Lmax`` bytes per
prompt instead of gathering ``[layers, 2, B W, H, Lmax, D]`` into a second buffer.

The one-byte cache: ``kv_quantize``, ``kv_store``, ``attention_decode_fp8``
---------------------------------------------------------------------------
A cached row - the D values of one (K or V, batch row, head, position) - is stored as D OCP
``e4m3fn`` codes (uint8) and one int8 exponent ``e``.  For a row ``x`` of finite values and
``a = max|x_i|``: ``e = 0`` if ``a == 0``; otherwise ``(m, p) = frexp(a)``, m in [0.5, 1), and
``e = max(p - 9 + (1 if m > 0.875 else 0), -127)``.  Then ``a * 2^-e`` lies in (224, 448] - 448 =
0.875 * 2^9 is e4m3fn's largest finite value - so no element saturates.  ``code_i = e4m3fn(x_i * 2^-e)``,
round to nearest even, subnormals kept; ``x^_i = float(code_i) * 2^e``.  The scaling is by a power of
two, so codes and exponent are a function of the input bits alone: the kernels and PyTorch
(``torch.ldexp(x.float(), -e).to(torch.float8_e4m3fn)``) agree bit for bit.  Non-finite values: memory
safe, the stored bytes are unspecified.  One finite edge: a row maximum above 240 * 2^120 (the top
eight bf16 magnitudes) rounds up to the code 256 at e = 120, and 2^128 dequantizes to inf in fp32.

* ``kv_quantize(x [..., D]) -> (codes uint8 [..., D], exp int8 [...])``; ``kv_dequantize(codes, exp) ->
  fp32 [..., D]``, exact.
* ``kv_store(qkv [B, L, 3*H*D], lens int32 [B], k8, ke, v8, ve)``: the prefill's store.  K and V of the
  positions ``l < lens[b]`` are quantized into cache row l of ``k8`` / ``v8`` uint8 [B, H, Lmax, D] and
  ``ke`` / ``ve`` int8 [B, H, Lmax]; every other byte is left as it is.
* ``attention_decode_fp8(qkv_new, k8, ke, v8, ve, lens, n_heads)`` is ``attention_decode`` with the
  dequantized caches in place of K and V: an active row quantizes its new k and v, stores codes and
  exponents at row ``lens[b]`` and attends over the cached keys and its own **dequantized** new key and
  value - "append, then attend over the cache" is one definition whatever the step.  An inactive row
  stores nothing, codes and exponents included, and returns zeros; rows at or beyond ``lens[b]`` are
  never read, whatever they hold.

bf16 on a HIP device with D in {64, 128} and packed 16-byte code rows: csrc/attn_decode_fp8.hip (the
conversions are gfx950's ``v_cvt_pk_fp8_f32`` / ``v_cvt_pk_f32_fp8``; the exponents are applied once per
key, as exact ``ldexp``).  Anything else: the ``_ref`` twins in PyTorch.  There is no table (beam) and no
block (lookahead) variant.

Attention of a block of new tokens: ``attention_decode_block``
--------------------------------------------------------------
``attention_decode_block(qkv_new [B, T, 3*H*D], k_cache, v_cache, lens int32 [B], n_heads, *,
counts=None) -> out [B, T, H*D]`` with ``1 <= T <= 8``: T new tokens per row against the cache in one
pass over K and V (lookahead decoding: a committed token and T - 1 guessed ones).

* Let ``c_b = 0`` for an inactive row (``lens[b]`` outside ``[0, Lmax)``), and otherwise
  ``c_b = clamp(counts[b], 0, min(T, Lmax - lens[b]))``; ``counts=None`` means T.
* The call equals T successive ``attention_decode`` calls: call j runs on ``qkv_new[:, j]`` with
  ``lens_j[b] = lens[b] + j`` if ``j < c_b``, else -1.
* So query ``j < c_b`` stores its k and v at cache row ``lens[b] + j``, the bits of ``qkv_new``, and
  attends over the keys ``0 .. lens[b] + j``, rounded once to bf16.
* Query ``j >= c_b`` stores nothing and returns zeros.
* ``lens`` and ``counts`` are not modified; the caller commits as many positions as it accepts.
* Cache rows at or beyond ``lens[b] + c_b`` are neither read nor written, whatever they hold.

bf16 on a HIP device with D in {64, 128}: one kernel (csrc/attn_decode_block.hip) that keeps the
plain kernel's fold order per query - a key goes to the (wave, lane group, iteration) its position
gives it there, the query's own key is folded last, the keys of the block in front of a query are
taken from ``qkv_new`` - so output and caches are meant to equal those of the T sequential calls bit
for bit; ``T = 1`` without ``counts`` is the plain kernel itself.  Anything else:
:func:`attention_decode_block_ref`, the T masked ``attention_decode_ref`` calls as written.  There is
no table (beam) variant.

The guesses: ``lookup_draft``
-----------------------------
``lookup_draft(history int64 [B, Lh], n [B], *, ngram, max_draft) -> (draft int64 [B, max_draft],
k int64 [B])`` copies a row's guesses from its own history ("prompt lookup").  For row b let s be the
first ``n_b`` tokens (``n_b`` clamped to ``[0, Lh]``) and ``g = ngram``.  If there is an
``i <= n_b - g - 1`` with ``s[i : i+g] == s[n_b-g : n_b]``, take the largest such i; with
``p = n_b - g - i >= 1`` the row gets ``k = max_draft`` and ``draft[m] = s[i + g + (m mod p)]`` - a copy
that may run into its own output, as an LZ77 match does, so a row that repeats with period p is
continued with that period.  Otherwise ``k = 0`` and the draft row is zeros.  Tensor ops only, on either
device (an ``unfold`` compare, a masked maximum over the start index, a gather): no kernel, no host
synchronisation, integers only.

One beam-search step: ``beam_step``
-----------------------------------
``beam_step(logits [B, W, V], scores fp32 [B, W], finished bool [B, W], *, eos_id=-1, fill=0)
-> (new_scores fp32 [B, W], parent int32 [B, W], token int64 [B, W], new_finished bool [B, W])``.
``logits`` is fp32 or bf16 with last stride 1 and any batch or beam stride; beam stride 0 is how the
first step runs (the prefill logits ``[B, 1, V]`` expanded, ``scores = [0, -inf, ...]``).

1. ``s_v = fp32(logit_v)``.  A NaN becomes -inf.
2. A beam with ``scores[b, w] == -inf`` (or NaN) does not exist and has no candidate.
3. A finished beam has exactly one candidate ``(w, fill)``, whose value is ``scores[b, w]`` with its
   bits unchanged.
4. A live beam has the candidates ``c(w, v) = scores[b, w] + ((s_v - m) - log Z)`` in fp32, in that
   operation order, with ``m = max_v s_v`` and ``Z = sum_v exp(s_v - m)`` summed in one fixed order
   per path (the kernel: per thread, then lanes, then waves; PyTorch: ``sum``), with the accurate
   ``logf``.  A live beam whose ``m`` is not finite (all -inf, or any +inf) has no candidate.
5. The result is the first W candidates in the order: descending ``c``, then ascending flat index
   ``w V + v`` (lowest beam, then lowest id) - the repository's tie rule.
6. A candidate with ``c == -inf`` (or NaN) is not a candidate.  Slots with no candidate left get
   ``(-inf, parent 0, token fill, finished False)``.
7. ``new_finished = finished[parent] | (token == eos_id)`` for the filled slots; ``eos_id < 0``: never.
8. Every output is in range for any input: ``parent`` in ``[0, W)``, ``token`` in ``[0, V)`` or ``fill``.
9. ``return_logp=True`` adds ``logp`` fp32 [B, W]: for a live beam's pick its own term
   ``(s_v - m) - log Z`` - the bits that went into ``c``, so ``new_scores == scores[parent] + logp`` in
   fp32 - and 0 for a finished beam's candidate and for an empty slot.  A caller that wants the sum
   of a hypothesis' log-probabilities without the rounding of every fp32 addition adds these up in
   float64 (``GPT2LMModel.beam_search`` does).

On a HIP device with ``V <= 65536`` and ``W <= 8``: two launches of csrc/beam_step.hip (a row's top W
per workgroup, then one wave per prompt merging the ``W W`` pairs - exact, since the global top W is
contained in the union of the rows' top W under the same order), no ``[B W, V]`` tensor and nothing
read back.  Anything else: :func:`beam_step_ref`, the same definition in PyTorch over chunks of
rows.  The two paths may differ only in that a candidate value can differ by fp32 rounding, and in a
pick where two candidates from different ``(w, s_v)`` lie within that rounding of each other.

The next token: ``sample_tokens``
---------------------------------
``sample_tokens(logits [B, V], *, temperature, top_k=0, top_p=0.0, seed, step, row_base=0)`` draws
one id per row with noise that is a function of ``(seed, step, global row, id)`` alone.  For row b,
global row ``R = row_base + b`` (``seed``: its low 64 bits; ``step``: the index of the new token):

1. Scaling.  ``s_v = fp32(logit_v) / fp32(temperature)``, correctly rounded IEEE division (no
   reciprocal).  A NaN becomes -inf.  ``temperature == 0`` is ``utils.lm_sampling.greedy``.
2. Degenerate rows.  If the row's maximum is not finite (all -inf, or any +inf) the result is
   ``greedy``'s id for the row, ``thr`` is that maximum and ``kept`` is 0.  No path returns an id
   outside ``[0, V)``.
3. ``top_k``, when ``0 < top_k < V``: with kappa the ``top_k``-th largest s, keep ``s_v >= kappa``
   (ties with the k-th are kept, as in ``filter_top_k``).  Comparisons only: exact.  Any other
   ``top_k`` is off.
4. ``top_p``, when ``0 < fp32(top_p) < 1``, on what step 3 kept: ``m = max s``, ``w_v = exp(s_v - m)``,
   ``Z`` = the sum of w over the kept ids, ``G(x)`` = the sum of ``w_v`` over the kept ids with
   ``s_v > x``; keep v iff ``G(s_v) < top_p * Z``.  Equal logits are kept or dropped together and the
   maximum is always kept (``G(m) = 0``).  This differs from ``filter_top_p`` only for ties at the
   boundary, which that function splits by id.  Sums are fp32 in an order that is fixed per path
   (the kernel: per thread, then lanes, then waves; PyTorch: one cumulative sum down the sorted
   row), so the two paths can disagree where a mass lies within rounding of ``top_p * Z``.
5. The kept set is ``{v : s_v >= tau}`` for one tau per row, the smallest kept s: ``thr[b] = tau``,
   ``kept[b]`` = the size of the set.
6. The draw is Gumbel-max with counter-based uniforms.  One block of ``philox4`` (csrc/common.h)
   serves the ids ``4j .. 4j+3``: with ``V4 = ceil(V / 4)`` and the 64-bit group index
   ``grp = R * V4 + j`` it is ``philox4(seed_lo, step, grp_lo, grp_hi, seed_hi, SM_DOMAIN)`` - the
   layout of the decoding noise of csrc/reverse_step.hip under a domain constant of its own.  Word
   ``r[v & 3]`` gives ``u_v = (2 (r >> 9) + 1) / 2^24``, an odd integer below 2^24 over 2^24: exact
   in fp32 and strictly inside (0, 1).  ``g_v = -log(-log u_v)`` and the token is the arg-max of
   ``s_v + g_v`` (fp32) over the kept ids, ties to the lowest id.  ``u_v`` depends on
   ``(seed, step, R, v)`` and V only: not on B, on any launch geometry, or on training's RNG state.
   The two paths can disagree where two perturbed scores lie within rounding of each other.

fp32 or bf16 logits with last stride 1 (any row stride) and V <= 65536 on a HIP device: one kernel
per call (csrc/sample.hip), nothing read back to the host.  Anything else: the same definition in
PyTorch with the same uniform bits, :func:`sample_tokens_ref`.  ``sample_uniforms`` returns the
``u_v``, so tests and tools can pin the noise bit for bit.

The logit processors: ``penalize_logits_``
------------------------------------------
``penalize_logits_(logits [R, V], hist [R, Lh], n [R], *, start=None, repetition_penalty=1.0,
presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram=0) -> logits`` applies the four
processors that read a row's token history, in place, and returns its first argument.

* ``logits``: fp32 or bf16 for the kernel, last stride 1, any row stride and alignment; rows that
  overlap in memory (a row stride below V, such as the beam-stride-0 view of a beam search's first
  step) are refused: they would have several writers.
* ``hist``: int32 or int64 ids, any strides; ``n`` and ``start``: any integer dtype.
* theta = ``repetition_penalty`` > 0, a_p = ``presence_penalty``, a_f = ``frequency_penalty``, each
  taken as fp32; g = ``no_repeat_ngram`` >= 0.

The window of row r.  ``n[r] < 0`` leaves the row untouched (a parked row).  Otherwise
``hi = min(n[r], Lh)``, ``lo = clamp(start[r], 0, Lh)`` (0 without ``start``), the window is
``w = hist[r, lo:hi]`` and ``m = max(hi - lo, 0)``.  Nothing outside the window is read for its value;
what lies beyond ``hi`` never influences the result.

Counts and bans.  ``c(x)`` is the number of positions of w that hold x.  With g >= 1 the banned set
is ``Bn = { w[i] : g - 1 <= i < m and w[i-g+1 .. i-1] == w[m-g+1 .. m-1] }``: every id that would
complete a g-gram the window already holds.  g = 1 bans every id of the window; ``m < g`` or g = 0
bans nothing.

The update, for every x in ``[0, V)`` with ``c(x) >= 1``, exactly once per distinct x, each step one
fp32 rounding:

1. ``s = fp32(logits[r, x])``;
2. ``s = s * theta if s < 0 else s / theta`` (correctly rounded division);
3. ``s = s - (a_p + a_f * fp32(c(x)))``: the multiply and the add are separate roundings (no FMA);
4. ``s = -inf`` if x is in Bn;
5. ``logits[r, x] = s`` rounded to the dtype of ``logits`` (round to nearest even).

So the order is repetition penalty, then presence / frequency penalty, then the ban.  Ids of the
window outside ``[0, V)`` take part in the n-gram comparison and write nothing.  Every other element
keeps its bits; a NaN stays a NaN unless its id is banned.  The window is whatever the caller puts
into ``hist`` - prompt and output alike, or with ``start`` the output alone - where conventions that
penalise "output only" or "prompt and output" differ in nothing else.

fp32 or bf16 logits on a HIP device with ``Lh <= 2048``: one launch of csrc/logit_penalty.hip, one
workgroup per row, no sweep over V, no workspace, no atomics, nothing read back.  Anything else (CPU,
other dtypes, a longer history): :func:`penalize_logits_ref`, the same definition with the same fp32
operations in PyTorch over chunks of rows; it gives the kernel's bits.  With every scalar at its
default nothing is done at all.

Teacher-forced scoring: ``token_stats``
---------------------------------------
``token_stats(logits [R, V], targets [R]) -> (logp fp32 [R], rank int32 [R], entropy fp32 [R], top1
int32 [R])``: how the row's distribution stands to one given id.  Per row, with target t:

1. ``s_v = fp32(logit_v)``.  A NaN becomes -inf and -0 becomes +0 (``beam_step``'s conditioning).
2. ``m = max_v s_v``; ``top1`` is the lowest id holding m.  If m is not finite (all -inf, or any +inf),
   ``logp`` and ``entropy`` are NaN; ``rank`` and ``top1`` are comparisons only and stay defined.
3. ``Z = sum_v exp(s_v - m)`` with the accurate ``expf``, ``lz = logf(Z)`` and ``logp = (s_t - m) - lz``,
   the expression ``beam_step`` uses for a pick's term.  A target logit of -inf gives -inf.
4. ``entropy = lz - (sum_v exp(s_v - m) (s_v - m)) / Z``, in nats; an id with ``s_v = -inf``
   contributes exactly 0 (no ``0 * -inf``).
5. ``rank = #{v : s_v > s_t} + #{v < t : s_v == s_t}``: 0-based, the target's place in the order (value
   descending, id ascending) - the repository's tie rule - so ``rank == 0`` iff ``top1 == t``.
6. t outside ``[0, V)`` is how a caller says "ignore": ``logp = 0`` and ``rank = -1``; ``entropy`` and
   ``top1`` are still the row's.

Both sums are fp32 in an order that is fixed per path (the kernel: per thread in register order, then
lanes, then waves; PyTorch: ``sum``).  ``targets`` holds integers of any dtype and stride; an int64
value beyond 32 bits is outside.

fp32 or bf16 logits with last stride 1 (any row stride and alignment) and ``1 <= V <= 65536`` on a HIP
device: one launch of csrc/token_stats.hip, one workgroup per row, the row read once into registers,
one 4-byte store per output and row, no workspace, no atomics, nothing read back: two calls agree bit
for bit.  Anything else (CPU, other dtypes, a larger V): :func:`token_stats_ref`, the same definition
in fp32 PyTorch over chunks of rows.  The two paths may differ by fp32 rounding in the two floats;
the two integers are exact on both.
"""
import math
import struct

import torch

from ._ext import get_ext

SM_DOMAIN = 0x536D706C  # csrc/sample.hip
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def _check_table(src, beams, R, Lmax):
    W = int(beams)
    if not 1 <= W <= 255:
        raise ValueError(f"beams must be in 1 .. 255, got {beams}")
    if R % W:
        raise ValueError(f"{R} cache rows are not whole groups of {W} beams")
    if src.dtype != torch.uint8 or tuple(src.shape) != (R, Lmax):
        raise ValueError(f"src must be uint8 [{R}, {Lmax}], got {src.dtype} {tuple(src.shape)}")
    return W


def attention_decode_ref(qkv_new, k_cache, v_cache, lens, n_heads, *, src=None, beams=1):
    """The definition in fp32 PyTorch (any device, any dtype); also the numerics yardstick of
    the kernel's tests.  With ``src`` the effective caches of every row are gathered first."""
    B, H, Lmax, D = k_cache.shape
    assert H == n_heads and qkv_new.shape == (B, 3 * H * D) and lens.shape == (B,)
    W = 1 if src is None else _check_table(src, beams, B, Lmax)
    q, k, v = qkv_new.detach().reshape(B, 3, H, D).unbind(1)
    n = lens.long()
    active = (n >= 0) & (n < Lmax)
    at = n.clamp(0, Lmax - 1)
    rows = torch.arange(B, device=qkv_new.device)
    keep = active.view(B, 1, 1)
    # the append: an inactive row writes back what its slot already holds
    k_cache[rows, :, at] = torch.where(keep, k.to(k_cache.dtype), k_cache[rows, :, at])
    v_cache[rows, :, at] = torch.where(keep, v.to(v_cache.dtype), v_cache[rows, :, at])
    pos = torch.arange(Lmax, device=qkv_new.device).view(1, Lmax)
    mask = (pos <= at.view(B, 1)).view(B, 1, Lmax)
    ke, ve = k_cache, v_cache
    if src is not None:
        # the slot each (row, position) is read from: the table's, clamped into the group, for the
        # cached keys and the row's own for the key just appended (what lies behind is masked)
        slot = torch.where(pos < at.view(B, 1), src.long().clamp(max=W - 1), (rows % W).view(B, 1))
        from_row = (rows // W * W).view(B, 1) + slot
        # [B, H, Lmax, D], packed like a whole cache: the sums below then run as on a gathered cache
        ke = k_cache[from_row, :, pos].permute(0, 2, 1, 3).contiguous()
        ve = v_cache[from_row, :, pos].permute(0, 2, 1, 3).contiguous()
    s = torch.einsum("bhd,bhld->bhl", q.float(), ke.float()) / math.sqrt(D)
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
    vf = torch.where(mask.unsqueeze(-1), ve.float(), 0.0)  # a NaN beyond lens must not reach the sum
    o = torch.einsum("bhl,bhld->bhd", p, vf)
    return torch.where(keep, o, 0.0).to(qkv_new.dtype).reshape(B, H * D)


@torch.no_grad()
def attention_decode(qkv_new, k_cache, v_cache, lens, n_heads, *, src=None, beams=1):
    """-> out [B, H*D] in ``qkv_new``'s dtype; ``k_cache`` / ``v_cache`` updated in place.
    ``src`` uint8 [B, Lmax] with ``beams = W``: the cache indirection table of the module docstring."""
    if src is not None:
        _check_table(src, beams, k_cache.shape[0], k_cache.shape[2])
    if qkv_new.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None:
            if qkv_new.stride(-1) != 1 or qkv_new.stride(0) % 8 or qkv_new.data_ptr() % 16:
                qkv_new = qkv_new.contiguous()
            if src is None:
                out = ext.attn_decode(qkv_new, k_cache, v_cache, lens, int(n_heads))
            else:
                out = ext.attn_decode_beam(qkv_new, k_cache, v_cache, lens, int(n_heads),
                                           src if src.stride(-1) == 1 else src.contiguous(), int(beams))
            if out is not None:
                return out
    return attention_decode_ref(qkv_new, k_cache, v_cache, lens, n_heads, src=src, beams=beams)


# ---- the one-byte cache: kv_quantize, kv_store, attention_decode_fp8 ---------------------------------

def kv_quantize_ref(x):
    """The format's definition in PyTorch (any device, any float dtype) -> (codes uint8 [..., D], exp
    int8 [...]).  Non-finite values: unspecified.

    The codes are ``torch.ldexp(x.float(), -e).to(torch.float8_e4m3fn)`` with every step exact on any
    device: the exponent is read off the bits of the largest magnitude (what ``frexp`` returns, without
    its arithmetic), ``2^-e`` is assembled from its bits, and a subnormal fp32 element is scaled from
    its integer mantissa, so a device whose PyTorch kernels flush fp32 subnormals to zero or round
    ``pow(2, k)`` gives the same bytes."""
    xf = x.detach().float().contiguous()
    mag = xf.view(torch.int32) & 0x7FFFFFFF
    amax = mag.amax(-1)  # integer order is magnitude order
    E, M = amax >> 23, amax & 0x7FFFFF
    # a normal a = 1.f 2^(E - 127) has frexp (1.f / 2, E - 126); m > 0.875 is f > 0.75; a subnormal a lies
    # below the clamp
    e = (E - 135 + (M > 0x600000).to(E.dtype)).clamp(min=-127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    # 2^-e = 2^-120 .. 2^127 assembled from its bits: exact on every device (a device's powf need not be)
    scale = ((127 - e) << 23).view(torch.float32).unsqueeze(-1)
    scaled = xf * scale
    # a subnormal element M 2^-149, through normal intermediates only (an underflow to 0 rounds to 0 anyway)
    sub = torch.copysign((mag & 0x7FFFFF).float() * 2.0 ** -75 * scale * 2.0 ** -74, xf)
    codes = torch.where(mag >> 23 == 0, sub, scaled).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.view(x.shape), e.to(torch.int8)


def kv_dequantize(codes, exp):
    """-> fp32 [..., D]: ``float(code) * 2^exp``, exact, assembled from the bits so that a result
    below 2^-126 is the subnormal it should be on any device (2^128, the one overflow, is inf)."""
    f = codes.contiguous().view(torch.float8_e4m3fn).float()  # exact: zero, or a normal fp32 of 4 significant bits
    bits = f.view(torch.int32)
    e = exp.to(torch.int32).unsqueeze(-1)
    sign, mag = bits & -0x80000000, bits & 0x7FFFFFFF
    En = (mag >> 23) + e  # the result's exponent field
    normal = mag + (e << 23)
    shift = (1 - En).clamp(0, 31)
    denorm = ((mag & 0x7FFFFF) | 0x800000) >> shift  # exact: the 4 significant bits stay above bit 9
    out = torch.where(En >= 1, normal, denorm)
    out = torch.where(En >= 255, torch.full_like(out, 0x7F800000), out)
    out = torch.where((mag == 0) | (mag > 0x7F800000), mag, out)  # zero and NaN codes stay what they are
    return (out | sign).view(torch.float32).view(codes.shape)


@torch.no_grad()
def kv_quantize(x):
    """-> (codes uint8 [..., D], exp int8 [...]): the module docstring has the format."""
    if x.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None and x.dtype == torch.bfloat16 and x.numel() > 0:
            D = x.shape[-1]
            out = ext.kv8_quantize(x.detach().reshape(-1, D).contiguous())
            if out is not None:
                return out[0].view(x.shape), out[1].view(x.shape[:-1])
    return kv_quantize_ref(x)


def _check_fp8_cache(k8, ke, v8, ve):
    if k8.dim() != 4 or k8.shape != v8.shape or ke.shape != k8.shape[:3] or ve.shape != k8.shape[:3]:
        raise ValueError(f"codes must be [B, H, Lmax, D] and exponents [B, H, Lmax], got {tuple(k8.shape)}, "
                         f"{tuple(ke.shape)}, {tuple(v8.shape)}, {tuple(ve.shape)}")
    if k8.dtype != torch.uint8 or v8.dtype != torch.uint8 or ke.dtype != torch.int8 or ve.dtype != torch.int8:
        raise ValueError(f"codes must be uint8 and exponents int8, got {k8.dtype}, {ke.dtype}, {v8.dtype}, {ve.dtype}")


def kv_store_ref(qkv, lens, k8, ke, v8, ve):
    """The prefill's store in PyTorch (any device, any float dtype): a position at or beyond ``lens[b]``
    writes back what its slot already holds."""
    _check_fp8_cache(k8, ke, v8, ve)
    B, H, Lmax, D = k8.shape
    L = qkv.shape[1]
    if qkv.shape[0] != B or qkv.shape[2] != 3 * H * D or tuple(lens.shape) != (B,) or L > Lmax:
        raise ValueError(f"qkv {tuple(qkv.shape)} and lens {tuple(lens.shape)} do not fit caches {tuple(k8.shape)}")
    kv = qkv.detach().reshape(B, L, 3, H, D)
    inside = torch.arange(L, device=qkv.device).view(1, L) < lens.to(qkv.device).view(B, 1)
    for c8, ce, part in ((k8, ke, kv[:, :, 1]), (v8, ve, kv[:, :, 2])):
        codes, ex = kv_quantize_ref(part)  # [B, L, H, D], [B, L, H]
        c8[:, :, :L] = torch.where(inside.view(B, 1, L, 1), codes.permute(0, 2, 1, 3), c8[:, :, :L])
        ce[:, :, :L] = torch.where(inside.view(B, 1, L), ex.permute(0, 2, 1), ce[:, :, :L])


@torch.no_grad()
def kv_store(qkv, lens, k8, ke, v8, ve):
    """Quantize K and V of ``qkv`` [B, L, 3*H*D] into the caches for the positions below ``lens``, in
    place: the module docstring has the definition."""
    _check_fp8_cache(k8, ke, v8, ve)
    if qkv.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None and qkv.dim() == 3:
            x = qkv
            if x.stride(-1) != 1 or x.stride(0) % 8 or x.stride(1) % 8 or x.data_ptr() % 16:
                x = x.contiguous()
            if ext.kv8_store(x, lens, k8, ke, v8, ve):
                return
    kv_store_ref(qkv, lens, k8, ke, v8, ve)


def attention_decode_fp8_ref(qkv_new, k8, ke, v8, ve, lens, n_heads):
    """The definition in fp32 PyTorch (any device, any float dtype); also the numerics yardstick of the
    kernel's tests."""
    _check_fp8_cache(k8, ke, v8, ve)
    B, H, Lmax, D = k8.shape
    assert H == n_heads and qkv_new.shape == (B, 3 * H * D) and lens.shape == (B,)
    q, k, v = qkv_new.detach().reshape(B, 3, H, D).unbind(1)
    n = lens.long()
    active = (n >= 0) & (n < Lmax)
    at = n.clamp(0, Lmax - 1)
    rows = torch.arange(B, device=qkv_new.device)
    # the append: an inactive row writes back what its slot already holds
    for c8, ce, new in ((k8, ke, k), (v8, ve, v)):
        codes, ex = kv_quantize_ref(new)
        c8[rows, :, at] = torch.where(active.view(B, 1, 1), codes, c8[rows, :, at])
        ce[rows, :, at] = torch.where(active.view(B, 1), ex, ce[rows, :, at])
    pos = torch.arange(Lmax, device=qkv_new.device).view(1, Lmax)
    mask = (pos <= at.view(B, 1)).view(B, 1, Lmax)
    # what lies beyond lens - any byte, a NaN code, a wild exponent - must not reach a sum
    kf = torch.where(mask.unsqueeze(-1), kv_dequantize(k8, ke), 0.0)
    vf = torch.where(mask.unsqueeze(-1), kv_dequantize(v8, ve), 0.0)
    s = torch.einsum("bhd,bhld->bhl", q.float(), kf) / math.sqrt(D)
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
    o = torch.einsum("bhl,bhld->bhd", p, vf)
    return torch.where(active.view(B, 1, 1), o, 0.0).to(qkv_new.dtype).reshape(B, H * D)


@torch.no_grad()
def attention_decode_fp8(qkv_new, k8, ke, v8, ve, lens, n_heads):
    """-> out [B, H*D] in ``qkv_new``'s dtype; the four cache tensors updated in place.  The module
    docstring has the definition."""
    _check_fp8_cache(k8, ke, v8, ve)
    if qkv_new.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None:
            if qkv_new.stride(-1) != 1 or qkv_new.stride(0) % 8 or qkv_new.data_ptr() % 16:
                qkv_new = qkv_new.contiguous()
            out = ext.attn_decode_fp8(qkv_new, k8, ke, v8, ve, lens, int(n_heads))
            if out is not None:
                return out
    return attention_decode_fp8_ref(qkv_new, k8, ke, v8, ve, lens, n_heads)


# ---- attention_decode_block, lookup_draft (lookahead decoding) -----------------------------------

BLOCK_MAX = 8  # the largest block of csrc/attn_decode_block.hip


def _check_block(qkv_new, k_cache, lens, n_heads, counts):
    if qkv_new.dim() != 3 or k_cache.dim() != 4:
        raise ValueError(f"qkv_new must be [B, T, 3*H*D] and the caches [B, H, Lmax, D], got "
                         f"{tuple(qkv_new.shape)}, {tuple(k_cache.shape)}")
    B, H, _, D = k_cache.shape
    T = qkv_new.shape[1]
    if not 1 <= T <= BLOCK_MAX:
        raise ValueError(f"a block holds 1 .. {BLOCK_MAX} tokens, got T = {T}")
    if H != n_heads or tuple(qkv_new.shape) != (B, T, 3 * H * D) or tuple(lens.shape) != (B,):
        raise ValueError("shapes of qkv_new, the caches, lens and n_heads do not agree")
    if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (B,)):
        raise ValueError(f"counts must be int32 [{B}], got {counts.dtype} {tuple(counts.shape)}")
    return B, T


def attention_decode_block_ref(qkv_new, k_cache, v_cache, lens, n_heads, *, counts=None):
    """The definition as written (any device, any dtype): T ``attention_decode_ref`` calls, call j
    with ``lens + j`` for the rows with ``j < c_b`` and -1 for the others."""
    B, T = _check_block(qkv_new, k_cache, lens, n_heads, counts)
    Lmax = k_cache.shape[2]
    n = lens.long()
    c = torch.full_like(n, T) if counts is None else counts.to(n.device).long()
    c = torch.where((n >= 0) & (n < Lmax), torch.minimum(c.clamp(0, T), Lmax - n), 0)
    outs = [attention_decode_ref(qkv_new[:, j], k_cache, v_cache, torch.where(j < c, n + j, -1).to(torch.int32),
                                 n_heads) for j in range(T)]
    return torch.stack(outs, 1)


@torch.no_grad()
def attention_decode_block(qkv_new, k_cache, v_cache, lens, n_heads, *, counts=None):
    """-> out [B, T, H*D] in ``qkv_new``'s dtype; ``k_cache`` / ``v_cache`` updated in place.  The
    module docstring has the definition."""
    _check_block(qkv_new, k_cache, lens, n_heads, counts)
    if qkv_new.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None:
            if (qkv_new.stride(-1) != 1 or qkv_new.stride(0) % 8 or qkv_new.stride(1) % 8
                    or qkv_new.data_ptr() % 16):
                qkv_new = qkv_new.contiguous()
            out = ext.attn_decode_block(qkv_new, k_cache, v_cache, lens, int(n_heads),
                                        None if counts is None else counts.contiguous())
            if out is not None:
                return out
    return attention_decode_block_ref(qkv_new, k_cache, v_cache, lens, n_heads, counts=counts)


@torch.no_grad()
def lookup_draft(history, n, *, ngram, max_draft):
    """-> (draft int64 [B, max_draft], k int64 [B]): the module docstring has the definition."""
    g, M = int(ngram), int(max_draft)
    if g < 1 or M < 0:
        raise ValueError(f"ngram must be >= 1 and max_draft >= 0, got {ngram}, {max_draft}")
    B, Lh = history.shape
    dev = history.device
    n = n.to(device=dev, dtype=torch.long).clamp(0, Lh)
    if Lh < g + 1 or M == 0:
        return torch.zeros(B, M, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
    win = history.unfold(1, g, 1)  # [B, Lh - g + 1, g]: window i is s[i : i + g]
    nw = Lh - g + 1
    rows = torch.arange(B, device=dev)
    suffix = win[rows, (n - g).clamp(0, nw - 1)]  # s[n - g : n] where n >= g
    start = torch.arange(nw, device=dev).view(1, nw)
    hit = (win == suffix.unsqueeze(1)).all(-1) & (start <= (n - g - 1).view(B, 1))
    i = torch.where(hit, start, -1).amax(1)  # the latest earlier occurrence, -1: none
    found = i >= 0
    p = (n - g - i).clamp(min=1)
    at = i.view(B, 1) + g + torch.arange(M, device=dev).view(1, M) % p.view(B, 1)
    draft = torch.where(found.view(B, 1), history.gather(1, at.clamp(0, Lh - 1)), 0)
    return draft, torch.where(found, M, 0)


# ---- sample_tokens ------------------------------------------------------------------------------

def _s64(x):
    """The low 64 bits of a Python int as a signed int64 (two's complement)."""
    x = int(x) & _M64
    return x - (1 << 64) if x >> 63 else x


def _mulhilo(m, c):
    """(hi, lo) words of the 64-bit product m * c: m a 32-bit constant, c an int64 tensor of 32-bit
    values.  The product does not fit a signed int64, so c is split into 16-bit halves."""
    ch, cl = c >> 16, c & 0xFFFF
    ph, pl = ch * m, cl * m                    # < 2^48 each; product = ph * 2^16 + pl
    low = ((ph & 0xFFFF) << 16) + pl           # < 2^49
    return (ph >> 16) + (low >> 32), low & _M32


def _philox4(k0, k1, c0, c1, c2, c3):
    """csrc/common.h philox4 on int64 tensors (or ints) holding 32-bit words -> four words."""
    for _ in range(7):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def sample_uniforms_ref(seed, step, row_base, B, V, device="cpu"):
    """The uniforms of ``sample_tokens`` in integer tensor ops (any device) -> fp32 [B, V]."""
    seed = int(seed) & _M64
    V4 = (V + 3) // 4
    rows = torch.arange(B, dtype=torch.int64, device=device) + _s64(row_base)
    grp = rows.view(B, 1) * V4 + torch.arange(V4, dtype=torch.int64, device=device).view(1, V4)  # mod 2^64
    zero = torch.zeros_like(grp)
    r = _philox4(seed & _M32, int(step) & _M32, grp & _M32, (grp >> 32) & _M32, zero + (seed >> 32),
                 zero + SM_DOMAIN)
    r = torch.stack(r, -1).reshape(B, 4 * V4)[:, :V]
    return (2 * (r >> 9) + 1).float() * (1.0 / 16777216.0)


@torch.no_grad()
def sample_uniforms(seed, step, row_base, B, V, device="cpu"):
    """-> fp32 [B, V]: ``u_v`` of the module docstring for the rows ``row_base .. row_base + B - 1``.
    On a HIP device the kernel's own values (csrc/sample.hip, V <= 65536), elsewhere the replica."""
    device = torch.device(device)
    if device.type == "cuda":
        ext = get_ext()  # raises on a GPU without the built extension
        if ext is not None:
            out = ext.sample_uniforms(torch.empty(0, device=device), _s64(seed), int(step) & _M32, _s64(row_base),
                                      int(B), int(V))
            if out is not None:
                return out
    return sample_uniforms_ref(seed, step, row_base, B, V, device)


def _fp32(x):
    """The float nearest to ``x`` that fp32 holds (what a kernel argument becomes)."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


@torch.no_grad()
def sample_tokens_ref(logits, *, temperature, top_k=0, top_p=0.0, seed, step, row_base=0, uniforms=None):
    """The definition in PyTorch (any device, any float dtype) -> (tokens int64 [B], thr fp32 [B],
    kept int32 [B]).  ``uniforms``: the ``u_v`` to use instead of computing them."""
    from utils.lm_sampling import greedy
    B, V = logits.shape
    dev = logits.device
    s = logits.float() / torch.full((1,), float(temperature), dtype=torch.float32, device=dev)  # a true division
    s = torch.where(torch.isnan(s), float("-inf"), s) + 0.0  # -0 -> +0
    m = s.amax(-1, keepdim=True)
    thr = s.amin(-1, keepdim=True)
    if 0 < top_k < V:
        thr = torch.topk(s, int(top_k), dim=-1).values[:, -1:]
    p = _fp32(top_p)
    if 0.0 < p < 1.0:
        srt = torch.sort(s, dim=-1, descending=True).values
        w = torch.where(srt >= thr, torch.exp(srt - m), 0.0)
        csum = w.cumsum(-1)
        above = torch.cat([torch.zeros_like(csum[:, :1]), csum[:, :-1]], 1)  # mass in front of each position
        # the mass strictly above a value is the one in front of the first element of its run
        pos = torch.arange(V, device=dev).view(1, V)
        first = torch.where(torch.cat([torch.ones_like(srt[:, :1], dtype=torch.bool), srt[:, 1:] != srt[:, :-1]], 1),
                            pos, 0).cummax(-1).values
        keep = (above.gather(1, first) < csum[:, -1:] * p) & (srt >= thr)
        thr = srt.gather(1, (keep.sum(-1, keepdim=True) - 1).clamp(min=0))
    keep = s >= thr
    u = sample_uniforms(seed, step, row_base, B, V, dev) if uniforms is None else uniforms
    score = torch.where(keep, s - torch.log(-torch.log(u)), float("-inf"))
    best = score.amax(-1, keepdim=True)
    ids = torch.arange(V, device=dev)
    tok = torch.where(keep & (score == best), ids, V).amin(-1).clamp(max=V - 1)
    bad = ~torch.isfinite(m.squeeze(-1))
    tok = torch.where(bad, greedy(logits), tok)
    thr = torch.where(bad, m.squeeze(-1), thr.squeeze(-1))
    kept = torch.where(bad, 0, keep.sum(-1)).to(torch.int32)
    return tok, thr, kept


@torch.no_grad()
def sample_tokens(logits, *, temperature, top_k=0, top_p=0.0, seed, step, row_base=0, return_stats=False):
    """-> tokens int64 [B], or (tokens, thr fp32 [B], kept int32 [B]) with ``return_stats``."""
    if logits.dim() != 2:
        raise ValueError(f"logits must be [B, V], got {tuple(logits.shape)}")
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    B, V = logits.shape
    if temperature == 0:
        from utils.lm_sampling import greedy
        tok = greedy(logits)
        if not return_stats:
            return tok
        s = torch.where(torch.isnan(logits), float("-inf"), logits.float())
        return tok, s.amax(-1), torch.zeros(B, dtype=torch.int32, device=logits.device)
    k = int(top_k) if 0 < top_k < V else 0
    p = _fp32(top_p)
    p = p if 0.0 < p < 1.0 else 0.0
    if logits.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None and logits.dtype in (torch.float32, torch.bfloat16) and B > 0:
            x = logits if logits.stride(-1) == 1 else logits.contiguous()
            out = ext.sample_tokens(x, float(temperature), k, p, _s64(seed), int(step) & _M32, _s64(row_base),
                                    bool(return_stats))
            if out is not None:
                return tuple(out) if return_stats else out[0]
    out = sample_tokens_ref(logits, temperature=temperature, top_k=k, top_p=p, seed=seed, step=step,
                            row_base=row_base)
    return out if return_stats else out[0]


# ---- beam_step ----------------------------------------------------------------------------------

def _check_beam_step(logits, scores, finished):
    if logits.dim() != 3:
        raise ValueError(f"logits must be [B, W, V], got {tuple(logits.shape)}")
    B, W, V = logits.shape
    if W < 1 or V < 1:
        raise ValueError(f"logits must have W >= 1 and V >= 1, got {tuple(logits.shape)}")
    if tuple(scores.shape) != (B, W) or tuple(finished.shape) != (B, W):
        raise ValueError(f"scores and finished must be [{B}, {W}], got {tuple(scores.shape)}, {tuple(finished.shape)}")
    if scores.dtype != torch.float32 or finished.dtype != torch.bool:
        raise ValueError(f"scores must be float32 and finished bool, got {scores.dtype}, {finished.dtype}")
    return B, W, V


@torch.no_grad()
def beam_step_ref(logits, scores, finished, *, eos_id=-1, fill=0, chunk=64, return_logp=False):
    """The definition in PyTorch (any device, any float dtype), at most ``chunk`` rows - one
    ``[chunk, V]`` fp32 block - at a time."""
    B, W, V = _check_beam_step(logits, scores, finished)
    dev = logits.device
    ninf = float("-inf")
    k = min(W, V)
    exists = scores > ninf  # False for a NaN too
    cand_c = torch.full((B, W, W), ninf, dtype=torch.float32, device=dev)
    cand_v = torch.zeros((B, W, W), dtype=torch.long, device=dev)
    cand_lp = torch.zeros((B, W, W), dtype=torch.float32, device=dev)
    step = max(1, int(chunk) // W)
    for b0 in range(0, B, step):
        s = logits[b0:b0 + step].float()  # [n, W, V]
        s = torch.where(torch.isnan(s), ninf, s)
        m = s.amax(-1, keepdim=True)
        d = s - m
        sc = scores[b0:b0 + step].unsqueeze(-1)
        lp = d - torch.log(torch.exp(d).sum(-1, keepdim=True))
        c = sc + lp
        live = (exists[b0:b0 + step] & ~finished[b0:b0 + step]).unsqueeze(-1) & torch.isfinite(m)
        c = torch.where(live & ~torch.isnan(c), c, ninf)
        # a stable sort keeps equal values in id order
        top, idx = torch.sort(c, dim=-1, descending=True, stable=True)
        cand_c[b0:b0 + step, :, :k] = top[..., :k]
        cand_v[b0:b0 + step, :, :k] = idx[..., :k]
        cand_lp[b0:b0 + step, :, :k] = lp.gather(-1, idx[..., :k])
    own = exists & finished  # one candidate: (score, fill), bits unchanged
    first = torch.zeros(W, dtype=torch.bool, device=dev)
    first[0] = True
    cand_c = torch.where(own.unsqueeze(-1), torch.where(first, scores.unsqueeze(-1), ninf), cand_c)
    cand_v = torch.where(own.unsqueeze(-1), int(fill), cand_v)
    # rows in beam order, a row's candidates in (c, id) order: a stable sort gives the tie rule
    new_scores, at = torch.sort(cand_c.view(B, W * W), dim=-1, descending=True, stable=True)
    new_scores, at = new_scores[:, :W], at[:, :W]
    valid = new_scores > ninf
    parent = torch.where(valid, at // W, 0)
    token = torch.where(valid, cand_v.view(B, W * W).gather(1, at), int(fill))
    new_finished = valid & (finished.gather(1, parent) | ((token == int(eos_id)) & (int(eos_id) >= 0)))
    out = (new_scores, parent.to(torch.int32), token, new_finished)
    if return_logp:
        live = valid & ~finished.gather(1, parent)
        out += (torch.where(live, cand_lp.view(B, W * W).gather(1, at), 0.0),)
    return out


@torch.no_grad()
def beam_step(logits, scores, finished, *, eos_id=-1, fill=0, return_logp=False):
    """-> (new_scores fp32, parent int32, token int64, new_finished bool), all [B, W]: the module
    docstring has the definition.  With ``return_logp`` also ``logp`` fp32 [B, W]."""
    B, W, V = _check_beam_step(logits, scores, finished)
    if logits.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None and logits.dtype in (torch.float32, torch.bfloat16) and B > 0:
            x = logits if logits.stride(-1) == 1 or V == 1 else logits.contiguous()
            out = ext.beam_step(x, scores.contiguous(), finished.contiguous(), int(eos_id), int(fill))
            if out is not None:
                return tuple(out) if return_logp else tuple(out[:4])
    return beam_step_ref(logits, scores, finished, eos_id=eos_id, fill=fill, return_logp=return_logp)


# ---- penalize_logits_ ---------------------------------------------------------------------------

PENALTY_MAX_HIST = 2048  # LP_MAX_L of csrc/logit_penalty.hip


def _check_penalty(logits, hist, n, start, theta, g):
    if logits.dim() != 2 or hist.dim() != 2 or n.dim() != 1:
        raise ValueError(f"logits must be [R, V], hist [R, Lh] and n [R], got {tuple(logits.shape)}, "
                         f"{tuple(hist.shape)}, {tuple(n.shape)}")
    R, V = logits.shape
    if hist.shape[0] != R or n.shape[0] != R or (start is not None and tuple(start.shape) != (R,)):
        raise ValueError(f"hist, n and start must have the {R} rows of logits, got {tuple(hist.shape)}, "
                         f"{tuple(n.shape)}" + ("" if start is None else f", {tuple(start.shape)}"))
    for name, t in (("hist", hist), ("n", n), ("start", start)):
        if t is not None and (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool):
            raise ValueError(f"{name} must hold integers, got {t.dtype}")
    if not logits.is_floating_point():
        raise ValueError(f"logits must be floating point, got {logits.dtype}")
    if not theta > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {theta}")
    if g < 0:
        raise ValueError(f"no_repeat_ngram must be >= 0, got {g}")
    if V > 1 and logits.stride(1) != 1:
        raise ValueError("logits must have last stride 1 (the op works in place)")
    if R > 1 and logits.stride(0) < V:
        raise ValueError(f"the rows of logits overlap in memory (row stride {logits.stride(0)} < V = {V}): "
                         "an in-place update would have several writers")


@torch.no_grad()
def penalize_logits_ref(logits, hist, n, *, start=None, repetition_penalty=1.0, presence_penalty=0.0,
                        frequency_penalty=0.0, no_repeat_ngram=0, chunk_elems=1 << 24):
    """The definition in PyTorch (any device, any float dtype), in place, over chunks of rows whose
    ``[rows, Lh, Lh]`` comparison holds at most ``chunk_elems`` elements.  The same fp32 operations as
    the kernel, one rounding each."""
    g = int(no_repeat_ngram)
    _check_penalty(logits, hist, n, start, float(repetition_penalty), g)
    R, V = logits.shape
    Lh = hist.shape[1]
    if R == 0 or V == 0 or Lh == 0:
        return logits
    dev = logits.device
    # one-element device tensors: a division by one is a true division, not a multiply by the reciprocal
    theta, a_p, a_f = (torch.full((1,), float(x), dtype=torch.float32, device=dev)
                       for x in (repetition_penalty, presence_penalty, frequency_penalty))
    n = n.to(dev).long()
    hi = n.clamp(0, Lh).view(R, 1)
    lo = torch.zeros_like(hi) if start is None else start.to(dev).long().clamp(0, Lh).view(R, 1)
    pos = torch.arange(Lh, device=dev).view(1, Lh)
    inside = (pos >= lo) & (pos < hi) & (n >= 0).view(R, 1)
    below = torch.ones(Lh, Lh, dtype=torch.bool, device=dev).tril(-1)  # [i, j]: j < i
    step = max(1, int(chunk_elems) // (Lh * Lh))
    for r0 in range(0, R, step):
        h = hist[r0:r0 + step].to(dev).long()
        rows = h.shape[0]
        inw = inside[r0:r0 + step]
        eq = (h.unsqueeze(2) == h.unsqueeze(1)) & inw.unsqueeze(2) & inw.unsqueeze(1)  # [r, i, j]
        count = eq.sum(-1)
        valid = inw & ~(eq & below).any(-1) & (h >= 0) & (h < V)  # the first occurrence of an id of [0, V)
        banned = torch.zeros_like(inw)
        if g >= 1:
            src = inw & (pos - lo[r0:r0 + step] >= g - 1)  # none when the window is shorter than g
            for t in range(g - 1 if g <= Lh else 0):
                mine = h.gather(1, (pos - (g - 1) + t).clamp(0, Lh - 1).expand(rows, Lh))
                last = h.gather(1, (hi[r0:r0 + step] - (g - 1) + t).clamp(0, Lh - 1))
                src = src & (mine == last)
            banned = (eq & src.unsqueeze(1)).any(-1)
        rr, ii = valid.nonzero(as_tuple=True)
        if rr.numel() == 0:
            continue
        x = h[rr, ii]
        view = logits[r0:r0 + step]
        s = view[rr, x].float()
        s = torch.where(s < 0, s * theta, s / theta)
        s = s - (a_p + a_f * count[rr, ii].float())
        s = torch.where(banned[rr, ii], float("-inf"), s)
        view[rr, x] = s.to(logits.dtype)
    return logits


def _as_i32(t, lowest, highest, dev):
    """``t`` as the contiguous int32 device tensor the kernel reads; values are clamped first, which
    the definition does anyway, so a wide dtype cannot wrap."""
    if t.dtype == torch.int32 and t.is_contiguous() and t.device == dev:
        return t
    return t.to(dev).clamp(lowest, highest).to(torch.int32).contiguous()


@torch.no_grad()
def penalize_logits_(logits, hist, n, *, start=None, repetition_penalty=1.0, presence_penalty=0.0,
                     frequency_penalty=0.0, no_repeat_ngram=0):
    """Repetition, presence and frequency penalty and the no-repeat-n-gram ban on ``logits`` [R, V],
    in place -> ``logits``: the module docstring has the definition."""
    theta, a_p, a_f, g = float(repetition_penalty), float(presence_penalty), float(frequency_penalty), int(no_repeat_ngram)
    _check_penalty(logits, hist, n, start, theta, g)
    if theta == 1.0 and a_p == 0.0 and a_f == 0.0 and g == 0:
        return logits
    Lh = hist.shape[1]
    if logits.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if (ext is not None and logits.dtype in (torch.float32, torch.bfloat16) and Lh <= PENALTY_MAX_HIST
                and hist.dtype in (torch.int32, torch.int64) and hist.device == logits.device):
            dev = logits.device
            if ext.penalize_logits(logits, hist, _as_i32(n, -1, Lh, dev),
                                   None if start is None else _as_i32(start, 0, Lh, dev), theta, a_p, a_f, g):
                return logits
    return penalize_logits_ref(logits, hist, n, start=start, repetition_penalty=theta, presence_penalty=a_p,
                               frequency_penalty=a_f, no_repeat_ngram=g)


# ---- token_stats --------------------------------------------------------------------------------

STATS_REF_ELEMS = 1 << 22  # fp32 scores one chunk of rows of token_stats_ref may hold (16 MiB per temporary)


def _check_token_stats(logits, targets):
    if logits.dim() != 2 or targets.dim() != 1 or targets.shape[0] != logits.shape[0]:
        raise ValueError(f"logits must be [R, V] and targets [R], got {tuple(logits.shape)}, {tuple(targets.shape)}")
    if not logits.is_floating_point():
        raise ValueError(f"logits must be floating point, got {logits.dtype}")
    if targets.is_floating_point() or targets.is_complex() or targets.dtype == torch.bool:
        raise ValueError(f"targets must hold integers, got {targets.dtype}")
    if logits.shape[1] < 1:
        raise ValueError("logits must have V >= 1")


@torch.no_grad()
def token_stats_ref(logits, targets, *, chunk_elems=STATS_REF_ELEMS):
    """The definition in fp32 PyTorch (any device, any float dtype) -> (logp fp32, rank int32, entropy
    fp32, top1 int32), all [R], over chunks of rows that hold at most ``chunk_elems`` scores."""
    _check_token_stats(logits, targets)
    R, V = logits.shape
    dev = logits.device
    ninf, nan = float("-inf"), float("nan")
    logp = torch.empty(R, dtype=torch.float32, device=dev)
    ent = torch.empty(R, dtype=torch.float32, device=dev)
    rank = torch.empty(R, dtype=torch.int32, device=dev)
    top1 = torch.empty(R, dtype=torch.int32, device=dev)
    ids = torch.arange(V, device=dev).view(1, V)
    step = max(1, int(chunk_elems) // V)
    for r0 in range(0, R, step):
        s = logits[r0:r0 + step].float()
        s = torch.where(torch.isnan(s), ninf, s) + 0.0  # -0 -> +0
        t = targets[r0:r0 + step].to(dev).long().view(-1, 1)
        scored = ((t >= 0) & (t < V)).view(-1)
        tc = t.clamp(0, V - 1)
        m = s.amax(-1, keepdim=True)
        fin = torch.isfinite(m).view(-1)
        st = s.gather(1, tc)
        d = s - m
        p = torch.exp(d)
        Z = p.sum(-1)
        lz = torch.log(Z)
        S = torch.where(d > ninf, p * d, 0.0).sum(-1)
        lp = (st - m).view(-1) - lz
        logp[r0:r0 + step] = torch.where(scored, torch.where(fin, lp, nan), 0.0)
        ent[r0:r0 + step] = torch.where(fin, lz - S / Z, nan)
        ahead = (s > st).sum(-1) + ((s == st) & (ids < tc)).sum(-1)
        rank[r0:r0 + step] = torch.where(scored, ahead, -1).to(torch.int32)
        top1[r0:r0 + step] = torch.where(s == m, ids, V).amin(-1).to(torch.int32)
    return logp, rank, ent, top1


@torch.no_grad()
def token_stats(logits, targets):
    """-> (logp fp32 [R], rank int32 [R], entropy fp32 [R], top1 int32 [R]): the module docstring has
    the definition."""
    _check_token_stats(logits, targets)
    if logits.is_cuda:
        ext = get_ext()  # raises on a GPU without the built extension: no quiet fall-back
        if ext is not None and logits.dtype in (torch.float32, torch.bfloat16) and logits.shape[0] > 0:
            t = targets.to(logits.device)
            if t.dtype not in (torch.int32, torch.int64):
                t = t.long()
            out = ext.token_stats(logits, t)
            if out is not None:
                return tuple(out)
    return token_stats_ref(logits, targets)
