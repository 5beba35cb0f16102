// Host-side launch entry points of the gfx950 kernels.  Kernels live in the
// .hip translation units (which include no torch headers, so they compile in
// seconds); only the binding TUs (bindings.cpp, bind_*.cpp, through bind_util.h) see ATen.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpa {

// ---- ipc_allreduce.hip: direct xGMI all-reduce over IPC-mapped peer buffers ----
constexpr int IPC_MAXW = 8;
struct IpcPeers {            // per rank: staging buffer (2 parity halves of `cap` floats) and flags
  float* stage[IPC_MAXW];
  uint32_t* flags[IPC_MAXW];
};
struct IpcData {             // in/out buffer of each (simulated) rank; real runs use p[rank]
  float* p[IPC_MAXW];
};
constexpr int64_t IPC_FLAG_WORDS = 4 * 1024;  // [2 parity][2 phase][IPC_NBMAX]
int ipc_allreduce_blocks(int64_t n, int W, bool two_shot);
// sim_ranks == W: one launch plays all W ranks on one device (tests); 1: this rank only.
bool launch_ipc_allreduce(const IpcPeers& peers, const IpcData& data, int W, int rank, int sim_ranks,
                          int64_t n, int64_t cap, uint32_t epoch, bool two_shot, int* err, hipStream_t s);

// ---- comm_sim.hip: one-GPU projection of the W > 1 data plane (reducer sim mode) ----
// tl: this bucket's timeline words {first start, ~last end} (both reset to all-ones)
void launch_comm_sim(void* buf, int64_t bytes, int64_t touch_bytes, uint64_t ticks, int cus,
                     unsigned long long* tl, hipStream_t s);
void launch_time_marker(unsigned long long* slot, hipStream_t s);
void launch_comm_sim_stats(const unsigned long long* tl, int nb, const unsigned long long* bwd_end,
                           unsigned long long* acc, hipStream_t s);

// ---- wgrad4w.hip: one-wave-per-SIMD weight gradient (both operands token-major) ----
bool launch_wgrad4w(const uint16_t* const* as, const uint16_t* const* bs, int nseg, int T, int M, int N, int splits,
                    int kps, float* dW, float* ws, hipStream_t s);
void set_wgrad4w(bool on);  // gemm256.hip: route db-free weight gradients to wgrad4w (default off: measured no faster)

// ---- optim.hip -------------------------------------------------------------
void launch_sqnorm(const void* g, bool g_bf16, int64_t n, float* partial, int nparts, float scale,
                   float max_norm, float* out, hipStream_t s);
void launch_adamw_ema(float* p, const void* g, bool g_bf16, float* m, float* v, uint16_t* p16,
                      float* const* ema_bufs, const float* ema_rates, int n_ema, int64_t n, float lr,
                      double beta1, double beta2, float eps, float wd, int64_t step, float grad_scale,
                      const float* clip, hipStream_t s,
                      const int* skip = nullptr);
void launch_ema(float* e, const float* p, int64_t n, float rate, hipStream_t s);
void launch_cast_bf16(const float* src, uint16_t* dst, int64_t n, hipStream_t s);
// dst_i = src_i^T for up to MAXN bf16 matrices [rows_i][cols_i] (multiples of 64), one launch;
// tile_start = prefix sums of (rows / 64) * (cols / 64), tile_start[n] = total
struct TransposeBatch {
  static constexpr int MAXN = 96;
  const uint16_t* src[MAXN];
  uint16_t* dst[MAXN];
  int rows[MAXN], cols[MAXN], tile_start[MAXN + 1];
  int n;
};
bool launch_transpose_bf16_batch(const TransposeBatch& d, hipStream_t s);
void launch_cast_f32(const uint16_t* src, float* dst, int64_t n, hipStream_t s);  // n % 4 == 0

// ---- linear_argmax.hip (fused linear + arg-max: decoding) -----------------------
// idx[t] = argmax_v (x[t] . W[v] + c[v]) (ties: lowest v), best[t] = that score; c fp32 or null;
// ws: linear_argmax_workspace_floats(N, V) floats of scratch (0: this shape is not split)
int64_t linear_argmax_workspace_floats(int N, int V);
void launch_linear_argmax(const uint16_t* x, const uint16_t* W, const float* c, int N, int V, int E,
                          int64_t* idx, float* best, float* ws, hipStream_t s);
// c[v] = -1/2 ||W[v]||^2 (fp32), E in {128, 256}
void launch_row_half_sqnorm(const uint16_t* W, int V, int E, float* c, hipStream_t s);

// ---- xent.hip (fused linear + cross-entropy) ----------------------------------
int64_t lxent_workspace_floats(int N, int V);
// forward + unscaled input gradient in one sweep: dxu[t] = softmax_t . W - W[target_t] (fp32)
void launch_lxent_fwd_dx(const uint16_t* x, const uint16_t* W, const uint16_t* b, const int64_t* tgt,
                         int N, int V, int E, float* loss, float* lse, float* dxu, hipStream_t s,
                         float* ws = nullptr);
// fp32 workspace of the vocabulary-split fused forward (0: no split for this shape)
int64_t lxent_fwd_dx_workspace_floats(int N, int V, int E);
bool lxent_dx_needs_acc(int N);
void launch_lxent_fwd(const uint16_t* x, const uint16_t* W, const uint16_t* b, const int64_t* tgt,
                      int N, int V, int E, float* loss, float* lse, float* ws, hipStream_t s);
void launch_lxent_dx(const uint16_t* x, const uint16_t* W, const uint16_t* b, const int64_t* tgt,
                     const float* lse, const float* dloss, int N, int V, int E, uint16_t* dx,
                     float* dx_acc, hipStream_t s);
// dW (+ db) += the head gradient; ws: lxent_dw_ws_floats(N, V, E) floats of scratch when that is
// > 0 (the token splits' partials, summed in split order: deterministic)
int64_t lxent_dw_ws_floats(int N, int V, int E);
void launch_lxent_dw(const uint16_t* x, const uint16_t* W, const uint16_t* b, const int64_t* tgt,
                     const float* lse, const float* dloss, int N, int V, int E, float* dW, float* db,
                     hipStream_t s, bool onehot, float* ws);

// ---- norm.hip (fused dropout + residual + LayerNorm) ---------------------------
bool launch_add_ln_fwd(const uint16_t* y, const uint16_t* res, const uint16_t* g, const uint16_t* b,
                       uint16_t* out, uint16_t* hsave, float* mean, float* rstd, int64_t R, int D,
                       float p, float eps, uint32_t seed, uint32_t off, hipStream_t s,
                       const uint16_t* pos = nullptr, const uint16_t* temb = nullptr, int L = 1,
                       bool post = false, bool hguard = false);  // hguard: write hsave only if some |gamma| is small
int ln_bwd_blocks(int64_t R);
// dyb (nullable): column sums of dy (the bias gradient of the layer producing y)
bool launch_add_ln_bwd(const uint16_t* dout, const uint16_t* hsave, const float* mean,
                       const float* rstd, const uint16_t* g, uint16_t* dres, uint16_t* dy, float* dyb,
                       float* dg, float* db, int64_t R, int D, float p, uint32_t seed, uint32_t off,
                       hipStream_t s, const uint16_t* dh_in = nullptr, bool post = false,
                       int zero_mask = 7, float* ws = nullptr, int part_mode = 0,
                       const uint16_t* beta = nullptr,    // beta: `hsave` is the LN output ...
                       const uint16_t* hcopy = nullptr,   // ... and hcopy the guarded h copy
                       bool pair_hash = false);           // dy's dropout bits: common.h pair_hash
// the deferred second stage of part_mode 1/2 (R = the rows of each summed micro-batch); consumes
// the partials (ordered two-pass sums, no atomics)
bool launch_ln_colreduce(float* part, int64_t R, int D, float* dg, float* db, float* dyb, hipStream_t s);
// dpos[L][H] (zeroed; += sum over b) and dtemb[B][H] (= sum over l) of a [B][L][H] bf16 gradient in
// one read; part: seq_pos_groups(B) * L * H floats of workspace.  L in {64, 128, 256}, H % 64 == 0.
int seq_pos_groups(int B);
bool launch_seq_pos_sums(const uint16_t* d, int B, int L, int H, float* dpos, float* dtemb, float* part,
                         hipStream_t s);
// dst[c] += sum_r part[r][c] in a fixed order (deterministic); consumes part
bool launch_colsum_acc(float* part, int rows, int cols, float* dst, hipStream_t s);
// fp32 workspace (floats) the small-R two-stage column sums of launch_add_ln_bwd use (0: none)
int64_t ln_bwd_ws_floats(int64_t R, int D);

// ---- elementwise.hip (bias + activation epilogues) -------------------------------
void launch_bias_act_fwd(uint16_t* z, const uint16_t* bias, uint16_t* y, int64_t R, int N, int act,
                         hipStream_t s);
// db (nullable) += column sums of dz, through ws = bias_act_bwd_ws_floats(R, N) floats of scratch
// (row-block partials summed in order: deterministic); ws is required when db is given
int64_t bias_act_bwd_ws_floats(int64_t R, int N);
void launch_bias_act_bwd(const uint16_t* dy, const uint16_t* zy, uint16_t* dz, float* db, int64_t R,
                         int N, int act, hipStream_t s, float* ws);

// ---- attention.hip (head_dim 64 or 128, dropout, causal) ---------------------------------
// head_major: qkv is [B, 3H, L, D] (QKV GEMM head-major store; L == 128, D == 64, bidirectional only)
bool launch_attn_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int B, int L, int H, int D,
                     float p, bool causal, uint32_t seed, uint32_t offset, hipStream_t s,
                     bool head_major = false);
bool attn128_supports(int L, int D, bool causal);
bool attn_bwd_needs_dq_acc(int L);
// attention128.hip: persistent L = 128 bidirectional kernels (false: not applicable)
bool launch_attn128_bwd_d128(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse,
                             float* delta, uint16_t* dqkv, int B, int L, int H, float p, bool causal,
                             uint32_t seed, uint32_t offset, hipStream_t s, float* colpart = nullptr);
// attention backward bias-gradient partials: rows of the colpart scratch ([rows][3 D] fp32) and
// the reduce pass db[3 H D] += column sums
int64_t attn_colpart_rows(int B, int L, int H, int D, bool causal);
void launch_colpart_reduce(float* colpart, float* db, int R, int H, int D, hipStream_t s);  // consumes colpart
bool launch_attn128_fwd_d128(const uint16_t* qkv, uint16_t* out, float* lse, int B, int L, int H,
                             float p, bool causal, uint32_t seed, uint32_t offset, hipStream_t s);
bool launch_attn128_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int B, int L, int H,
                        float p, bool causal, uint32_t seed, uint32_t offset, hipStream_t s,
                        bool head_major = false);
// colpart [B*H][192] fp32 scratch; when dbias != nullptr also writes the column sums of
// dqkv (the qkv bias gradient) into dbias [3*H*64] (overwritten).
bool launch_attn128_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout,
                        const float* lse, uint16_t* dqkv, float* colpart, float* dbias, int B,
                        int L, int H, float p, bool causal, uint32_t seed, uint32_t offset,
                        hipStream_t s, bool head_major = false, bool db_accumulate = false,
                        bool defer_reduce = false);
// Returns true when the column sums of dqkv were written to dbias (L == 128 path).  defer_reduce:
// the column-sum partials stay in colpart (dbias untouched) for one launch_colpart_reduce over
// several calls' partials (the reference schedule's deferral window).
bool launch_attn_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse,
                     float* delta, uint16_t* dqkv, float* dq_acc, float* colpart, float* dbias, int B,
                     int L, int H, int D, float p, bool causal, uint32_t seed, uint32_t offset,
                     hipStream_t s, bool head_major = false, bool db_accumulate = false,
                     bool defer_reduce = false);

// ---- xent_rows.hip: row softmax-CE over materialised logits (wide-E chunked path) ----
// forward that leaves softmax - onehot (unscaled) in place of the logits (false: row too long)
bool launch_xent_rows_fwd_grad(uint16_t* lg, int64_t ld, int V, const int64_t* tgt, int64_t R, float* loss,
                               float* lse, hipStream_t s);
bool launch_xent_rows_fwd(const uint16_t* lg, int64_t ld, int V, const int64_t* tgt, int64_t R,
                          float* loss, float* lse, hipStream_t s);
bool launch_xent_rows_bwd(uint16_t* lg, int64_t ld, int V, const int64_t* tgt, const float* lse,
                          const float* dloss, int64_t R, hipStream_t s);

// ---- diffusion.hip: DiffuSeq q_sample / diffusion losses / timestep embedding ------
bool launch_emb_qsample_fwd(const int64_t* ids, const int64_t* mask, const int64_t* t, const float* W,
                            const float* sa, const float* s1a, int64_t NT, int L, int E, int V,
                            float std0, uint32_t seed, uint32_t offset, float* x_start,
                            uint16_t* x_start16, uint16_t* x_t, hipStream_t s);
// Deterministic segment sums over a STABLE sort: part = emb_grad_part_floats(NT, E, qsample) fp32
// scratch (qsample: for launch_emb_qsample_bwd, else launch_emb_grad)
int64_t emb_grad_part_floats(int64_t NT, int E, bool qsample);
bool launch_emb_grad(const int64_t* sorted_ids, const int64_t* perm, const float* dy32, const uint16_t* dy16,
                     int64_t NT, int E, int V, float* dW, float* part, hipStream_t s);
bool launch_emb_qsample_bwd(const int64_t* ids, const int64_t* mask, const int64_t* t, const float* sa,
                            const float* d_xs, const uint16_t* d_xs16, const uint16_t* d_xt16,
                            const float* d_xt32, int64_t NT, int L, int E, int V, float* dW,
                            hipStream_t s, const int64_t* sorted_ids = nullptr,
                            const int64_t* perm = nullptr, float* part = nullptr);
bool launch_diff_loss_fwd(const float* x_start, const void* out, bool out_bf16, const int64_t* ids,
                          const int64_t* t, const float* W, int B, int L, int E, int V, float sa_last,
                          float* mse, float* tT, hipStream_t s);
bool launch_diff_loss_bwd(const float* x_start, const void* out, bool out_bf16, const int64_t* ids,
                          const int64_t* t, const float* W, const float* dmse, const float* dtT, int B,
                          int L, int E, int V, float sa_last, void* d_out, float* d_xs, float* dW,
                          hipStream_t s, bool fold_t0 = false);  // fold_t0: the t == 0 W term into d_xs
void launch_timestep_emb(const float* ts, int B, int dim, float max_period, uint16_t* out,
                         hipStream_t s);

// ---- reverse_step.hip: one DiffuSeq reverse-process update (decoding) ------------------
// out[n] = mask[n] == 0 ? x_start[n] : a x0[n] + b x[n] + s z[n], x0 = pred (bf16) or scale * W[idx[n]]
// (ids outside [0, V): a zero row); z from Philox keyed by (seed, step) and counted by the global
// group index ((row_base + n) E + c) / 4, truncated to [-tau, tau] when tau > 0 (erf_tau =
// erf(tau / sqrt 2)).  x may be null when b == 0, pred / idx / W when a == 0, mask / x_start and
// out16 (the bf16 copy) always.  false: E % 4 != 0, N <= 0 or a required pointer is null.
// a_prev != 0 (DPM-Solver++ 2M) adds a_prev x0_prev[n] on the same rows, x0_prev = pred_prev (bf16) or
// scale * W[idx_prev[n]], and draws nothing; it needs one of the two (false otherwise).  a_prev == 0
// is the three-term kernel, which reads neither: both may be null.
bool launch_reverse_step(const float* x, const uint16_t* pred, const int64_t* idx, const float* W,
                         const float* x_start, const int64_t* mask, int64_t N, int E, int V, float scale,
                         float a, float b, float s, uint64_t seed, uint32_t step, uint64_t row_base,
                         float tau, float erf_tau, float* out, uint16_t* out16, hipStream_t st,
                         const uint16_t* pred_prev = nullptr, const int64_t* idx_prev = nullptr,
                         float a_prev = 0.f);

// ---- attn_decode.hip: KV-cache append + single-query attention (GPT-2 generation) -------
// Row b with 0 <= lens[b] < Lmax: cache[b, h, lens[b]] = the new k / v of qkv_new ([B][3][H][D] bf16,
// rows qkv_stride elements apart), out[b, h] = softmax(q K^T / sqrt D) V over the keys 0 .. lens[b]
// (bf16 [B][H][D]); any other lens[b]: nothing stored, out row zeros.  Cache rows of D elements at
// base + b * sb + h * sh + key * D; rows at or beyond lens[b] + 1 are never read; lens is not
// modified.  false, with no launch: D not in {64, 128}, a stride that is no multiple of 8 elements,
// an empty shape or a null pointer.  Bases must be 16-byte aligned.
bool launch_attn_decode(const uint16_t* qkv_new, int64_t qkv_stride, uint16_t* k_cache, uint16_t* v_cache,
                        int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* lens, int B, int H,
                        int Lmax, int D, uint16_t* out, hipStream_t s);
// The same step through a cache indirection table (beam search): rows in groups of W (B % W == 0),
// src uint8 [B][Lmax] with rows src_stride bytes apart; active row b reads cached key t < lens[b] from
// cache row (b / W) W + min(src[b][t], W - 1) and appends at its own (b, lens[b]).  src is not
// modified and src[b][t], t >= lens[b], is never read.  With src[b][t] == b % W everywhere the results
// are launch_attn_decode's bit for bit.  The caller guarantees that no active row reads a (slot,
// position) another active row of the call appends to (equal lens within a group's active rows).
// false, with no launch: as above, or W outside 1 .. 255, B % W != 0, src_stride < Lmax, Lmax > 2^30.
bool launch_attn_decode_beam(const uint16_t* qkv_new, int64_t qkv_stride, uint16_t* k_cache, uint16_t* v_cache,
                             int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* lens,
                             const uint8_t* src, int64_t src_stride, int W, int B, int H, int Lmax, int D,
                             uint16_t* out, hipStream_t s);

// ---- attn_decode_fp8.hip: the same step over a one-byte cache, and the quantizing stores ----------
// The format (the file's header has it in full): a row of D values is D e4m3fn codes of x 2^-e and one
// int8 exponent e = max(p - 9 + (m > 0.875), -127) from (m, p) = frexp(max |x|), 0 for a zero row.
// Code rows of D bytes at base + b * sb + h * sh + key * D, exponents at ebase + b * esb + h * esh + key.
// launch_attn_decode with K^, V^ for K, V: an active row quantizes its new k and v, stores codes and
// exponents at cache row lens[b] and attends over the cached keys and the dequantized new one; an
// inactive row stores nothing and returns zeros; rows at or beyond lens[b] are never read.  false, with
// no launch: D not in {64, 128}, qkv_stride no multiple of 8 elements, a code stride no multiple of 16
// bytes, a base that is not 16-byte aligned, an empty shape or a null pointer.
bool launch_attn_decode_fp8(const uint16_t* qkv_new, int64_t qkv_stride, uint8_t* k8, int8_t* ke, uint8_t* v8,
                            int8_t* ve, int64_t k_sb, int64_t k_sh, int64_t ke_sb, int64_t ke_sh, int64_t v_sb,
                            int64_t v_sh, int64_t ve_sb, int64_t ve_sh, const int* lens, int B, int H, int Lmax, int D,
                            uint16_t* out, hipStream_t s);
// The prefill's store: K and V of qkv [B][L][3][H][D] bf16 (row b, position l at b * qkv_sb + l * qkv_sl
// elements) quantized into cache row l for every l < lens[b]; nothing else is written.  false, with no
// launch: as above, or L > Lmax.
bool launch_kv8_store(const uint16_t* qkv, int64_t qkv_sb, int64_t qkv_sl, const int* lens, uint8_t* k8, int8_t* ke,
                      uint8_t* v8, int8_t* ve, int64_t k_sb, int64_t k_sh, int64_t ke_sb, int64_t ke_sh, int64_t v_sb,
                      int64_t v_sh, int64_t ve_sb, int64_t ve_sh, int B, int L, int H, int Lmax, int D, hipStream_t s);
// x [rows][D] bf16, packed -> codes [rows][D], exps [rows].
bool launch_kv8_quantize(const uint16_t* x, int64_t rows, int D, uint8_t* codes, int8_t* exps, hipStream_t s);

// ---- attn_decode_block.hip: the same step for a block of T new tokens per row (lookahead decoding) ----
// qkv_new [B][T][3][H][D] bf16 (row b, token j at b * qkv_sb + j * qkv_st elements), counts [B] int32
// or null (= T), out [B][T][H][D] bf16.  With c_b = 0 for lens[b] outside [0, Lmax) and otherwise
// clamp(counts[b], 0, min(T, Lmax - lens[b])), the call equals T launch_attn_decode calls, call j on
// token j with lens[b] + j where j < c_b and -1 elsewhere - bit for bit, each query keeping the plain
// kernel's fold order: tokens j < c_b are stored at cache rows lens[b] + j and attend over the keys
// 0 .. lens[b] + j, queries j >= c_b store nothing and return zeros, cache rows at or beyond
// lens[b] + c_b are neither read nor written, lens and counts are not modified.  T == 1 without
// counts is launch_attn_decode itself.  false, with no launch: as launch_attn_decode, or T outside
// 1 .. 8, or qkv_st no multiple of 8.
bool launch_attn_decode_block(const uint16_t* qkv_new, int64_t qkv_sb, int64_t qkv_st, uint16_t* k_cache,
                              uint16_t* v_cache, int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh,
                              const int* lens, const int* counts, int B, int T, int H, int Lmax, int D,
                              uint16_t* out, hipStream_t s);

// ---- beam_step.hip: log-softmax + score + top-W of W V candidates (beam search) ----------
// logits [B][W][V] fp32 or bf16 (element strides stride_b, stride_w >= 0 - 0 repeats a row - and 1),
// scores fp32 [B][W], finished bytes [B][W] -> the first W candidates of each b in the order
// (descending c, ascending beam, ascending id): a live beam's c(w, v) = scores + ((s_v - max) - log Z),
// a finished beam's one candidate (w, fill) at its score, none for a beam at -inf or a row whose
// maximum is not finite.  new_scores fp32, parent int32, token int64, new_finished bytes, all [B][W];
// slots without a candidate hold (-inf, 0, fill, 0).  logp (may be null) fp32 [B][W]: a live pick's own
// term (s_v - max) - log Z, the bits that went into its c; 0 for a finished beam's candidate and an
// empty slot.  Workspace: ws_c B W (W + 2) floats, ws_v B W W ints.
// Two launches, no atomics.  false, with no launch: W outside 1 .. 8, V outside 1 .. 65536, B < 1, a
// negative stride or a null pointer.
bool launch_beam_step(const void* logits, bool bf16, int64_t stride_b, int64_t stride_w, int64_t B, int W, int V,
                      const float* scores, const uint8_t* finished, int eos_id, int fill, float* ws_c, int* ws_v,
                      float* new_scores, int* parent, int64_t* token, uint8_t* new_finished, float* logp,
                      hipStream_t st);

// ---- token_stats.hip: teacher-forced statistics of logits rows against target ids (scoring) ----
// For every row r of logits ([R][V] fp32 or bf16, rows row_stride >= 0 elements apart, any alignment) and
// its target t = targets[r * t_stride] (int32, or int64 with t64): with s = fp32(logit), NaN -> -inf and
// -0 -> +0, m = max s, Z = sum exp(s - m): logp[r] = (s_t - m) - log Z, rank[r] = #{s_v > s_t} +
// #{v < t : s_v == s_t}, entropy[r] = log Z - (sum exp(s_v - m) (s_v - m)) / Z (an id at -inf adds 0),
// top1[r] = the lowest id holding m.  m not finite: logp and entropy NaN.  t outside [0, V): logp 0 and
// rank -1.  One launch, one workgroup per row, no workspace, no atomics.  false, with no launch: V outside
// 1 .. 65536, R outside 1 .. 2^31 - 1, a negative row stride or a null pointer.
bool launch_token_stats(const void* logits, bool bf16, int64_t row_stride, int64_t R, int V, const void* targets,
                        bool t64, int64_t t_stride, float* logp, int* rank, float* entropy, int* top1,
                        hipStream_t st);

// ---- sample.hip: temperature / top-k / top-p next-token draw (GPT-2 generation) ---------
// tokens[b] = the id drawn for row b of logits ([B][V] fp32 or bf16, rows row_stride elements apart, any
// alignment): s = logit / temperature, top_k (0 < top_k < V, ties with the k-th kept), top_p (0 < top_p <
// 1) on what is left, then Gumbel-max with Philox uniforms keyed by (seed, step) and counted by the global
// group index (row_base + b) ceil(V / 4) + v / 4.  A row whose maximum is not finite gets the lowest id
// holding it.  thr / kept (either may be null): the smallest kept s and the size of the kept set (the
// maximum and 0 for such a row).  One launch, no workspace.  false, with no launch: V outside 1 .. 65536,
// B outside 1 .. 2^31 - 1, temperature not > 0, or a null pointer.
bool launch_sample_tokens(const void* logits, bool bf16, int64_t row_stride, int64_t B, int V, float temperature,
                          int top_k, float top_p, uint64_t seed, uint32_t step, uint64_t row_base,
                          int64_t* tokens, float* thr, int* kept, hipStream_t st);
// out[b][v] = the uniform u_v in (0, 1) that launch_sample_tokens draws with (fp32 [B][V], contiguous).
bool launch_sample_uniforms(float* out, int64_t B, int V, uint64_t seed, uint32_t step, uint64_t row_base,
                            hipStream_t st);

// ---- logit_penalty.hip: repetition / presence / frequency penalty and n-gram ban, in place ----
// For every row r of logits ([R][V] fp32 or bf16, rows row_stride elements apart and not overlapping, any
// alignment) with n[r] >= 0: the window is hist[r][lo .. hi), hi = min(n[r], Lh), lo = clamp(start[r], 0,
// Lh) (0 with start == nullptr); hist holds int32 or int64 ids, element strides hs_r and hs_l.  Each
// distinct id x of the window inside [0, V), seen c times, is updated once: s = logit, s = s < 0 ? s theta
// : s / theta, s = s - (alpha_p + alpha_f c), each step one fp32 rounding, and s = -inf when x would
// complete a g-gram that the window already holds (g >= 1).  Nothing else is written and nothing beyond
// hi is read.  One launch, one workgroup per row, no workspace, no atomics.  false, with no launch: Lh
// outside 1 .. LP_MAX_L, R outside 1 .. 2^31 - 1, V < 1, theta not > 0, g < 0, or a null pointer.
constexpr int LP_MAX_L = 2048;
bool launch_logit_penalty(void* logits, bool bf16, int64_t row_stride, int64_t R, int V, const void* hist,
                          bool hist64, int64_t hs_r, int64_t hs_l, int Lh, const int* n, const int* start,
                          float theta, float alpha_p, float alpha_f, int g, hipStream_t st);

// ---- ngram_match.hip: clipped n-gram match counts of sequence pairs (MBR, BLEU) --------
// m[g][i][j][n-1] = sum over the distinct n-grams y of min(count_i(y), count_j(y)), n = 1..4, for the
// K sequences tokens[g][k][0 .. lens[g][k]) of every group (ids there in [0, 2^31); lens clamped to
// [0, L]; int32 or int64 ids).  Exact integers, no atomics.  false: a shape outside 1 <= K <= 16,
// 1 <= L <= 256, 1 <= G < 2^31, or a null pointer.
bool launch_ngram_match(const void* tokens, bool tok64, const int* lens, int64_t G, int K, int L, int* m,
                        hipStream_t st);

// ---- ngram_distinct.hip: distinct n-gram counts per sequence and per group (dist-n, div-n) ----
// d[g][k][n-1] = number of distinct n-grams of tokens[g][k][0 .. lens[g][k]) for k < K, d[g][K][n-1] =
// number of distinct n-grams of the union of the group's K sequences, n = 1..4 (the conventions of
// launch_ngram_match; d int32 [G, K + 1, 4]).  Exact integers, no global atomics.  false, with no
// launch: a shape outside 1 <= K <= 16, 1 <= L <= 256, 1 <= G < 2^31, or a null pointer.
bool launch_ngram_distinct(const void* tokens, bool tok64, const int* lens, int64_t G, int K, int L, int* d,
                           hipStream_t st);

// ---- lcs.hip: longest-common-subsequence lengths of sequence pairs (ROUGE-L) ------------
// out[g][i][j] = LCS length of tokens[g][i][0 .. lens[g][i]) and tokens[g][j][0 .. lens[g][j]) (ids
// there in [0, 2^31); lens clamped to [0, L]; int32 or int64 ids; out int32 [G, K, K]).  Exact
// integers, no atomics.  false, with no launch: a shape outside 1 <= K <= 16, 1 <= L <= 256,
// 1 <= G < 2^31 / 136, or a null pointer.
bool launch_lcs_lengths(const void* tokens, bool tok64, const int* lens, int64_t G, int K, int L, int* out,
                        hipStream_t st);

// ---- sort.hip: counting sort of token ids, stable 0/1 partition ---------------------
// STABLE counting sort of ids into V + 1 buckets (out-of-range ids -> bucket V); ws:
// id_sort_workspace_ints(n, V) ints.  Equal ids end up adjacent in index order (the same
// permutation on every run).  false: V + 1 > 81920 or n == 0.
int64_t id_sort_workspace_ints(int64_t n, int V);
bool launch_id_bucket_sort(const int64_t* ids, int64_t n, int V, int* ws, int64_t* sorted, int64_t* perm,
                           hipStream_t s);
// order = indices of the nonzero mask entries, then of the zero ones, each in index order
int64_t partition01_workspace_ints(int64_t n);
bool launch_partition01(const int64_t* mask, int64_t n, int* blk_ws, int64_t* order, hipStream_t s);

// ---- gemm.hip (bf16 MFMA GEMMs of Linear layers) ----------------------------------
bool launch_gemm_nt(const uint16_t* x, const uint16_t* W, const uint16_t* bias, uint16_t* y,
                    uint16_t* z, int T, int N, int K, int act, hipStream_t s,
                    bool* zderiv = nullptr, int hm = 0);
bool launch_gemm_nn(const uint16_t* dy, const uint16_t* W, uint16_t* dx, int T, int N, int K,
                    hipStream_t s, const uint16_t* WT = nullptr);
bool launch_gemm_wgrad(const uint16_t* dy, const uint16_t* x, float* dW, float* db, int T, int N,
                       int K, hipStream_t s, float* ws = nullptr);
// gemm256.hip: 256x256 8-phase variants (return false when the shape does not tile
// or DPA_GEMM256=0); the launch_gemm_* entry points try them first.
bool launch_gemm256_nt(const uint16_t* x, const uint16_t* W, const uint16_t* bias, uint16_t* y,
                       uint16_t* z, int T, int N, int K, int act, hipStream_t s);
bool launch_gemm256_nn(const uint16_t* dy, const uint16_t* W, uint16_t* dx, int T, int N, int K,
                       hipStream_t s);
void set_gemm256(bool on);
void set_gemmp_dynamic(bool on);  // dynamic tile schedule of the persistent GEMMs (world > 1)
void set_gemmp_grid_cap(int cap);  // persistent-GEMM grid cap (0 = #CUs)
void set_gemmp_half(int mode);     // 128-row tiles: 0 off, 1 auto (occupancy rule), 2 always
bool launch_gemm256_nn_dact(const uint16_t* dy, const uint16_t* W, const uint16_t* aux,
                            uint16_t* dz, int T, int N, int K, int act, hipStream_t s);
bool launch_gemm256_wgrad(const uint16_t* dy, const uint16_t* x, float* dW, float* db, int T,
                          int N, int K, hipStream_t s, float* ws = nullptr);
// fp32 workspace the split-K weight gradient merges through (0: atomics / no split)
int64_t gemm256_wgrad_workspace_floats(int T, int N, int K, int nseg = 1);
// dW += sum_s dy_s^T x_s over nseg (<= 8) equal token segments in one split-K launch
bool launch_gemm256_wgrad_multi(const uint16_t* const* dys, const uint16_t* const* xs, int nseg, float* dW,
                                float* db, int T, int N, int K, hipStream_t s, float* ws);
// Grouped weight gradient of several Linears (the deferral flush): site i adds
// sum_s a[s]^T b[s] (a: dy [T][M], b: x [T][N], bf16) into dW [M][N] fp32 (+ colsum[M] += column
// sums of the dy segments when colsum != null); one workgroup per 256 x 256 tile, no token split.
// The table is filled on the host (wgrad_group_prepare: tile0, returns the tile total or -1 when a
// site does not tile) and passed in device memory.
struct WgGroupSite {
  const uint16_t* a[8];
  const uint16_t* b[8];
  float* dW;
  float* colsum;
  int nseg, M, N, ktiles, tile0, pad[3];
};
int wgrad_group_prepare(WgGroupSite* sites, int nsites);
bool launch_wgrad_group(const WgGroupSite* d_sites, int nsites, int ntiles, hipStream_t s);
// gemm256.hip persistent forward / data-gradient kernels with fused epilogues (false when
// the shape does not tile).  ncu: compute units (grid = min(tiles, ncu)).
//   nt: y[T][N] = act(x[T][K] W[N][K]^T + bias); z (nullable) = pre-activation, or act'(it)
//       when zderiv (backward act code 4 multiplies by it)
//   nn: dx[T][K] = dy[T][N] W[N][K] (* act'(aux[T][K]) when aux; act 4: * aux); colpart (nullable, needs
//       aux): per-tile column-sum partials [(T/256)*2][K] of dx (the bias gradient)
//       z8 (with zderiv): act'(z) as u8 codes in a tile-native layout ([T * N] bytes; only the
//       persistent data-gradient kernel reads it: launch_gemmp_nn act 5)
bool launch_gemmp_nt(const uint16_t* x, const uint16_t* W, const uint16_t* bias, uint16_t* y,
                     uint16_t* z, int T, int N, int K, int act, int ncu, hipStream_t s,
                     bool zderiv = false, int hm = 0, bool z8 = false);
//   nt_res: h[T][N] = res + dropout_p(x W^T + bias), pair-hash dropout bits (common.h pair_hash)
bool launch_gemmp_nt_res(const uint16_t* x, const uint16_t* W, const uint16_t* bias, const uint16_t* res,
                         uint16_t* h, int T, int N, int K, int ncu, hipStream_t s, float p, uint32_t seed,
                         uint32_t offset);
// WT (optional): W^T [K][N] bf16 - the data gradient then takes the row-form operand path
bool launch_gemmp_nn(const uint16_t* dy, const uint16_t* W, uint16_t* dx, const uint16_t* aux, int act,
                     int T, int N, int K, int ncu, hipStream_t s, float* colpart, const uint16_t* WT = nullptr);
bool launch_gemmp_nn_acc(const uint16_t* dy, const uint16_t* W, uint16_t* dx, int T, int N, int K, int ncu,
                         hipStream_t s, const uint16_t* WT = nullptr);
int device_cu_count();
// bump the device-side Philox offset base of each translation unit that draws numbers
// (common.h g_rng_base: graph replays)
void rng_base_add_attention(uint32_t d, hipStream_t s);
void rng_base_add_attention128(uint32_t d, hipStream_t s);
void rng_base_add_diffusion(uint32_t d, hipStream_t s);
void rng_base_add_norm(uint32_t d, hipStream_t s);
void rng_base_add_gemm256(uint32_t d, hipStream_t s);

}  // namespace dpa
