// Teacher-forced statistics of logits rows [R, V] against one target id per row: the target's
// log-probability, its 0-based rank, the row's entropy and its arg-max - without a log-softmax, a sort
// or any [R, V] temporary (ops/decode.py token_stats holds the definition).
//
//   token_stats_kernel   one workgroup of 1024 threads per row, rows in the grid's x dimension.  The row's
//                        V <= 65536 logits are read once into registers with beam_rows_kernel's mapping
//                        (thread t owns the ids 4 j .. 4 j + 3, j = t + 1024 i; NaN -> -inf, -0 -> +0, ids
//                        >= V hold -inf); the target's logit is one more broadcast load, conditioned the
//                        same way.  Five block reductions of row_block.h, one barrier each:
//                          m     the maximum, on keys;
//                          top1  the lowest id holding m: the maximum of ~id over those ids;
//                          rank  the count of ids in front of the target in the order (value descending,
//                                id ascending);
//                          Z     the sum of exp(s - m), and
//                          S     the sum of exp(s - m) (s - m), an id at -inf contributing 0 - both per
//                                thread in register order, lanes by xor butterfly, waves in wave order.
//                        logp = (s_t - m) - log Z, the expression of beam_step's picks; entropy =
//                        log Z - S / Z.  A maximum that is not finite gives NaN for both; rank and top1
//                        are comparisons and stay defined.  A target outside [0, V) gives logp 0, rank -1.
//
// One 4-byte store per output and row, no atomics, no workspace: two calls give identical bits.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "launchers.h"
#include "row_block.h"

namespace dpa {

template <int NG, bool BF16>
__global__ void __launch_bounds__(SM_THREADS) token_stats_kernel(
    const void* __restrict__ logits, int64_t row_stride, int V, const void* __restrict__ targets, bool t64,
    int64_t t_stride, float* __restrict__ logp, int* __restrict__ rank, float* __restrict__ entropy,
    int* __restrict__ top1) {
  __shared__ sm_red_t red;
  int ph = 0;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float ninf = -INFINITY;
  const float qnan = __uint_as_float(0x7fc00000u);

  // the target: an id outside [0, V) (a 64-bit value beyond 32 bits included) means "ignore"
  const int64_t tv = t64 ? ((const int64_t*)targets)[row * t_stride] : (int64_t)((const int*)targets)[row * t_stride];
  const bool scored = tv >= 0 && tv < (int64_t)V;
  const int t = scored ? (int)tv : 0;

  // ---- the row and the target's logit: NaN -> -inf, -0 -> +0, ids >= V -> -inf; the maximum ----
  const int64_t base = row * row_stride;
  float s[NG][4];
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // branch-free, so that the row's loads are all in flight together: an id >= V reads id V - 1
      const int64_t at = base + min(4 * (tid + i * SM_THREADS) + e, V - 1);
      s[i][e] = BF16 ? __uint_as_float((uint32_t)((const bf16_t*)logits)[at]) : ((const float*)logits)[at];
    }
  float st = BF16 ? __uint_as_float((uint32_t)((const bf16_t*)logits)[base + t]) : ((const float*)logits)[base + t];
  __builtin_amdgcn_sched_barrier(0);
  if (BF16) st = __uint_as_float(__float_as_uint(st) << 16);
  if (st != st) st = ninf;
  if (st == 0.f) st = 0.f;
  float smax = ninf;
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = BF16 ? __uint_as_float(__float_as_uint(s[i][e]) << 16) : s[i][e];
      if (x != x || 4 * tid >= V - (4 * i * SM_THREADS + e)) x = ninf;  // id >= V, on one register for all ids
      if (x == 0.f) x = 0.f;  // -0 -> +0: the key order needs it
      smax = fmaxf(smax, x);
      s[i][e] = x;
    }
  const float m = sm_unkey(sm_block_umax(sm_key(smax), red, ph));

  // ---- top1 (the lowest id holding m: the largest ~id) and the ids in front of the target ----
  uint32_t low = 0;  // below every ~id of an id < 2^31
  int front = 0;
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = 4 * (tid + i * SM_THREADS) + e;
      const float x = s[i][e];
      if (x == m) low = max(low, ~(uint32_t)v);  // an id >= V can hold m = -inf, behind id 0 that does too
      // id < t against 4 tid again; an id >= V holds -inf and is never below t < V
      front += (x > st || (x == st && 4 * tid < t - (4 * i * SM_THREADS + e))) ? 1 : 0;
    }
  const int best = (int)~sm_block_umax(low, red, ph);  // < V: an id < V holds m, in front of every id >= V
  const int ahead = sm_block_count(front, red, ph);
  if (tid == 0) {  // stored here: held for the end, each would stay 16 partial results in registers
    rank[row] = scored ? ahead : -1;
    top1[row] = best;
  }

  // ---- Z and S in the fixed order ----
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  float w[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NG; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = s[i][e] - m;
      const float p = expf(d);  // exp(-inf) = 0
      a[e] += p;
      w[e] += d > ninf ? p * d : 0.f;  // not 0 * -inf
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  const float Z = sm_block_mass((a[0] + a[1]) + (a[2] + a[3]), red, ph);  // >= 1: the maximum's term
  const float S = sm_block_mass((w[0] + w[1]) + (w[2] + w[3]), red, ph);
  if (tid == 0) {
    const bool fin = fabsf(m) < INFINITY;  // else all -inf, or a +inf
    const float lz = logf(Z);
    logp[row] = !scored ? 0.f : fin ? (st - m) - lz : qnan;
    entropy[row] = fin ? lz - S / Z : qnan;
  }
}

template <int NG>
static void ts_launch(bool bf16, const void* logits, int64_t row_stride, int64_t R, int V, const void* targets,
                      bool t64, int64_t t_stride, float* logp, int* rank, float* entropy, int* top1,
                      hipStream_t st) {
  const dim3 grid((unsigned)R), block(SM_THREADS);
  if (bf16)
    hipLaunchKernelGGL((token_stats_kernel<NG, true>), grid, block, 0, st, logits, row_stride, V, targets, t64,
                       t_stride, logp, rank, entropy, top1);
  else
    hipLaunchKernelGGL((token_stats_kernel<NG, false>), grid, block, 0, st, logits, row_stride, V, targets, t64,
                       t_stride, logp, rank, entropy, top1);
}

bool launch_token_stats(const void* logits, bool bf16, int64_t row_stride, int64_t R, int V, const void* targets,
                        bool t64, int64_t t_stride, float* logp, int* rank, float* entropy, int* top1,
                        hipStream_t st) {
  if (!logits || !targets || !logp || !rank || !entropy || !top1) return false;
  if (R < 1 || R > 0x7fffffffLL || V < 1 || V > 65536 || row_stride < 0) return false;
  const int ng = ((V + 3) / 4 + SM_THREADS - 1) / SM_THREADS;  // 1 .. 16
#define TS_CASE(N) ts_launch<N>(bf16, logits, row_stride, R, V, targets, t64, t_stride, logp, rank, entropy, top1, st)
  if (ng <= 1) TS_CASE(1);
  else if (ng <= 2) TS_CASE(2);
  else if (ng <= 4) TS_CASE(4);
  else if (ng <= 8) TS_CASE(8);
  else if (ng <= 13) TS_CASE(13);  // V = 50257 (GPT-2)
  else TS_CASE(16);
#undef TS_CASE
  return true;
}

}  // namespace dpa
