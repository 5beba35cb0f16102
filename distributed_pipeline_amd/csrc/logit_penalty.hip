// The logit processors of GPT-2 generation as one in-place kernel: repetition, presence and frequency
// penalty and the no-repeat-n-gram ban on a [R, V] logits tensor, one workgroup per row
// (ops/decode.py penalize_logits_ holds the definition).
//
// All four read the row's token history and touch at most Lh of its V logits, so the kernel never
// sweeps V.  Thread t of 256 owns the positions t + 256 k, k < 8, of the window w = hist[r, lo:hi]
// (m <= LP_MAX_L ids) and keeps their ids in registers.
//
//   stage:  with 2 <= g <= m the window goes to LDS in the width of the history's dtype - an int64 id
//           outside [0, V) takes part in the n-gram comparison with all its bits.  The id table in LDS
//           (the power of two >= 2 m slots, open addressing) is cleared.  One barrier.
//   insert: per owned position whose id x lies inside [0, V): is it a ban source - do the g - 1 ids
//           in front of it equal the window's last g - 1 (a compare loop on the staged row; g = 1:
//           always)?  Then x is looked up or claimed in the table (compare-and-swap on the key, linear
//           probing; at most m of >= 2 m slots are ever taken, so a probe ends), and two LDS
//           atomics on its slot follow: tally += 1 + 65536 * source, first = min(first, position).
//           One barrier.
//   update: the owner of the first occurrence of x (first == its position) loads the logit, updates
//           it with c = tally & 0xffff, sets it to -inf when tally >> 16 != 0, and stores it.
//
// Why a table: letting every position walk the whole window with broadcast LDS reads is m^2 / 256
// compares per thread and measured 45 us at m = 1023, six times the launch; the table does m / 256
// inserts per thread.
// Which slot an id gets depends on the order of the claims, but a slot's count, source count and
// lowest position are sums and minima of integers: the result has the same bits in every run.
// Global memory sees one writer per element, no atomics and no workspace, and a banned id has no second
// writer.  Each arithmetic step is one fp32 rounding (lp_update: no FMA contraction, IEEE division).
#include <limits.h>
#include <math.h>

#include "common.h"
#include "launchers.h"

namespace dpa {

constexpr int LP_THREADS = 256;
constexpr int LP_OWN = LP_MAX_L / LP_THREADS;  // positions per thread at the longest window
constexpr int LP_SLOTS = 2 * LP_MAX_L;         // the largest id table
constexpr int LP_SRC = 1 << 16;                // a ban source's share of a tally; counts stay below it
static_assert(LP_MAX_L < LP_SRC && LP_MAX_L <= INT_MAX / LP_SRC, "count and source count share one int");

// s < 0 ? s theta : s / theta, minus (alpha_p + alpha_f c): four fp32 operations, one rounding each.
// __fmul_rn and __fadd_rn are plain * and + in this toolchain, which device code contracts into an FMA
// by default, so contraction is switched off for the block; the flag stays with the operations when
// the function is inlined.
__device__ __forceinline__ float lp_update(float s, float theta, float alpha_p, float alpha_f, float c) {
#pragma clang fp contract(off)
  s = (s < 0.f) ? s * theta : __fdiv_rn(s, theta);
  const float per_count = alpha_f * c;
  const float penalty = alpha_p + per_count;
  return s - penalty;
}

template <typename T, bool BF16>
__global__ void __launch_bounds__(LP_THREADS) logit_penalty_kernel(
    void* __restrict__ logits, int64_t row_stride, int V, const T* __restrict__ hist, int64_t hs_r, int64_t hs_l,
    int Lh, const int* __restrict__ n, const int* __restrict__ start, float theta, float alpha_p, float alpha_f,
    int g) {
  __shared__ T row[LP_MAX_L];
  __shared__ int keys[LP_SLOTS], tally[LP_SLOTS], first[LP_SLOTS];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int nr = n[r];
  if (nr < 0) return;  // a parked row
  const int hi = min(nr, Lh);
  const int lo = start ? min(max(start[r], 0), Lh) : 0;
  const int m = hi - lo;
  if (m <= 0) return;

  // ---- clear the table, stage the window (only an n-gram compare reads it); the owned ids stay in registers
  int bits = 6;
  while ((1 << bits) < 2 * m) ++bits;  // <= 12
  const int slots = 1 << bits;
  for (int s = tid; s < slots; s += LP_THREADS) {
    keys[s] = -1;
    tally[s] = 0;
    first[s] = INT_MAX;
  }
  const bool compare = g >= 2 && g <= m;
  const T* w = hist + r * hs_r + (int64_t)lo * hs_l;
  T a[LP_OWN];
#pragma unroll
  for (int k = 0; k < LP_OWN; ++k) {
    const int i = tid + k * LP_THREADS;
    a[k] = (T)-1;
    if (i < m) {
      a[k] = w[(int64_t)i * hs_l];
      if (compare) row[i] = a[k];
    }
  }
  __syncthreads();

  // ---- insert the owned ids of [0, V) ----
  int slot[LP_OWN];
#pragma unroll
  for (int k = 0; k < LP_OWN; ++k) {
    const int i = tid + k * LP_THREADS;
    slot[k] = -1;
    if (i < m && a[k] >= (T)0 && a[k] < (T)V) {
      bool source = g == 1;
      if (compare && i >= g - 1) {
        const T* mine = row + (i - g + 1);
        const T* last = row + (m - g + 1);
        source = true;
        for (int t = g - 2; t >= 0 && source; --t) source = mine[t] == last[t];
      }
      const int x = (int)a[k];
      unsigned h = ((unsigned)x * 2654435761u) >> (32 - bits);
      for (;;) {
        const int old = atomicCAS(&keys[h], -1, x);
        if (old == -1 || old == x) break;
        h = (h + 1u) & (unsigned)(slots - 1);
      }
      atomicAdd(&tally[h], 1 + (source ? LP_SRC : 0));
      atomicMin(&first[h], i);
      slot[k] = (int)h;
    }
  }
  __syncthreads();

  // ---- the update, by the owner of each first occurrence ----
#pragma unroll
  for (int k = 0; k < LP_OWN; ++k) {
    const int i = tid + k * LP_THREADS;
    if (slot[k] >= 0 && first[slot[k]] == i) {
      const int t = tally[slot[k]];
      const int64_t at = r * row_stride + (int64_t)a[k];
      float s = BF16 ? bf2f(((const bf16_t*)logits)[at]) : ((const float*)logits)[at];
      s = lp_update(s, theta, alpha_p, alpha_f, (float)(t & (LP_SRC - 1)));
      if (t >= LP_SRC) s = -INFINITY;
      if (BF16) ((bf16_t*)logits)[at] = (s != s) ? (bf16_t)0x7FC0 : f2bf(s);
      else ((float*)logits)[at] = s;
    }
  }
}

bool launch_logit_penalty(void* logits, bool bf16, int64_t row_stride, int64_t R, int V, const void* hist,
                          bool hist64, int64_t hs_r, int64_t hs_l, int Lh, const int* n, const int* start,
                          float theta, float alpha_p, float alpha_f, int g, hipStream_t st) {
  if (!logits || !hist || !n || R < 1 || R > 0x7fffffffLL || V < 1 || Lh < 1 || Lh > LP_MAX_L || !(theta > 0.f) ||
      g < 0)
    return false;
  const dim3 grid((unsigned)R), block(LP_THREADS);
#define LP_CASE(T, B)                                                                                           \
  hipLaunchKernelGGL((logit_penalty_kernel<T, B>), grid, block, 0, st, logits, row_stride, V, (const T*)hist, \
                     hs_r, hs_l, Lh, n, start, theta, alpha_p, alpha_f, g)
  if (hist64) {
    if (bf16) LP_CASE(int64_t, true);
    else LP_CASE(int64_t, false);
  } else {
    if (bf16) LP_CASE(int, true);
    else LP_CASE(int, false);
  }
#undef LP_CASE
  return true;
}

}  // namespace dpa
