// Next-token choice of GPT-2 generation as one kernel: temperature, top-k, top-p and the draw on a
// [B, V] logits tensor, one workgroup per row (ops/decode.py sample_tokens holds the definition).
//
// A row's V <= 65536 scaled logits s_v = logit_v / temperature (IEEE division; NaN -> -inf) live in
// registers for the whole kernel: thread t of 1024 owns the ids 4 j .. 4 j + 3 of the groups
// j = t + 1024 i, i < NG = ceil(ceil(V / 4) / 1024) (the template parameter) - the ids one Philox
// block serves.  Ids >= V hold NaN, which fails every comparison and so never counts, never adds
// mass and never wins.  Rows are read with scalar loads: V = 50257 is odd, so neither a bf16 nor an
// fp32 row starts on a vector boundary, and the row is read once.
//
// Both filters keep a set {v : s_v >= tau}.  Floats are mapped to order-preserving uint32 keys and
// the threshold key is built bit by bit from the top:
//   top-k:  kappa = the largest c with count(key >= c) >= k      (integers: exact, ties kept)
//   top-p:  tau   = the largest c with mass(key >= c) >= top_p Z  (w_v = exp(s_v - max); v is kept
//           iff the mass strictly above it is < top_p Z, which is the same set)
// at most 32 block reductions each; a candidate above the row's maximum or not above the current
// lower bound is decided without one.  Every mass is an fp32 sum in one fixed order - a thread's
// values in register order, the 64 lanes by xor butterfly (every lane ends with the same bits), the
// 16 waves in wave order - so it is monotone in each term and hence in c, and bitwise reproducible.
//
// The draw is Gumbel-max: u_v from philox4(seed_lo, step, grp_lo, grp_hi, seed_hi, SM_DOMAIN) with
// the 64-bit group index grp = (row_base + b) ceil(V / 4) + j, the layout of reverse_step.hip's
// noise; g_v = -log(-log u_v) with the accurate logf (winners mostly have u within 1e-6 of 1, where
// -log u ~ 3e-8 and the fast log has no relative accuracy); the token is the arg-max of s_v + g_v
// over the kept ids, ties to the lowest id.  u_v depends on (seed, step, global row, v) and V only:
// not on B, the launch geometry or training's g_rng_base.
//
// No workspace, no second launch, no atomics; nothing is read back to the host.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "launchers.h"
#include "row_block.h"  // keys, wave and block reductions (shared with beam_step.hip)

namespace dpa {

// distinguishes the token draws from the decoding noise (RS_DOMAIN) and every training stream
constexpr uint32_t SM_DOMAIN = 0x536D706Cu;

// u = (2 (r >> 9) + 1) / 2^24: an odd integer below 2^24 over 2^24, exact in fp32, inside (0, 1)
__device__ __forceinline__ void sm_uniform4(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint64_t grp,
                                            float u[4]) {
  uint32_t r[4];
  philox4(seed_lo, step, (uint32_t)grp, (uint32_t)(grp >> 32), seed_hi, SM_DOMAIN, r);
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = (float)(2u * (r[k] >> 9) + 1u) * (1.0f / 16777216.0f);
}

// One thread's share of mass(s >= x), w = exp(s - max) = 2^(s log2 e - ml2): four running sums, one per
// id of a group, added up at the end - always in this order.  The scheduling barrier keeps the
// compiler from computing every exponential before the first add (64 more live registers).
template <int NG>
__device__ __forceinline__ float sm_thread_mass(const float (&s)[NG][4], float x, float ml2) {
  float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NG; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += (s[i][e] >= x) ? fexp2(fmaf(s[i][e], LOG2E, -ml2)) : 0.f;
    __builtin_amdgcn_sched_barrier(0);
  }
  return (a[0] + a[1]) + (a[2] + a[3]);
}

template <int NG, bool BF16>
__global__ void __launch_bounds__(SM_THREADS) sample_tokens_kernel(
    const void* __restrict__ logits, int64_t row_stride, int V, float temperature, int top_k, float top_p,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint64_t row_base, int64_t* __restrict__ tokens,
    float* __restrict__ thr, int* __restrict__ kept) {
  __shared__ sm_red_t red;
  __shared__ float best_s_w[SM_WAVES];
  __shared__ int best_i_w[SM_WAVES];
  int ph = 0;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int V4 = (V + 3) >> 2;
  const float ninf = -INFINITY;

  // ---- the row: scale, NaN -> -inf, -0 -> +0; its largest and smallest key ----
  float s[NG][4];
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // branch-free, so that the row's loads are all in flight together: an id >= V reads id V - 1
      const int64_t at = b * row_stride + min(4 * (tid + i * SM_THREADS) + e, V - 1);
      s[i][e] = BF16 ? __uint_as_float((uint32_t)((const bf16_t*)logits)[at]) : ((const float*)logits)[at];
    }
  // the loads first, as raw bits (a use right behind a load would wait for it), and then one division
  // at a time: with up to 64 values per thread there is no room for the temporaries of several
  __builtin_amdgcn_sched_barrier(0);
  float smax = ninf, smin = INFINITY;  // an id >= V holds a copy of id V - 1, which moves neither
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = __fdiv_rn(BF16 ? __uint_as_float(__float_as_uint(s[i][e]) << 16) : s[i][e], temperature);
      if (x != x) x = ninf;
      if (x == 0.f) x = 0.f;
      smax = fmaxf(smax, x);
      smin = fminf(smin, x);
      s[i][e] = x;
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * (tid + i * SM_THREADS) + e >= V) s[i][e] = __builtin_nanf("");
  const uint32_t M = sm_block_umax(sm_key(smax), red, ph);
  const uint32_t L = ~sm_block_umax(~sm_key(smin), red, ph);
  const float m = sm_unkey(M);

  // ---- a maximum that is not finite: greedy's id (the lowest id that holds it) ----
  if (!(fabsf(m) < INFINITY)) {
    uint32_t nid = 0u;  // ~(lowest id)
#pragma unroll
    for (int i = 0; i < NG; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (s[i][e] == m) nid = max(nid, ~(uint32_t)(4 * (tid + i * SM_THREADS) + e));
    const uint32_t id = ~sm_block_umax(nid, red, ph);
    if (tid == 0) {
      tokens[b] = (int64_t)min(id, (uint32_t)(V - 1));
      if (thr) thr[b] = m;
      if (kept) kept[b] = 0;
    }
    return;
  }

  uint32_t lo = L;  // the kept set is {key >= lo}
  // ---- top-k: the largest c with count(key >= c) >= k ----
  if (top_k > 0 && top_k < V) {
    uint32_t c = 0u;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = c | (1u << bit);
      bool take;
      if (cand > M) take = false;
      else if (cand <= lo) take = true;
      else {
        // a wave's count per compare, on the scalar unit (every lane is active here)
        const float x = sm_unkey(cand);
        int n = 0;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
#pragma unroll
          for (int e = 0; e < 4; ++e) n += __popcll(__ballot(s[i][e] >= x));
          __builtin_amdgcn_sched_barrier(0);  // four lane masks at a time, not 4 NG of them
        }
        take = sm_block_wave_count(n, red, ph) >= top_k;
      }
      if (take) c = cand;
    }
    lo = c;
  }
  // ---- top-p on what is left: the largest c with mass(key >= c) >= top_p Z ----
  if (top_p > 0.f && top_p < 1.f) {
    const float ml2 = m * LOG2E;
    const float xlo = sm_unkey(lo);
    const float target = top_p * sm_block_mass(sm_thread_mass<NG>(s, xlo, ml2), red, ph);
    uint32_t c = 0u;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = c | (1u << bit);
      bool take;
      if (cand > M) take = false;
      else if (cand <= lo) take = true;
      else {
        // the exponentials do not change from pass to pass, and with NG <= 8 the compiler is free
        // to hoist them out of this loop and keep them in registers; beyond that they do not fit
        // beside s (hoisted, NG = 13 and 16 spill), so the empty asm hides that ml2 is constant
        // and they are computed again in every pass
        float ml2v = ml2;
        if (NG > 8) asm volatile("" : "+v"(ml2v));
        take = sm_block_mass(sm_thread_mass<NG>(s, sm_unkey(cand), ml2v), red, ph) >= target;
      }
      if (take) c = cand;
    }
    lo = c;
  }

  // ---- the draw over {s >= tau}: arg-max of s + g, ties to the lowest id ----
  const float tau = sm_unkey(lo);
  const uint64_t grp0 = (row_base + (uint64_t)b) * (uint64_t)V4;
  int n = 0;
  float bs = ninf;
  int bi = INT_MAX;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int j = tid + i * SM_THREADS;
    if (s[i][0] >= tau || s[i][1] >= tau || s[i][2] >= tau || s[i][3] >= tau) {
      float u[4];
      sm_uniform4(seed_lo, seed_hi, step, grp0 + (uint64_t)j, u);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (s[i][e] >= tau) {
          ++n;
          const float sc = s[i][e] - logf(-logf(u[e]));
          const int v = 4 * j + e;
          if (sc > bs || (sc == bs && v < bi)) { bs = sc; bi = v; }
        }
      }
    }
  }
  n = sm_block_count(n, red, ph);
  sm_wave_argmax(bs, bi);
  if ((tid & 63) == 0) { best_s_w[tid >> 6] = bs; best_i_w[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < SM_WAVES; ++w) {
      const float os = best_s_w[w];
      const int oi = best_i_w[w];
      if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    tokens[b] = (int64_t)min(bi, V - 1);
    if (thr) thr[b] = tau;
    if (kept) kept[b] = n;
  }
}

__global__ void __launch_bounds__(256) sample_uniforms_kernel(float* __restrict__ out, int64_t B, int V,
                                                              uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                              uint64_t row_base) {
  const int64_t V4 = (V + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * V4) return;
  const int64_t b = idx / V4, j = idx - b * V4;
  float u[4];
  sm_uniform4(seed_lo, seed_hi, step, (row_base + (uint64_t)b) * (uint64_t)V4 + (uint64_t)j, u);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (4 * j + e < V) out[b * V + 4 * j + e] = u[e];
}

template <int NG>
static void sm_launch(bool bf16, const void* logits, int64_t row_stride, int64_t B, int V, float temperature,
                      int top_k, float top_p, uint64_t seed, uint32_t step, uint64_t row_base, int64_t* tokens,
                      float* thr, int* kept, hipStream_t st) {
  const dim3 grid((unsigned)B), block(SM_THREADS);
  const uint32_t slo = (uint32_t)seed, shi = (uint32_t)(seed >> 32);
  if (bf16)
    hipLaunchKernelGGL((sample_tokens_kernel<NG, true>), grid, block, 0, st, logits, row_stride, V, temperature,
                       top_k, top_p, slo, shi, step, row_base, tokens, thr, kept);
  else
    hipLaunchKernelGGL((sample_tokens_kernel<NG, false>), grid, block, 0, st, logits, row_stride, V, temperature,
                       top_k, top_p, slo, shi, step, row_base, tokens, thr, kept);
}

bool launch_sample_tokens(const void* logits, bool bf16, int64_t row_stride, int64_t B, int V, float temperature,
                          int top_k, float top_p, uint64_t seed, uint32_t step, uint64_t row_base,
                          int64_t* tokens, float* thr, int* kept, hipStream_t st) {
  if (!logits || !tokens || B < 1 || B > 0x7fffffffLL || V < 1 || V > 65536 || !(temperature > 0.f)) return false;
  const int ng = ((V + 3) / 4 + SM_THREADS - 1) / SM_THREADS;  // 1 .. 16
#define SM_CASE(N)                                                                                              \
  sm_launch<N>(bf16, logits, row_stride, B, V, temperature, top_k, top_p, seed, step, row_base, tokens, thr, \
               kept, st)
  if (ng <= 1) SM_CASE(1);
  else if (ng <= 2) SM_CASE(2);
  else if (ng <= 4) SM_CASE(4);
  else if (ng <= 8) SM_CASE(8);
  else if (ng <= 13) SM_CASE(13);  // V = 50257 (GPT-2)
  else SM_CASE(16);
#undef SM_CASE
  return true;
}

bool launch_sample_uniforms(float* out, int64_t B, int V, uint64_t seed, uint32_t step, uint64_t row_base,
                            hipStream_t st) {
  if (!out || B < 1 || V < 1 || V > 65536) return false;
  const int64_t blocks = (B * (int64_t)((V + 3) / 4) + 255) / 256;
  if (blocks > 0x7fffffffLL) return false;
  hipLaunchKernelGGL(sample_uniforms_kernel, dim3((unsigned)blocks), dim3(256), 0, st, out, B, V, (uint32_t)seed,
                     (uint32_t)(seed >> 32), step, row_base);
  return true;
}

}  // namespace dpa
