// One step of beam search on logits [B, W, V]: log-softmax of every live beam's row, the beam's
// cumulative score added, and the W best of the W V candidates of each prompt - without ever
// writing a [B W, V] tensor (ops/decode.py beam_step holds the definition).
//
// Two launches (the structure with one workgroup per (b, w); a single workgroup per b sweeping its W
// rows would leave most of the chip idle at the small B of a decode step):
//
//   beam_rows_kernel   one workgroup of 1024 threads per (b, w).  The row's V <= 65536 logits live in
//                      registers as in sample.hip (thread t owns the ids 4 j .. 4 j + 3, j = t + 1024 i;
//                      NaN -> -inf, ids >= V hold -inf).  m = the row maximum, Z = the sum of
//                      exp(s - m) - a thread's values in register order, the lanes by xor butterfly,
//                      the waves in wave order (row_block.h) - and every register becomes its
//                      candidate c = score + ((s - m) - log Z).  Then W rounds of block arg-max on
//                      (c, lowest id): round j takes the best candidate strictly behind round
//                      j - 1's in that order, so nothing is marked and nothing is re-read.  The
//                      row's top W (c, id) pairs go to a [B, W, W] workspace; a finished beam writes
//                      its one candidate (score, fill) and a beam that does not exist none.
//   beam_merge_kernel  one wave per b: lane w W + j holds pair j of row w; W rounds of wave arg-max
//                      on (c, lowest w, lowest id) write the outputs.  The global top W is
//                      contained in the union of the rows' top W under the same order, so the merge
//                      is exact.  A live pick's own term (s - m) - log Z is written beside them,
//                      recomputed from its logit and the row's m and log Z (kept in the workspace).
//
// No atomics, one writer per element: two calls give identical bits.  Nothing is read back.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "launchers.h"
#include "row_block.h"

namespace dpa {

constexpr int BS_MAX_W = 8;

template <int NG, bool BF16>
__global__ void __launch_bounds__(SM_THREADS) beam_rows_kernel(
    const void* __restrict__ logits, int64_t stride_b, int64_t stride_w, int V, int W,
    const float* __restrict__ scores, const uint8_t* __restrict__ finished, int fill, float* __restrict__ ws_c,
    int* __restrict__ ws_v, float* __restrict__ ws_ml) {
  __shared__ sm_red_t red;
  __shared__ float best_s_w[2][SM_WAVES];
  __shared__ int best_i_w[2][SM_WAVES];
  int ph = 0;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;  // b W + w
  const int64_t b = row / W;
  const int w = (int)(row - b * W);
  const float ninf = -INFINITY;
  float* oc = ws_c + row * W;
  int* ov = ws_v + row * W;
  const float score = scores[row];

  // a beam that does not exist (-inf; a NaN score counts as one), or a finished one: at most one pair
  if (!(score > ninf) || finished[row]) {
    if (tid < W) {
      const bool one = score > ninf && tid == 0;
      oc[tid] = one ? score : ninf;
      ov[tid] = one ? fill : 0;
    }
    return;
  }

  // ---- the row: NaN -> -inf, ids >= V -> -inf; its maximum ----
  const int64_t base = b * stride_b + (int64_t)w * stride_w;
  float s[NG][4];
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // branch-free, so that the row's loads are all in flight together: an id >= V reads id V - 1
      const int64_t at = base + min(4 * (tid + i * SM_THREADS) + e, V - 1);
      s[i][e] = BF16 ? __uint_as_float((uint32_t)((const bf16_t*)logits)[at]) : ((const float*)logits)[at];
    }
  __builtin_amdgcn_sched_barrier(0);
  float smax = ninf;
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = BF16 ? __uint_as_float(__float_as_uint(s[i][e]) << 16) : s[i][e];
      if (x != x || 4 * (tid + i * SM_THREADS) + e >= V) x = ninf;
      if (x == 0.f) x = 0.f;  // -0 -> +0: the key order needs it
      smax = fmaxf(smax, x);
      s[i][e] = x;
    }
  const float m = sm_unkey(sm_block_umax(sm_key(smax), red, ph));
  if (!(fabsf(m) < INFINITY)) {  // all -inf, or a +inf: no candidate
    if (tid < W) {
      oc[tid] = ninf;
      ov[tid] = 0;
    }
    return;
  }

  // ---- Z in the fixed order, then every register becomes its candidate ----
  float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NG; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += expf(s[i][e] - m);  // exp(-inf) = 0
    __builtin_amdgcn_sched_barrier(0);
  }
  const float Z = sm_block_mass((a[0] + a[1]) + (a[2] + a[3]), red, ph);  // >= 1: the maximum's term
  const float lz = logf(Z);
  if (tid == 0) {  // for the merge: a pick's own term (s - m) - log Z, from the same two numbers
    ws_ml[2 * row] = m;
    ws_ml[2 * row + 1] = lz;
  }
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) s[i][e] = score + ((s[i][e] - m) - lz);

  // ---- W rounds: the best (c, lowest id) strictly behind the last pick ----
  float pc = INFINITY;
  int pv = -1;
#pragma unroll 1
  for (int j = 0; j < W; ++j) {
    float bs = ninf;
    int bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < NG; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float c = s[i][e];
        const int v = 4 * (tid + i * SM_THREADS) + e;
        const bool behind = c < pc || (c == pc && v > pv);
        if (behind && (c > bs || (c == bs && v < bi))) { bs = c; bi = v; }
      }
    sm_wave_argmax(bs, bi);
    if ((tid & 63) == 0) { best_s_w[ph][tid >> 6] = bs; best_i_w[ph][tid >> 6] = bi; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SM_WAVES; ++k) {  // every thread: the same 16 pairs in the same order
      const float os = best_s_w[ph][k];
      const int oi = best_i_w[ph][k];
      if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    ph ^= 1;
    // c = -inf (an id >= V, a -inf or NaN logit) and a NaN c are no candidates: neither beats bs = -inf
    const bool got = bs > ninf && bi < V;
    if (tid == 0) {
      oc[j] = got ? bs : ninf;
      ov[j] = got ? bi : 0;
    }
    if (!got) {  // uniform: nothing is left for the later rounds either
      if (tid > j && tid < W) {
        oc[tid] = ninf;
        ov[tid] = 0;
      }
      return;
    }
    pc = bs;
    pv = bi;
  }
}

// one wave per b; lane l < W W holds pair l % W of row l / W
// logp (may be null): the log-probability term (s - m) - log Z of a live pick, recomputed from its
// logit with the row's m and log Z - the bits that went into its candidate; 0 for a finished beam's
// candidate and for an empty slot
__global__ void __launch_bounds__(256) beam_merge_kernel(const float* __restrict__ ws_c, const int* __restrict__ ws_v,
                                                         const float* __restrict__ ws_ml,
                                                         const uint8_t* __restrict__ finished, int64_t B, int V,
                                                         int W, int eos_id, int fill, const void* __restrict__ logits,
                                                         bool bf16, int64_t stride_b, int64_t stride_w,
                                                         float* __restrict__ new_scores, int* __restrict__ parent,
                                                         int64_t* __restrict__ token, uint8_t* __restrict__ new_finished,
                                                         float* __restrict__ logp) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform
  const float ninf = -INFINITY;
  float c = ninf;
  int key = INT_MAX;  // (w, pair index): rows in beam order, a row's pairs already in (c, id) order
  int v = 0;
  if (lane < W * W) {
    c = ws_c[b * W * W + lane];
    v = ws_v[b * W * W + lane];
    if (c > ninf) key = lane; else c = ninf;
  }
  for (int j = 0; j < W; ++j) {
    float bs = c;
    int bi = key;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(bs, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    const bool got = bs > ninf && bi < W * W;
    const int src = got ? bi : 0;
    const int tv = __shfl(v, src, 64);
    if (lane == 0) {
      const int p = got ? src / W : 0;
      int t = got ? tv : fill;
      const bool pfin = got && finished[b * W + p];
      if (!pfin && got) t = min(max(t, 0), V - 1);  // a live pick is an id of the row
      new_scores[b * W + j] = got ? bs : ninf;
      parent[b * W + j] = p;
      token[b * W + j] = (int64_t)t;
      new_finished[b * W + j] = (got && (pfin || (eos_id >= 0 && t == eos_id))) ? 1 : 0;
      if (logp) {
        float lp = 0.f;
        if (got && !pfin) {  // t is an id of the live row p, whose m and log Z were written
          const int64_t at = b * stride_b + (int64_t)p * stride_w + t;
          const float x = bf16 ? __uint_as_float((uint32_t)((const bf16_t*)logits)[at] << 16) : ((const float*)logits)[at];
          lp = ((x == 0.f ? 0.f : x) - ws_ml[2 * (b * W + p)]) - ws_ml[2 * (b * W + p) + 1];
        }
        logp[b * W + j] = lp;
      }
    }
    if (got && lane == src) { c = ninf; key = INT_MAX; }  // taken
  }
}

template <int NG>
static void bs_launch(bool bf16, const void* logits, int64_t sb, int64_t sw, int64_t B, int V, int W,
                      const float* scores, const uint8_t* finished, int fill, float* ws_c, int* ws_v, float* ws_ml,
                      hipStream_t st) {
  const dim3 grid((unsigned)(B * W)), block(SM_THREADS);
  if (bf16)
    hipLaunchKernelGGL((beam_rows_kernel<NG, true>), grid, block, 0, st, logits, sb, sw, V, W, scores, finished, fill,
                       ws_c, ws_v, ws_ml);
  else
    hipLaunchKernelGGL((beam_rows_kernel<NG, false>), grid, block, 0, st, logits, sb, sw, V, W, scores, finished, fill,
                       ws_c, ws_v, ws_ml);
}

bool launch_beam_step(const void* logits, bool bf16, int64_t stride_b, int64_t stride_w, int64_t B, int W, int V,
                      const float* scores, const uint8_t* finished, int eos_id, int fill, float* ws_c, int* ws_v,
                      float* new_scores, int* parent, int64_t* token, uint8_t* new_finished, float* logp,
                      hipStream_t st) {
  if (!logits || !scores || !finished || !ws_c || !ws_v || !new_scores || !parent || !token || !new_finished)
    return false;
  if (B < 1 || W < 1 || W > BS_MAX_W || V < 1 || V > 65536 || B * W > 0x7fffffffLL || stride_b < 0 || stride_w < 0)
    return false;
  const int ng = ((V + 3) / 4 + SM_THREADS - 1) / SM_THREADS;  // 1 .. 16
  float* ws_ml = ws_c + B * W * W;  // (m, log Z) per row, behind the pairs
#define BS_CASE(N) bs_launch<N>(bf16, logits, stride_b, stride_w, B, V, W, scores, finished, fill, ws_c, ws_v, ws_ml, st)
  if (ng <= 1) BS_CASE(1);
  else if (ng <= 2) BS_CASE(2);
  else if (ng <= 4) BS_CASE(4);
  else if (ng <= 8) BS_CASE(8);
  else if (ng <= 13) BS_CASE(13);  // V = 50257 (GPT-2)
  else BS_CASE(16);
#undef BS_CASE
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, ws_c, ws_v, ws_ml, finished, B,
                     V, W, eos_id, fill, logits, bf16, stride_b, stride_w, new_scores, parent, token, new_finished,
                     logp);
  return true;
}

}  // namespace dpa
