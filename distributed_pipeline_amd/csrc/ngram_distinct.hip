// Distinct n-gram counts of the K short token sequences of a group, per sequence and over the
// group's union (dist-n / div-n of run.eval, utils/diversity.py):
//
//   d[g][k][n-1], k < K : number of distinct n-grams among the first len[g][k] tokens of sequence k
//   d[g][K][n-1]        : number of distinct n-grams in the union of the group's K sequences
//   n = 1..4; int32 [G][K + 1][4], one 16-byte row per sequence plus one for the union
//
// Whatever lies at or beyond the length never counts and an n-gram that would cross it does not
// exist (the conventions of ngram_match.hip; lengths clamped to [0, L] here).
//
// First-occurrence form, integers only (no hashing, no global atomics, bitwise reproducible).
// Position p of sequence k holds a new n-gram for the sequence when gram_n(k, p) exists and no
// q < p of the same sequence holds the same n-gram; it holds a new n-gram for the union when, in
// addition, no position of any sequence k' < k holds it.  d[g][k] counts the first kind over p,
// d[g][K] the second kind over (k, p).  The two sentinels (ngram_common.h) make a non-existent
// n-gram equal to nothing, so its "seen before" counts are 0: existence, p + n <= len, is masked
// explicitly.
//
// One workgroup per group g.  The ids are staged in LDS with sentinels (ngram_common.h).  A wave
// owns a task (sequence k, 64 consecutive positions p): its lanes hold their n-gram's 4 tokens in
// registers and walk together their own row below p, then every earlier row in full, so every LDS
// read is a broadcast and one walk serves the four orders.  Tasks are handed out from the last
// sequence (the longest walk) to the first.  The two 4-vectors are wave-reduced; the per-sequence
// sums of a workgroup's tasks meet in LDS (integer adds: any order gives the same sums), the union
// sums stay in the wave's registers until its tasks are done.  One int4 store per output row.
// The block has as many waves as there are tasks, K * ceil(L / 64), from 1 to 4: a K = 1 call (the
// dist-n of thousands of single sequences) runs one wave per group.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), int32 / int64
// ids alike: 33 VGPRs, 76 SGPRs, no scratch, occupancy 8 waves/SIMD, no static LDS; dynamic LDS
// (K + 1) * 16 + 64 + K * (L + 4) * 4 bytes, 16 976 (16.6 KiB) at K = 16, L = 256.
#include "common.h"
#include "launchers.h"
#include "ngram_common.h"

namespace dpa {

constexpr int ND_MAX_WAVES = 4;

template <typename T>
__global__ void __launch_bounds__(64 * ND_MAX_WAVES) ngram_distinct_kernel(const T* __restrict__ tokens,
                                                                           const int* __restrict__ lens,
                                                                           int K, int L, int* __restrict__ d) {
  extern __shared__ __attribute__((aligned(16))) char nd_smem[];
  const int LS = L + NG_PAD;
  int* acc = reinterpret_cast<int*>(nd_smem);  // [K + 1][4]: the output rows of the group
  int* len = acc + (K + 1) * 4;                // [NG_MAX_K]
  int* tok = len + NG_MAX_K;                   // [K][LS]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
  const int64_t g = blockIdx.x;
  const T* tg = tokens + g * K * L;

  if (tid < K) len[tid] = min(max(lens[g * K + tid], 0), L);
  for (int e = tid; e < (K + 1) * 4; e += blockDim.x) acc[e] = 0;
  __syncthreads();
  for (int e = tid; e < K * LS; e += blockDim.x) {
    const int k = e / LS, p = e - k * LS;
    tok[e] = p < len[k] ? (int)tg[k * L + p] : NG_NONE_Q;  // len <= L: the loads stay inside the rows
  }
  __syncthreads();

  const int nchunk = (L + 63) >> 6;
  int uni[4] = {0, 0, 0, 0};
  for (int t = wid; t < K * nchunk; t += nw) {
    const int k = K - 1 - t / nchunk, p0 = (t % nchunk) * 64, p = p0 + lane;
    const int n = len[k];
    if (p0 >= n) continue;  // the whole chunk lies beyond the length (wave-uniform)
    const int* row = tok + k * LS;
    int a[4], own[4] = {0, 0, 0, 0}, earlier[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = p + c < n ? row[p + c] : NG_NONE_P;
    ng_walk<true>(row, min(n, p0 + 64), p, a, own);
    for (int j = 0; j < k; ++j) ng_walk<false>(tok + j * LS, len[j], p, a, earlier);
    int seq[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool fresh = p + c < n && own[c] == 0;  // gram_{c+1}(k, p) exists and is the first in k
      seq[c] = ng_wave_sum((int)fresh);
      uni[c] += ng_wave_sum((int)(fresh && earlier[c] == 0));
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) atomicAdd(&acc[k * 4 + c], seq[c]);  // LDS
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) atomicAdd(&acc[K * 4 + c], uni[c]);  // LDS
  }
  __syncthreads();
  if (tid <= K)  // K + 1 <= 17 rows, at least 64 threads
    reinterpret_cast<int4*>(d + g * (K + 1) * 4)[tid] = reinterpret_cast<const int4*>(acc)[tid];
}

bool launch_ngram_distinct(const void* tokens, bool tok64, const int* lens, int64_t G, int K, int L, int* d,
                           hipStream_t st) {
  if (tokens == nullptr || lens == nullptr || d == nullptr) return false;
  if (G <= 0 || G > 0x7fffffffLL || K < 1 || K > NG_MAX_K || L < 1 || L > NG_MAX_L) return false;
  const int tasks = K * ((L + 63) / 64);
  const dim3 grid((unsigned)G), block(64 * (tasks < ND_MAX_WAVES ? tasks : ND_MAX_WAVES));
  const size_t lds = ((size_t)(K + 1) * 4 + NG_MAX_K + (size_t)K * (L + NG_PAD)) * sizeof(int);  // <= 16.6 KiB
  if (tok64)
    hipLaunchKernelGGL(ngram_distinct_kernel<int64_t>, grid, block, lds, st, (const int64_t*)tokens, lens, K, L,
                       d);
  else
    hipLaunchKernelGGL(ngram_distinct_kernel<int32_t>, grid, block, lds, st, (const int32_t*)tokens, lens, K, L,
                       d);
  return true;
}

}  // namespace dpa
