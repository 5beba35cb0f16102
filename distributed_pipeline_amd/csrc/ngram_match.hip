// Clipped n-gram match counts between every pair of the K short token sequences of a group
// (minimum-Bayes-risk selection among decoded candidates, BLEU / self-BLEU of run.eval):
//
//   m[g][i][j][n-1] = sum over the distinct n-grams y of min(count_i(y), count_j(y)),   n = 1..4
//
// count_k counts the occurrences of y among the first len[g][k] tokens of sequence k; whatever
// lies at or beyond the length never counts and an n-gram that would cross it does not exist.
//
// Rank/count form, integers only (no hashing, no atomics, bitwise reproducible).  For a position
// p of sequence i let r_n(p) = #{q < p : gram_n(i, q) == gram_n(i, p)} (its occurrence rank in i)
// and c_n(p) = #{q : gram_n(j, q) == gram_n(i, p)}.  The occurrences of one n-gram in i carry the
// ranks 0 .. count_i - 1 and those below count_j are the clipped matches, so
// m_n = #{p : c_n(p) > r_n(p)}.
//
// One workgroup per group g.  The ids are staged in LDS as 32-bit values with every position at
// or beyond its length replaced by a sentinel, each row padded by 4 sentinels, so gram_n(p)
// exists exactly when none of its n tokens is a sentinel; the "p side" of a comparison uses
// another sentinel than the "q side", so two sentinels never compare equal.  A wave owns one
// sequence (ranks) or one unordered pair (matches); its lanes own 64 consecutive positions p and
// walk q together, so every LDS read of the q side is a broadcast, and one walk serves the four
// orders: the n-gram at (p, q) matches when the first n tokens do.  The ranks (< L <= 256) are
// kept as 4 bytes of one LDS dword per position.  Wave-reduce, then lane 0 writes m[g][i][j][:]
// and m[g][j][i][:] as one 16-byte store each; the diagonal is max(len - n + 1, 0).
#include "common.h"
#include "launchers.h"
#include "ngram_common.h"

namespace dpa {

template <typename T>
__global__ void __launch_bounds__(256) ngram_match_kernel(const T* __restrict__ tokens,
                                                          const int* __restrict__ lens, int K, int L,
                                                          int* __restrict__ m) {
  extern __shared__ __attribute__((aligned(16))) char ng_smem[];
  const int LS = L + NG_PAD;
  int* tok = reinterpret_cast<int*>(ng_smem);              // [K][LS]
  uint32_t* rank = reinterpret_cast<uint32_t*>(tok + K * LS);  // [K][L]: the 4 ranks, one byte each
  int* len = reinterpret_cast<int*>(rank + K * L);         // [K]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
  const int64_t g = blockIdx.x;
  const T* tg = tokens + g * K * L;
  int* mg = m + g * K * K * 4;

  if (tid < K) {
    const int n = min(max(lens[g * K + tid], 0), L);
    len[tid] = n;
    int4 d;
    d.x = n;
    d.y = max(n - 1, 0);
    d.z = max(n - 2, 0);
    d.w = max(n - 3, 0);
    *reinterpret_cast<int4*>(mg + (tid * K + tid) * 4) = d;
  }
  __syncthreads();
  for (int e = tid; e < K * LS; e += blockDim.x) {
    const int k = e / LS, p = e - k * LS;
    tok[e] = p < len[k] ? (int)tg[k * L + p] : NG_NONE_Q;
  }
  __syncthreads();

  const int nchunk = (L + 63) >> 6;
  // ranks: one (sequence, 64 positions) task per wave
  for (int t = wid; t < K * nchunk; t += nw) {
    const int k = t / nchunk, p = (t - k * nchunk) * 64 + lane;
    const int n = len[k];
    const int* row = tok + k * LS;
    if (p - lane >= n) continue;  // the whole chunk lies beyond the length (wave-uniform)
    int a[4], cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = p + c < n ? row[p + c] : NG_NONE_P;
    ng_walk<true>(row, min(n, p - lane + 64), p, a, cnt);
    if (p < n) rank[k * L + p] = (uint32_t)cnt[0] | (uint32_t)cnt[1] << 8 | (uint32_t)cnt[2] << 16 | (uint32_t)cnt[3] << 24;
  }
  __syncthreads();

  // matches: one unordered pair i < j per wave
  const int npair = K * (K - 1) / 2;
  for (int t = wid; t < npair; t += nw) {
    int i = 0, rest = t;
    while (rest >= K - 1 - i) {
      rest -= K - 1 - i;
      ++i;
    }
    const int j = i + 1 + rest;
    const int ni = len[i], nj = len[j];
    const int* row_i = tok + i * LS;
    const int* row_j = tok + j * LS;
    int tot[4] = {0, 0, 0, 0};
    for (int p0 = 0; p0 < ni; p0 += 64) {
      const int p = p0 + lane;
      int a[4], cnt[4] = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = p + c < ni ? row_i[p + c] : NG_NONE_P;
      ng_walk<false>(row_j, nj, p, a, cnt);
      const uint32_t r = p < ni ? rank[i * L + p] : 0u;
#pragma unroll
      for (int c = 0; c < 4; ++c) tot[c] += cnt[c] > (int)((r >> (8 * c)) & 0xffu);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) tot[c] = ng_wave_sum(tot[c]);
    if (lane == 0) {
      int4 d;
      d.x = tot[0];
      d.y = tot[1];
      d.z = tot[2];
      d.w = tot[3];
      *reinterpret_cast<int4*>(mg + (i * K + j) * 4) = d;
      *reinterpret_cast<int4*>(mg + (j * K + i) * 4) = d;
    }
  }
}

bool launch_ngram_match(const void* tokens, bool tok64, const int* lens, int64_t G, int K, int L, int* m,
                        hipStream_t st) {
  if (tokens == nullptr || lens == nullptr || m == nullptr) return false;
  if (G <= 0 || G > 0x7fffffffLL || K < 1 || K > NG_MAX_K || L < 1 || L > NG_MAX_L) return false;
  const size_t lds = ((size_t)K * (L + NG_PAD) + (size_t)K * L + NG_MAX_K) * sizeof(int);  // <= 33 KiB
  if (tok64)
    hipLaunchKernelGGL(ngram_match_kernel<int64_t>, dim3((unsigned)G), dim3(256), lds, st,
                       (const int64_t*)tokens, lens, K, L, m);
  else
    hipLaunchKernelGGL(ngram_match_kernel<int32_t>, dim3((unsigned)G), dim3(256), lds, st,
                       (const int32_t*)tokens, lens, K, L, m);
  return true;
}

}  // namespace dpa
