// Length of the longest common subsequence (LCS) of every pair of the K short token sequences of a
// group (ROUGE-L of run.eval, ROUGE-L minimum-Bayes-risk selection among decoded candidates):
//
//   out[g][i][j] = LCS(tokens[g][i][0 .. len[g][i]), tokens[g][j][0 .. len[g][j]))
//
// Whatever lies at or beyond a length never matches.  Bit-parallel recurrence (Allison-Dix / Hyyro):
// one bit per position of sequence A, one step per token y of sequence B,
//
//   V = all ones;   per y:  M = {p < len_a : A[p] == y},  U = V & M,  V = (V + U) | (V & ~M)
//
// and the LCS is the number of zero bits of V.  Bits at or beyond len_a stay 1 because M is 0 there.
//
// One wave owns one unordered pair (i <= j); the pairs of all groups are spread flat over the waves
// of the grid, so a K = 2 call (run.eval) fills its blocks as a K = 10 call (MBR) does.  Lane l holds
// A[l + 64 c] and B[l + 64 c], c = 0..3 (L <= 256), loaded straight from global memory with a
// sentinel beyond the length.  The words of M are the ballots of (a[c] == y), y is a readlane of
// the B registers at a wave-uniform index, so M, U and V are wave-uniform and the whole update runs
// in the scalar ALU: no LDS, no barriers, no atomics; integers only, bitwise reproducible.  Every
// branch is wave-uniform (all 64 lanes are active at every ballot and readlane).  V has as many
// 64-bit words as A has chunks inside its length; of the two sequences, A is the one that makes
// (steps x words) smaller.  Lane 0 writes out[g][i][j] and out[g][j][i]; the diagonal is len.
#include "common.h"
#include "launchers.h"

namespace dpa {

constexpr int LCS_MAX_K = 16;
constexpr int LCS_MAX_L = 256;
constexpr int LCS_WAVES = 4;       // waves (pairs) per block
constexpr int LCS_NONE_A = -1;     // beyond the length of A; ids inside the lengths are >= 0
constexpr int LCS_NONE_B = -2;     // beyond the length of B (never stepped over)

// Number of zero bits of V after stepping over the first nb tokens of b; W = words of V = chunks of
// a that hold a position inside its length.  nb is wave-uniform.
template <int W>
__device__ __forceinline__ int lcs_zero_bits(const int (&a)[4], const int (&b)[4], int nb) {
  // V as 2 W 32-bit words: the add is one scalar add-with-carry chain
  uint32_t V[2 * W];
#pragma unroll
  for (int w = 0; w < 2 * W; ++w) V[w] = ~0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int n = min(nb - 64 * c, 64);
    for (int q = 0; q < n; ++q) {
      const int y = __builtin_amdgcn_readlane(b[c], q);
      uint32_t M[2 * W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const uint64_t m = __ballot(a[w] == y);
        M[2 * w] = (uint32_t)m;
        M[2 * w + 1] = (uint32_t)(m >> 32);
      }
      uint32_t carry = 0;
#pragma unroll
      for (int w = 0; w < 2 * W; ++w) {
        const uint32_t s = __builtin_addc(V[w], V[w] & M[w], carry, &carry);
        V[w] = s | (V[w] & ~M[w]);
      }
    }
  }
  int z = 0;
#pragma unroll
  for (int w = 0; w < 2 * W; ++w) z += __popc(~V[w]);
  return z;
}

template <typename T>
__global__ void __launch_bounds__(64 * LCS_WAVES) lcs_kernel(const T* __restrict__ tokens,
                                                             const int* __restrict__ lens, int64_t tasks,
                                                             int K, int L, int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t task = (int64_t)blockIdx.x * LCS_WAVES + wid;
  if (task >= tasks) return;  // the whole wave
  const int npair = K * (K + 1) / 2;
  const int64_t g = task / npair;
  int rest = (int)(task - g * npair), i = 0;
  while (rest >= K - i) {
    rest -= K - i;
    ++i;
  }
  const int j = i + rest;
  const int64_t ri = g * K + i, rj = g * K + j;  // rows of tokens / lens
  const int ni = min(max(lens[ri], 0), L), nj = min(max(lens[rj], 0), L);
  int* og = out + g * K * K;
  if (i == j) {
    if (lane == 0) og[i * K + i] = ni;
    return;
  }
  // A: the sequence with the cheaper (steps of the other) x (own words)
  const bool swap = (int64_t)ni * ((nj + 63) >> 6) < (int64_t)nj * ((ni + 63) >> 6);
  const int na = swap ? nj : ni, nb = swap ? ni : nj;
  const T* ta = tokens + (swap ? rj : ri) * L;
  const T* tb = tokens + (swap ? ri : rj) * L;
  int a[4], b[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int p = lane + 64 * c;
    a[c] = p < na ? (int)ta[p] : LCS_NONE_A;  // na, nb <= L: the loads stay inside the rows
    b[c] = p < nb ? (int)tb[p] : LCS_NONE_B;
  }
  int z;
  if (na <= 64)
    z = lcs_zero_bits<1>(a, b, nb);
  else if (na <= 128)
    z = lcs_zero_bits<2>(a, b, nb);
  else if (na <= 192)
    z = lcs_zero_bits<3>(a, b, nb);
  else
    z = lcs_zero_bits<4>(a, b, nb);
  if (lane == 0) {
    og[i * K + j] = z;
    og[j * K + i] = z;
  }
}

bool launch_lcs_lengths(const void* tokens, bool tok64, const int* lens, int64_t G, int K, int L, int* out,
                        hipStream_t st) {
  if (tokens == nullptr || lens == nullptr || out == nullptr) return false;
  if (G <= 0 || K < 1 || K > LCS_MAX_K || L < 1 || L > LCS_MAX_L) return false;
  if (G > 0x7fffffffLL / (LCS_MAX_K * (LCS_MAX_K + 1) / 2)) return false;  // the grid stays below 2^31 blocks
  const int64_t tasks = G * (K * (K + 1) / 2);
  const dim3 grid((unsigned)((tasks + LCS_WAVES - 1) / LCS_WAVES)), block(64 * LCS_WAVES);
  if (tok64)
    hipLaunchKernelGGL(lcs_kernel<int64_t>, grid, block, 0, st, (const int64_t*)tokens, lens, tasks, K, L, out);
  else
    hipLaunchKernelGGL(lcs_kernel<int32_t>, grid, block, 0, st, (const int32_t*)tokens, lens, tasks, K, L, out);
  return true;
}

}  // namespace dpa
