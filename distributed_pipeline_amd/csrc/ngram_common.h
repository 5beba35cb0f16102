// What the n-gram kernels (ngram_match.hip, ngram_distinct.hip) share: the limits, the LDS row
// layout with its two sentinels, the wave sum and the broadcast walk over one staged row.
//
// A group's ids are staged in LDS as 32-bit values, one row of L + NG_PAD entries per sequence, with
// every position at or beyond its length replaced by NG_NONE_Q; the n-gram a lane holds in registers
// carries NG_NONE_P there instead, so gram_n(p) exists exactly when none of its n tokens is a
// sentinel and two sentinels never compare equal.
#pragma once
#include "common.h"

namespace dpa {

constexpr int NG_MAX_K = 16;
constexpr int NG_MAX_L = 256;
constexpr int NG_PAD = 4;          // sentinels after each LDS row: p + 3 and q + 4 stay inside it
constexpr int NG_NONE_P = -1;      // sentinel of the p side (registers)
constexpr int NG_NONE_Q = -2;      // sentinel of the q side (LDS); ids inside the lengths are >= 0

__device__ __forceinline__ int ng_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// cnt[n-1] += 1 for every q in [0, q_end) (and q < p when BELOW) whose n-gram in `row` equals the
// n-gram a[0..n-1]; q_end <= L, row holds L + NG_PAD entries.  q_end is wave-uniform.
template <bool BELOW>
__device__ __forceinline__ void ng_walk(const int* row, int q_end, int p, const int a[4], int cnt[4]) {
  int b0 = row[0], b1 = row[1], b2 = row[2], b3 = row[3];
  for (int q = 0; q < q_end; ++q) {
    const bool e0 = (a[0] == b0) && (!BELOW || q < p);
    const bool e1 = e0 && (a[1] == b1);
    const bool e2 = e1 && (a[2] == b2);
    const bool e3 = e2 && (a[3] == b3);
    cnt[0] += e0;
    cnt[1] += e1;
    cnt[2] += e2;
    cnt[3] += e3;
    b0 = b1;
    b1 = b2;
    b2 = b3;
    b3 = row[q + 4];  // q + 4 <= L + 3
  }
}

}  // namespace dpa
