// K-M29: the Linears of a GPT-2 decode step on one-byte weights (W8A16) - a few bf16 rows against a
// whole matrix of e4m3fn codes.
//
//   x    [M][K] bf16    1 <= M <= 128 rows, ldx elements apart (ldx % 8 == 0, 16-byte aligned base)
//   W8   [N][K] uint8   OCP e4m3fn codes, row-major, rows ldw bytes apart (ldw >= K, ldw % 16 == 0,
//                       16-byte aligned base): a row slice of a larger matrix works
//   we   [N]    int8    one power-of-two exponent per weight row, the format of kv_quantize
//   bias [N]    bf16    or null
//   y    [M][N] bf16    y[m][n] = bf16(act(ldexp(sum_k x[m][k] float(W8[n][k]), we[n]) + bias[n]))
//
// Products and sums are fp32 (MFMA accumulators); the exponent is applied once per output, to the
// finished fp32 sum, as an exact v_ldexp_f32; the bias is added and act (the codes of act.h) applied
// in fp32; one rounding, to bf16.  K % 64 == 0; any N >= 1.
//
// The problem is K-M26's (linear_rows.hip) with half the bytes: the step is a stream of W from HBM,
// and every e4m3fn value is exactly a bf16 value, so the codes become the A operand of
// v_mfma_f32_32x32x16_bf16 without any rounding while x stays bf16 as the B operand.  y^T = W x^T,
// 32 weight rows per MFMA, MB = ceil(M / 32) accumulators of 16 registers.
//
// Work split.  A workgroup of 4 waves owns 32 weight rows (grid = ceil(N / 32)) and all of K.  A
// 16-byte load now carries 16 k, so K is cut into chunks of 512: inside chunk c wave w owns the 128
// codes c 512 + w 128 .. + 127 - one 128-byte line of every weight row - and lane half h the 64
// contiguous bytes h 64 .. h 64 + 63 of it, which it fetches with four 16-byte loads issued back to
// back.  The two halves together consume the whole line: no line is fetched for a fragment of it.
// K is never split across workgroups: one launch, no workspace, no second pass.
//
// k order.  A wave's piece of a chunk takes eight MFMA steps s = 0 .. 7; load q = s >> 1 of the lane
// holds the codes of steps 2 q and 2 q + 1 (its low and high 8 bytes), so in step s
//
//     lane (r, h), element j   <->   k = c 512 + w 128 + h 64 + s 8 + j
//
// for A and B alike.  K % 64 == 0, so a lane half's 64 bytes lie inside K or outside: a half outside
// holds zero codes (it reads its row's first bytes instead), a wave wholly outside skips the chunk.
//
// Conversion, in registers between load and MFMA.  v_cvt_pk_f32_fp8 turns two codes into two fp32
// (subnormal codes included, exactly) and one v_perm_b32 keeps the two high halves as a bf16 pair -
// exact, an e4m3fn value has four significant bits.  16 VALU operations per 16-byte load, 64 per
// wave and chunk, against 8 MB MFMAs of 8 passes: a quarter of the VALU's rate at the HBM's.  The
// route by shift (magnitude bits four places up, 2^120 folded into the epilogue) is not taken: it
// relies on the MFMA honouring bf16 subnormals, which has not been measured here.
//
// Latency.  A register set is four raw loads (16 VGPRs, 4 KB per wave - as many bytes as a set of
// K-M26, twice the k).  A ring of three: while the wave converts and computes on chunk c the sets
// of chunks c + 1 and c + 2 are in flight, 8 KB per wave and 32 KB per workgroup.  Every load is
// unconditional and from inside W8 (a lane without a row reads row N - 1 and keeps zero codes), so
// the compiler counts them in flight exactly.  W never sees LDS.
//
// B operand.  x is staged through 64 KB of LDS with swz in units of half a chunk: unit (c, f) holds,
// for every (w, h), the 32 k of steps 4 f .. 4 f + 3 - 512 bytes per row, the 16-byte piece of
// (w, h, s & 3) at column (2 w + h) 4 + (s & 3).  MB 32 rows of 4 / MB units are staged together
// (two chunks, one chunk, half a chunk), read back as ds_read_b128 fragments of 32 consecutive rows
// at one column, which swz keeps conflict-free.  Rows m >= M and columns k >= K are written as zeros;
// their threads read row M - 1 and column 0 again, never anything beyond x.  How many units are
// staged together depends on MB; the order in which an accumulator receives its MFMAs does not:
// chunk by chunk, step by step.  Known weakness: at MB = 4 the second unit of a chunk is staged
// behind the chunk's weight loads, so waiting for x there also waits for the ring.
//
// The row contract, as K-M26 states it.  Column m of an MFMA result depends on column m of B alone,
// each wave folds its pieces in chunk and step order, and the four partial accumulators are added
// through LDS in wave order, ((p0 + p1) + p2) + p3, by one writer per element; ldexp, bias and act
// act on that one value.  So the bits of y[m][n] are a function of x[m][:], W8[n][:], we[n],
// bias[n], act, K and N - not of M, of the row's place in the call, of the other rows or of the
// grid.  No atomics.
//
// Epilogue.  K-M26's: partials to LDS in register layout, wave w sums registers 4 w .. 4 w + 3 of
// every block, scales by 2^we[n], adds the bias, applies act (GELU through erfc: l8_act) and rounds;
// the bf16 tile is transposed through LDS ([m][34]) so that the stores run along n.  Rows m >= M and
// columns n >= N are not stored; we and bias are read at n < N only.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), MB = 1 / 2 / 4:
// 182 / 174 / 156 VGPRs + 16 / 32 / 64 AGPRs (the accumulators), 63 / 62 / 64 SGPRs, 65536 bytes of LDS,
// scratch 0: two workgroups per compute unit, by LDS (MB = 4 stages x in two batches to stay there).
#include "act.h"
#include "common.h"
#include "launchers.h"
#include "mfma.h"

namespace dpa {

constexpr int L8_WAVES = 4;
constexpr int L8_ROWS = 32;    // weight rows per workgroup: one MFMA row block
constexpr int L8_KC = 512;     // k per chunk: 128 per wave (a line of the row), 64 per lane half
constexpr int L8_KU = 256;     // k per staged unit of x: half a chunk, 32 per (wave, lane half)
constexpr int L8_RING = 3;     // register sets of raw codes: one in use, two in flight
constexpr int L8_LDS = 65536;
constexpr int L8_TILE_LD = 34;  // bf16 elements per row of the transposed tile: 17 dwords, odd

// Four codes of `word` -> two bf16 pairs (elements 0, 1 and 2, 3): the high halves of the exact fp32.
__device__ __forceinline__ uint32_t l8_pair(uint32_t word, bool hi) {
  const f32x2 v = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)word, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)word, false);
  return __builtin_amdgcn_perm(__float_as_uint(v[1]), __float_as_uint(v[0]), 0x07060302u);
}

// act of act.h's codes.  GELU is z / 2 erfc(-z / sqrt 2) here, not act.h's gelu_f: that one's absolute error of
// 1.5e-7 |z| is a relative one of tens of percent where z < -4, and an output is held to its own column's scale.
__device__ __forceinline__ float l8_act(float z, int act) {
  return act == 1 ? 0.5f * z * erfcf(-0.70710678118654752f * z) : act_apply(z, act);
}

// Eight codes (two dwords) -> one A fragment.
__device__ __forceinline__ bf16x8 l8_frag(uint32_t a, uint32_t b) {
  const u32x4 p = {l8_pair(a, false), l8_pair(a, true), l8_pair(b, false), l8_pair(b, true)};
  return __builtin_bit_cast(bf16x8, p);
}

template <int MB>
__global__ void __launch_bounds__(64 * L8_WAVES) linear_rows_fp8_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const uint8_t* __restrict__ W8, int64_t ldw,
    const int8_t* __restrict__ we, const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int64_t ldy, int M,
    int N, int K, int act) {
  constexpr int G = 4 / MB;               // units staged together
  constexpr int ROWB = L8_KU * 2 * G;     // bytes of a staged row of x
  constexpr int CPR = ROWB / 16;          // its 16-byte pieces
  constexpr int NT = 64 * L8_WAVES;
  constexpr int PIECES = MB * 32 * CPR / NT;  // per thread and stage: 16
  static_assert(MB * 32 * ROWB == L8_LDS, "a stage fills the LDS buffer");
  static_assert(L8_WAVES * MB * 16 * 64 * 4 <= L8_LDS && MB * 32 * L8_TILE_LD * 2 <= L8_LDS, "epilogue fits");
  __shared__ __attribute__((aligned(16))) char lds[L8_LDS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * L8_ROWS;
  const bool row_ok = n0 + r < N;
  const int NC = (K + L8_KC - 1) / L8_KC;
  const uint8_t* wrow = W8 + (int64_t)min(n0 + r, N - 1) * ldw;

  // The lane's four raw loads of chunk c: 64 contiguous bytes of its weight row.  Unconditional, from an
  // address inside W8; a lane without a row or a half beyond K (the tail chunk, or the ring running past
  // the end) keeps zero codes, which are +0.
  auto loadw = [&](int c, uint4 f[4]) {
    const int k = c * L8_KC + wave * 128 + h * 64;  // K % 64 == 0: the half is inside or outside
    const bool ok = row_ok && k < K;
    const uint8_t* p = wrow + (k < K ? k : 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 g = *reinterpret_cast<const uint4*>(p + q * 16);
      f[q] = ok ? g : make_uint4(0u, 0u, 0u, 0u);
    }
  };

  // units st G .. st G + G - 1 of x into LDS; rows >= M and columns >= K as zeros.  MB = 4 moves its 16 pieces
  // in two batches of 8, which keeps the kernel at two workgroups per compute unit (256 registers).
  auto stage = [&](int st) {
    constexpr int BATCH = MB == 4 ? PIECES / 2 : PIECES;
#pragma unroll
    for (int i0 = 0; i0 < PIECES; i0 += BATCH) {
      uint4 v[BATCH];
#pragma unroll
      for (int i = 0; i < BATCH; ++i) {
        const int p = tid + NT * (i0 + i), row = p / CPR, ch = p % CPR;
        const int ui = st * G + (ch >> 5), wh = (ch & 31) >> 2, sq = ch & 3;
        const int k = (ui >> 1) * L8_KC + wh * 64 + (ui & 1) * 32 + sq * 8;
        // unconditional, from an address inside x; what lies outside becomes zeros
        const uint4 g = *reinterpret_cast<const uint4*>(x + (int64_t)min(row, M - 1) * ldx + (k < K ? k : 0));
        v[i] = (row < M && k < K) ? g : make_uint4(0u, 0u, 0u, 0u);
      }
      if (i0 == 0) __syncthreads();  // every wave is done with the previous stage
#pragma unroll
      for (int i = 0; i < BATCH; ++i) {
        const int p = tid + NT * (i0 + i), row = p / CPR, ch = p % CPR;
        *reinterpret_cast<uint4*>(lds + swz<ROWB>(row, ch)) = v[i];
      }
    }
    __syncthreads();
  };

  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = zero16();

  // steps 4 f .. 4 f + 3 of chunk c: loads 2 f and 2 f + 1 of the set, against unit 2 c + f of x
  auto compute = [&](int c, int f, const uint4 w[4]) {
    if (c * L8_KC + wave * 128 >= K) return;  // wave-uniform: the tail chunk has no piece for this wave
    const int ch0 = ((2 * c + f) % G) * 32 + (wave * 2 + h) * 4;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const uint4 g = w[2 * f + q];
      const bf16x8 a0 = l8_frag(g.x, g.y), a1 = l8_frag(g.z, g.w);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[mb] = mfma32(a0, lds_frag<ROWB>(lds, mb * 32 + r, ch0 + 2 * q), acc[mb]);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[mb] = mfma32(a1, lds_frag<ROWB>(lds, mb * 32 + r, ch0 + 2 * q + 1), acc[mb]);
    }
  };

  uint4 w[L8_RING][4];
  loadw(0, w[0]);
  loadw(1, w[1]);
  for (int c0 = 0; c0 < NC; c0 += L8_RING) {
#pragma unroll
    for (int j = 0; j < L8_RING; ++j) {
      const int c = c0 + j;
      if (c < NC) {
        if ((2 * c) % G == 0) stage(2 * c / G);
        loadw(c + 2, w[(j + 2) % L8_RING]);
        compute(c, 0, w[j]);
        if (G == 1) stage(2 * c + 1);
        compute(c, 1, w[j]);
      }
    }
  }

  // the four waves' partials, added in wave order by one writer per element
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);  // [wave][mb][register][lane]
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) red[((wave * MB + mb) * 16 + i) * 64 + lane] = acc[mb][i];
  }
  __syncthreads();
  float v[MB][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 4 * wave + q;
    const int n = n0 + acc_row(i, h);
    const int e = we[min(n, N - 1)];
    const float b = (bias != nullptr && n < N) ? bf2f(bias[n]) : 0.f;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      float s = red[(mb * 16 + i) * 64 + lane];
#pragma unroll
      for (int ww = 1; ww < L8_WAVES; ++ww) s += red[((ww * MB + mb) * 16 + i) * 64 + lane];
      s = ldexpf(s, e);  // exact: the row's power of two, once per output
      if (bias != nullptr) s += b;
      v[mb][q] = l8_act(s, act);
    }
  }
  __syncthreads();
  bf16_t* tile = reinterpret_cast<bf16_t*>(lds);  // [m][L8_TILE_LD]: y, transposed back
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[(mb * 32 + r) * L8_TILE_LD + acc_row(4 * wave + q, h)] = f2bf(v[mb][q]);
  }
  __syncthreads();
  const int n = tid & 31;
  if (n0 + n < N) {
    for (int m = tid >> 5; m < M; m += NT / 32) y[(int64_t)m * ldy + n0 + n] = tile[m * L8_TILE_LD + n];
  }
}

bool launch_linear_rows_fp8(const uint16_t* x, int64_t ldx, const uint8_t* W8, int64_t ldw, const int8_t* we,
                            const uint16_t* bias, uint16_t* y, int64_t ldy, int M, int64_t N, int K, int act,
                            hipStream_t s) {
  if (!x || !W8 || !we || !y || M < 1 || M > 128 || N < 1 || N > 0x7fffffffLL - L8_ROWS || K < 64 || K % 64) return false;
  if (ldx < K || ldw < K || ldy < N || ldx % 8 || ldw % 16 || act < 0 || act > 3) return false;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(W8) % 16) return false;
  const dim3 grid((unsigned)((N + L8_ROWS - 1) / L8_ROWS)), block(64 * L8_WAVES);
  if (M <= 32)
    hipLaunchKernelGGL((linear_rows_fp8_kernel<1>), grid, block, 0, s, x, ldx, W8, ldw, we, bias, y, ldy, M, (int)N, K, act);
  else if (M <= 64)
    hipLaunchKernelGGL((linear_rows_fp8_kernel<2>), grid, block, 0, s, x, ldx, W8, ldw, we, bias, y, ldy, M, (int)N, K, act);
  else
    hipLaunchKernelGGL((linear_rows_fp8_kernel<4>), grid, block, 0, s, x, ldx, W8, ldw, we, bias, y, ldy, M, (int)N, K, act);
  return true;
}

}  // namespace dpa
