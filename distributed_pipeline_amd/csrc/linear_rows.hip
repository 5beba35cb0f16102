// K-M26: the Linears of a GPT-2 decode step - a few rows against a whole weight matrix.
//
//   x [M][K] bf16      1 <= M <= 128 rows, ldx elements apart (ldx % 8 == 0, 16-byte aligned base)
//   W [N][K] bf16      row-major, the layout of every layers.Linear and of the tied wte; rows ldw
//                      elements apart (ldw >= K, ldw % 8 == 0): a row slice of a larger matrix works
//   bias [N] bf16      or null
//   y [M][N] bf16      y[m][n] = bf16(act(sum_k x[m][k] W[n][k] + bias[n])), rows ldy elements apart
//
// Products and sums are fp32 (MFMA accumulators), the bias is added and act (the codes of act.h) is
// applied in fp32, and there is one rounding, to bf16.  K % 64 == 0; any N >= 1.
//
// The problem: every weight element is used once per launch, by all M rows at once, so the step is a
// stream of W from HBM with a little matrix work hanging off it.  The kernel computes y^T = W x^T on
// v_mfma_f32_32x32x16_bf16 with W as the A operand (32 weight rows per MFMA) and x as the B operand
// (32 rows of x per MFMA, MB = ceil(M / 32) accumulators of 16 VGPRs).
//
// Work split.  A workgroup of 4 waves owns 32 weight rows (grid = ceil(N / 32)) and all of K.  K is
// cut into chunks of 256; inside chunk c wave w owns the 64 elements c 256 + w 64 .. + 63, so the
// four waves of a workgroup take a weight row in consecutive 128-byte lines.  There is no split of K
// across workgroups: one launch, no workspace, no second pass.
//
// k order (the mapping of the hardware's k = 8 h + j, lane l, r = l & 31, h = l >> 5, j = 0 .. 7, onto
// the wave's 64 elements; A and B use the same one, so any permutation is a valid product).  A wave's
// piece of a chunk takes four MFMA steps s = 0 .. 3, and in step s
//
//     lane (r, h), element j   <->   k = c 256 + w 64 + h 32 + s 8 + j
//
// The natural order (k = s 16 + 8 h + j) would have a lane touch its weight row in four 16-byte
// fragments 32 bytes apart.  Here lane half h walks 64 contiguous bytes of row r in its four steps
// and the two halves together walk one whole 128-byte line: every line of W a wave touches is
// consumed completely by the four loads it issues back to back, none is fetched for one fragment.
//
// A operand.  Lane (r, h)'s fragment of step s is 16 contiguous bytes of weight row n0 + r, loaded
// from global memory straight into registers; W has no reuse, so it never sees LDS.  A lane whose row
// is at or beyond N reads row N - 1 instead and holds zero fragments: nothing at or beyond W[N] is
// ever loaded.
//
// Latency.  With no reuse the stream is hidden only by bytes in flight: a wave keeps a ring of three
// register sets of four fragments (3 x 16 VGPRs).  While it computes on the set of chunk c the sets
// of chunks c + 1 and c + 2 are in flight: 8 fragments = 8 KB per wave, 32 KB per workgroup.
//
// B operand.  x is staged through 64 KB of LDS with swz: MB 32 rows of 4 / MB chunks at a time (512,
// 1024 or 2048 bytes per row), read back as ds_read_b128 fragments of 32 consecutive rows at one
// 16-byte column, which swz keeps conflict-free.  Every fragment serves the wave's MB accumulators'
// columns once; the rows m >= M of the last block are written to LDS as zeros - their threads read
// row M - 1 again, never anything beyond x - and the columns k >= K likewise.  How many chunks are staged together depends on MB, the order in
// which an accumulator receives its MFMAs does not: chunk by chunk, step by step.
//
// The row contract.  Column m of an MFMA result depends on column m of B alone, each wave folds its
// pieces in chunk order, and the four partial accumulators are added through LDS in wave order,
// ((p0 + p1) + p2) + p3, by one writer per element.  So the bits of y[m][n] are a function of x[m][:],
// W[n][:], bias[n], act, K and N - not of M, of the row's place in the call, of the other rows or of
// the grid.  One MFMA shape serves every M; the instantiations differ in the number of 32-row blocks
// (1, 2, 4) only.  No atomics.
//
// Epilogue.  Partials go to LDS in register layout ([wave][block][register][lane], conflict-free);
// wave w sums registers 4 w .. 4 w + 3 of every block, adds the bias, applies act and rounds; the
// accumulator holds y^T (register -> weight row, lane -> m), so the bf16 tile is transposed through
// LDS ([m][34]) and the stores run along n: 32 lanes write 32 consecutive 2-byte elements of a row
// of y.  Rows m >= M and columns n >= N are not stored.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), MB = 1 / 2 / 4:
// 188 / 168 / 174 VGPRs + 16 / 32 / 64 AGPRs (the accumulators), 62 SGPRs, 65536 bytes of LDS, scratch 0:
// two workgroups per compute unit, by LDS.
#include "act.h"
#include "common.h"
#include "launchers.h"
#include "mfma.h"

namespace dpa {

constexpr int LR_WAVES = 4;
constexpr int LR_ROWS = 32;   // weight rows per workgroup: one MFMA row block
constexpr int LR_KC = 256;    // k per chunk: 64 per wave, 32 per lane half
constexpr int LR_LDS = 65536;
constexpr int LR_TILE_LD = 34;  // bf16 elements per row of the transposed tile: 17 dwords, odd

template <int MB>
__global__ void __launch_bounds__(64 * LR_WAVES) linear_rows_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ W, int64_t ldw,
    const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int64_t ldy, int M, int N, int K, int act) {
  constexpr int G = 4 / MB;               // chunks staged together
  constexpr int ROWB = LR_KC * 2 * G;     // bytes of a staged row of x
  constexpr int CPR = ROWB / 16;          // its 16-byte pieces
  constexpr int NT = 64 * LR_WAVES;
  constexpr int PIECES = MB * 32 * CPR / NT;  // per thread and stage: 16
  static_assert(MB * 32 * ROWB == LR_LDS, "a stage fills the LDS buffer");
  static_assert(LR_WAVES * MB * 16 * 64 * 4 <= LR_LDS && MB * 32 * LR_TILE_LD * 2 <= LR_LDS, "epilogue fits");
  __shared__ __attribute__((aligned(16))) char lds[LR_LDS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * LR_ROWS;
  const bool row_ok = n0 + r < N;
  const int NC = (K + LR_KC - 1) / LR_KC;

  // The wave's four fragments of chunk c.  Every load is unconditional, from an address inside W: a lane
  // without a row reads row N - 1 and keeps zeros, a wave without a piece in the chunk (the tail chunk,
  // or the ring running past the end) reads its lane's first 64 bytes of the row again and compute()
  // skips the set.  Without a branch around the loads the compiler counts them in flight exactly,
  // instead of draining the ring at every join.
  auto loadw = [&](int c, bf16x8 f[4]) {
    const int k = c * LR_KC + wave * 64;  // K % 64 == 0: a piece is inside or outside
    const bf16_t* p = W + (int64_t)min(n0 + r, N - 1) * ldw + (k < K ? k : 0) + h * 32;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 g = ld_frag(p + s * 8);
      f[s] = row_ok ? g : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };

  // chunks sc G .. sc G + G - 1 of x into LDS; rows >= M and columns >= K as zeros
  auto stage = [&](int sc) {
    uint4 v[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int p = tid + NT * i, row = p / CPR, ch = p % CPR;
      const int k = sc * (LR_KC * G) + ch * 8;
      // unconditional, from an address inside x; what lies outside becomes zeros
      const uint4 g = *reinterpret_cast<const uint4*>(x + (int64_t)min(row, M - 1) * ldx + (k < K ? k : 0));
      v[i] = (row < M && k < K) ? g : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();  // every wave is done with the previous stage
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int p = tid + NT * i, row = p / CPR, ch = p % CPR;
      *reinterpret_cast<uint4*>(lds + swz<ROWB>(row, ch)) = v[i];
    }
    __syncthreads();
  };

  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = zero16();

  auto compute = [&](int c, const bf16x8 f[4]) {
    if (c * LR_KC + wave * 64 >= K) return;  // wave-uniform: the tail chunk has no piece for this wave
    const int ch0 = (c % G) * (LR_KC / 8) + wave * 8 + h * 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        acc[mb] = mfma32(f[s], lds_frag<ROWB>(lds, mb * 32 + r, ch0 + s), acc[mb]);
    }
  };

  bf16x8 w[3][4];
  loadw(0, w[0]);
  loadw(1, w[1]);
  for (int c0 = 0; c0 < NC; c0 += 3) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int c = c0 + j;
      if (c < NC) {
        if (c % G == 0) stage(c / G);
        loadw(c + 2, w[(j + 2) % 3]);
        compute(c, w[j]);
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
  for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * wave + q;
      float s = red[(mb * 16 + i) * 64 + lane];
#pragma unroll
      for (int ww = 1; ww < LR_WAVES; ++ww) s += red[((ww * MB + mb) * 16 + i) * 64 + lane];
      const int n = n0 + acc_row(i, h);
      if (bias != nullptr && n < N) s += bf2f(bias[n]);
      v[mb][q] = act_apply(s, act);
    }
  }
  __syncthreads();
  bf16_t* tile = reinterpret_cast<bf16_t*>(lds);  // [m][LR_TILE_LD]: y, transposed back
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[(mb * 32 + r) * LR_TILE_LD + acc_row(4 * wave + q, h)] = f2bf(v[mb][q]);
  }
  __syncthreads();
  const int n = tid & 31;
  if (n0 + n < N) {
    for (int m = tid >> 5; m < M; m += NT / 32) y[(int64_t)m * ldy + n0 + n] = tile[m * LR_TILE_LD + n];
  }
}

bool launch_linear_rows(const uint16_t* x, int64_t ldx, const uint16_t* W, int64_t ldw, const uint16_t* bias,
                        uint16_t* y, int64_t ldy, int M, int64_t N, int K, int act, hipStream_t s) {
  if (!x || !W || !y || M < 1 || M > 128 || N < 1 || N > 0x7fffffffLL - LR_ROWS || K < 64 || K % 64) return false;
  if (ldx < K || ldw < K || ldy < N || ldx % 8 || ldw % 8 || act < 0 || act > 3) return false;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(W) % 16) return false;
  const dim3 grid((unsigned)((N + LR_ROWS - 1) / LR_ROWS)), block(64 * LR_WAVES);
  if (M <= 32)
    hipLaunchKernelGGL((linear_rows_kernel<1>), grid, block, 0, s, x, ldx, W, ldw, bias, y, ldy, M, (int)N, K, act);
  else if (M <= 64)
    hipLaunchKernelGGL((linear_rows_kernel<2>), grid, block, 0, s, x, ldx, W, ldw, bias, y, ldy, M, (int)N, K, act);
  else
    hipLaunchKernelGGL((linear_rows_kernel<4>), grid, block, 0, s, x, ldx, W, ldw, bias, y, ldy, M, (int)N, K, act);
  return true;
}

}  // namespace dpa
