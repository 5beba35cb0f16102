// K-M30: a decode step's sublayer in one launch - LayerNorm -> Linear (+ act) -> + residual on a few rows.
//
//   x [M][K] bf16         1 <= M <= 128 rows, ldx elements apart (ldx % 8 == 0, 16-byte aligned base)
//   gamma, beta [K] bf16  the LayerNorm's scale and shift (LN), 16-byte aligned
//   W [N][K] bf16         row-major, rows ldw elements apart (ldw >= K, ldw % 8 == 0)
//   bias [N] bf16         or null
//   res [M][N] bf16       the residual stream (RES), rows ldr elements apart; no alignment asked
//   y [M][N] bf16         rows ldy elements apart; may not overlap x or res
//
//   mean_m = (sum_k x[m][k]) / K
//   var_m  = (sum_k (x[m][k] - mean_m)^2) / K                     two passes over the row
//   a[m][k] = bf16((x[m][k] - mean_m) rsqrt(var_m + eps) gamma[k] + beta[k])     (without LN: a = x)
//   y[m][n] = bf16(act(sum_k a[m][k] W[n][k] + bias[n]) + res[m][n])             one rounding
//
// All arithmetic is fp32.  K % 64 == 0; any N >= 1.  This is K-M26 (linear_rows.hip) with a prologue in
// front of its chunk loop and a residual read in its store phase; the work split (32 weight rows and all
// of K per workgroup of 4 waves), the k order, the weight ring of three register sets, the swizzled LDS
// image of x, the MFMA loop and the wave-order sum of the partials are K-M26's and are described there.
// It lives in a file of its own so that K-M26's instantiations keep their generated code.
//
// Prologue (LN).  A workgroup needs mean and rstd of all M rows before it can stage a piece of x, and
// there is no cross-workgroup dependency to get them from: every workgroup computes them itself, one more
// read of x through L2 (M K 2 bytes per workgroup).  Row m belongs to wave m & 3; a wave takes its rows
// eight at a time (eight independent 16-byte loads in flight per lane).  Lane l owns the pieces
// k = 8 l + 512 t, t = 0, 1, ..., adds their elements in k order, and the 64 lane sums go through a
// butterfly (xor 32, 16, .. 1: every lane ends with the same bits).  The squared deviations take the same
// route with fmaf(d, d, s), re-reading the row (an L1/L2 hit).  Lanes, pieces and order depend on K alone.
// mean and var are true divisions by K (a constant row gives mean == x exactly, var == 0).  The weight
// ring's first two sets are issued before the prologue, so the HBM latency of W runs under it.
//
// The statistics live in 1 KB of LDS ([128] float2) beside the 64 KB stage buffer: 66560 bytes of static
// LDS in the LN instantiations, still two workgroups per compute unit by LDS (gfx950 has 160 KB per
// compute unit).  Holding them in the staging threads' registers would cost 32 VGPRs all through the chunk
// loop (a thread stages pieces of 16 rows).
//
// stage() applies them where a 16-byte piece of x is on its way into the LDS image: a thread's 16 pieces
// of a stage are 16 rows at one column (256 threads are a multiple of the pieces of a row), so it loads
// one piece of gamma and one of beta per stage and 16 float2 of statistics.  Per element: d = x - mean,
// u = d rstd, a = bf16(fmaf(u, gamma, beta)) - written out so that no contraction is left to the compiler.
// Rows m >= M and columns k >= K are staged as zeros, never as normalised garbage; their threads read row
// M - 1 / column 0 and statistics row M - 1 again.
//
// Epilogue (RES).  The four waves' partials are added in wave order, bias and act applied in fp32 as in
// K-M26; the tile that is transposed through LDS holds fp32 ([m][33]) instead of bf16, and the thread that
// stores y[m][n] reads res[m][n] (along n, coalesced like the store), adds it in fp32 and rounds once.
// Without RES the tile is K-M26's bf16 one and y equals K-M26 on the rounded a bit for bit.
//
// The row contract.  The bits of a[m][:] are a function of x[m][:], gamma, beta, eps and K alone; the bits
// of y[m][n] additionally of W[n][:], bias[n], act and res[m][n] - not of M, of the row's place, of N for
// a, of the other rows or of the grid.  No atomics, no workspace, two calls bit-equal.  Nothing at or
// beyond x[M], W[N], res[M] is loaded; rows m >= M and columns n >= N are not stored.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), scratch 0 in all nine;
// VGPRs + AGPRs (the accumulators) for MB = 1 / 2 / 4, LDS bytes, waves per SIMD:
//   LN        222 + 16 / 199 + 32 / 207 + 64    66560    2 / 2 / 1
//   RES       192 + 16 / 168 + 32 / 174 + 64    65536    2 / 2 / 2
//   LN + RES  222 + 16 / 199 + 32 / 207 + 64    66560    2 / 2 / 1
// LN at MB = 4 (M > 64) needs 271 registers and runs one workgroup per compute unit.  Forcing two (a second
// __launch_bounds__ argument) spills 36 bytes per lane, and the LN Linears of a decode step (qkv, mlp_fc: N <= 4 K)
// have fewer workgroups than the device has compute units, so the second slot would stay empty anyway.
#include "act.h"
#include "common.h"
#include "launchers.h"
#include "mfma.h"

namespace dpa {

constexpr int LRF_WAVES = 4;
constexpr int LRF_ROWS = 32;      // weight rows per workgroup: one MFMA row block
constexpr int LRF_KC = 256;       // k per chunk: 64 per wave, 32 per lane half
constexpr int LRF_STAGE = 65536;  // the LDS image of x; the epilogue's buffers reuse it
constexpr int LRF_MAXM = 128;
constexpr int LRF_TILE_LD = 34;   // bf16 elements per row of the transposed tile: 17 dwords, odd
constexpr int LRF_TILE32_LD = 33; // fp32 elements per row of the transposed tile (RES)
constexpr int LRF_RG = 8;         // rows a wave takes together in the prologue

template <int MB, bool LN, bool RES>
__global__ void __launch_bounds__(64 * LRF_WAVES) linear_rows_fused_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ gamma, const bf16_t* __restrict__ beta,
    float eps, const bf16_t* __restrict__ W, int64_t ldw, const bf16_t* __restrict__ bias,
    const bf16_t* __restrict__ res, int64_t ldr, bf16_t* __restrict__ y, int64_t ldy, int M, int N, int K, int act) {
  constexpr int G = 4 / MB;               // chunks staged together
  constexpr int ROWB = LRF_KC * 2 * G;    // bytes of a staged row of x
  constexpr int CPR = ROWB / 16;          // its 16-byte pieces
  constexpr int NT = 64 * LRF_WAVES;
  constexpr int PIECES = MB * 32 * CPR / NT;  // per thread and stage: 16
  static_assert(MB * 32 * ROWB == LRF_STAGE, "a stage fills the LDS buffer");
  static_assert(NT % CPR == 0, "a thread's pieces of a stage share one column");
  static_assert(LRF_WAVES * MB * 16 * 64 * 4 <= LRF_STAGE && MB * 32 * LRF_TILE_LD * 2 <= LRF_STAGE &&
                    MB * 32 * LRF_TILE32_LD * 4 <= LRF_STAGE, "epilogue fits");
  __shared__ __attribute__((aligned(16))) char lds[LRF_STAGE];
  __shared__ float2 stat[LN ? LRF_MAXM : 1];  // (mean, rstd) of row m

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * LRF_ROWS;
  const bool row_ok = n0 + r < N;
  const int NC = (K + LRF_KC - 1) / LRF_KC;

  // K-M26's loadw: unconditional loads from inside W, zeros kept for a lane without a row
  auto loadw = [&](int c, bf16x8 f[4]) {
    const int k = c * LRF_KC + wave * 64;
    const bf16_t* p = W + (int64_t)min(n0 + r, N - 1) * ldw + (k < K ? k : 0) + h * 32;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 g = ld_frag(p + s * 8);
      f[s] = row_ok ? g : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };

  bf16x8 w[3][4];
  loadw(0, w[0]);
  loadw(1, w[1]);

  if constexpr (LN) {
    // rows wave, wave + 4, ... of x, LRF_RG at a time; a row at or beyond M reads row M - 1 and writes nothing
    const float fK = (float)K;
    for (int m0 = wave; m0 < M; m0 += 4 * LRF_RG) {
      const bf16_t* xr[LRF_RG];
#pragma unroll
      for (int i = 0; i < LRF_RG; ++i) xr[i] = x + (int64_t)min(m0 + 4 * i, M - 1) * ldx;
      float mean[LRF_RG], s[LRF_RG];
#pragma unroll
      for (int i = 0; i < LRF_RG; ++i) s[i] = 0.f;
      for (int k = lane * 8; k < K; k += 512) {
        bf16x8 g[LRF_RG];
#pragma unroll
        for (int i = 0; i < LRF_RG; ++i) g[i] = ld_frag(xr[i] + k);
#pragma unroll
        for (int i = 0; i < LRF_RG; ++i) {
#pragma unroll
          for (int j = 0; j < 8; ++j) s[i] += bf2f((bf16_t)g[i][j]);
        }
      }
#pragma unroll
      for (int i = 0; i < LRF_RG; ++i) {
        mean[i] = wave_sum(s[i]) / fK;
        s[i] = 0.f;
      }
      for (int k = lane * 8; k < K; k += 512) {
        bf16x8 g[LRF_RG];
#pragma unroll
        for (int i = 0; i < LRF_RG; ++i) g[i] = ld_frag(xr[i] + k);
#pragma unroll
        for (int i = 0; i < LRF_RG; ++i) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = bf2f((bf16_t)g[i][j]) - mean[i];
            s[i] = __builtin_fmaf(d, d, s[i]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < LRF_RG; ++i) {
        const float rstd = rsqrtf(wave_sum(s[i]) / fK + eps);
        if (lane == 0 && m0 + 4 * i < M) stat[m0 + 4 * i] = make_float2(mean[i], rstd);
      }
    }
    __syncthreads();
  }

  // chunks sc G .. sc G + G - 1 of a into LDS; rows >= M and columns >= K as zeros
  auto stage = [&](int sc) {
    uint4 v[PIECES];
    const int ch = tid % CPR;
    const int k = sc * (LRF_KC * G) + ch * 8;
    const int kk = k < K ? k : 0;
    bf16x8 gm, bt;
    if constexpr (LN) {
      gm = ld_frag(gamma + kk);
      bt = ld_frag(beta + kk);
    }
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int row = (tid + NT * i) / CPR;
      // unconditional, from an address inside x; what lies outside becomes zeros
      uint4 g = *reinterpret_cast<const uint4*>(x + (int64_t)min(row, M - 1) * ldx + kk);
      if constexpr (LN) {
        const float2 st = stat[min(row, M - 1)];
        const bf16x8 e = __builtin_bit_cast(bf16x8, g);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = bf2f((bf16_t)e[j]) - st.x;
          const float u = d * st.y;
          o[j] = (short)f2bf(__builtin_fmaf(u, bf2f((bf16_t)gm[j]), bf2f((bf16_t)bt[j])));
        }
        g = __builtin_bit_cast(uint4, o);
      }
      v[i] = (row < M && k < K) ? g : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();  // every wave is done with the previous stage
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int row = (tid + NT * i) / CPR;
      *reinterpret_cast<uint4*>(lds + swz<ROWB>(row, ch)) = v[i];
    }
    __syncthreads();
  };

  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = zero16();

  auto compute = [&](int c, const bf16x8 f[4]) {
    if (c * LRF_KC + wave * 64 >= K) return;  // wave-uniform: the tail chunk has no piece for this wave
    const int ch0 = (c % G) * (LRF_KC / 8) + wave * 8 + h * 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        acc[mb] = mfma32(f[s], lds_frag<ROWB>(lds, mb * 32 + r, ch0 + s), acc[mb]);
    }
  };

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
      for (int ww = 1; ww < LRF_WAVES; ++ww) s += red[((ww * MB + mb) * 16 + i) * 64 + lane];
      const int n = n0 + acc_row(i, h);
      if (bias != nullptr && n < N) s += bf2f(bias[n]);
      v[mb][q] = act_apply(s, act);
    }
  }
  __syncthreads();
  const int n = tid & 31;
  if constexpr (RES) {
    float* tile = reinterpret_cast<float*>(lds);  // [m][LRF_TILE32_LD]: act(..) in fp32, transposed back
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
      for (int q = 0; q < 4; ++q) tile[(mb * 32 + r) * LRF_TILE32_LD + acc_row(4 * wave + q, h)] = v[mb][q];
    }
    __syncthreads();
    if (n0 + n < N) {
      for (int m = tid >> 5; m < M; m += NT / 32)
        y[(int64_t)m * ldy + n0 + n] = f2bf(tile[m * LRF_TILE32_LD + n] + bf2f(res[(int64_t)m * ldr + n0 + n]));
    }
  } else {
    bf16_t* tile = reinterpret_cast<bf16_t*>(lds);  // [m][LRF_TILE_LD]: y, transposed back
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
      for (int q = 0; q < 4; ++q) tile[(mb * 32 + r) * LRF_TILE_LD + acc_row(4 * wave + q, h)] = f2bf(v[mb][q]);
    }
    __syncthreads();
    if (n0 + n < N) {
      for (int m = tid >> 5; m < M; m += NT / 32) y[(int64_t)m * ldy + n0 + n] = tile[m * LRF_TILE_LD + n];
    }
  }
}

template <int MB, bool LN, bool RES>
static void lrf_launch(dim3 grid, hipStream_t s, const uint16_t* x, int64_t ldx, const uint16_t* gamma,
                       const uint16_t* beta, float eps, const uint16_t* W, int64_t ldw, const uint16_t* bias,
                       const uint16_t* res, int64_t ldr, uint16_t* y, int64_t ldy, int M, int N, int K, int act) {
  hipLaunchKernelGGL((linear_rows_fused_kernel<MB, LN, RES>), grid, dim3(64 * LRF_WAVES), 0, s, x, ldx, gamma, beta,
                     eps, W, ldw, bias, res, ldr, y, ldy, M, N, K, act);
}

template <bool LN, bool RES, class... A>
static void lrf_by_rows(int M, A... a) {
  if (M <= 32)
    lrf_launch<1, LN, RES>(a...);
  else if (M <= 64)
    lrf_launch<2, LN, RES>(a...);
  else
    lrf_launch<4, LN, RES>(a...);
}

bool launch_linear_rows_fused(const uint16_t* x, int64_t ldx, const uint16_t* gamma, const uint16_t* beta, float eps,
                              const uint16_t* W, int64_t ldw, const uint16_t* bias, const uint16_t* res, int64_t ldr,
                              uint16_t* y, int64_t ldy, int M, int64_t N, int K, int act, hipStream_t s) {
  if (!x || !W || !y || M < 1 || M > LRF_MAXM || N < 1 || N > 0x7fffffffLL - LRF_ROWS || K < 64 || K % 64) return false;
  if (ldx < K || ldw < K || ldy < N || ldx % 8 || ldw % 8 || act < 0 || act > 3) return false;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(W) % 16) return false;
  const bool ln = gamma != nullptr, rs = res != nullptr;
  if ((!ln && !rs) || (ln != (beta != nullptr)) || (rs && ldr < N)) return false;
  if (ln && (reinterpret_cast<uintptr_t>(gamma) % 16 || reinterpret_cast<uintptr_t>(beta) % 16 || !(eps >= 0.f)))
    return false;
  const dim3 grid((unsigned)((N + LRF_ROWS - 1) / LRF_ROWS));
  if (ln && rs)
    lrf_by_rows<true, true>(M, grid, s, x, ldx, gamma, beta, eps, W, ldw, bias, res, ldr, y, ldy, M, (int)N, K, act);
  else if (ln)
    lrf_by_rows<true, false>(M, grid, s, x, ldx, gamma, beta, eps, W, ldw, bias, res, ldr, y, ldy, M, (int)N, K, act);
  else
    lrf_by_rows<false, true>(M, grid, s, x, ldx, gamma, beta, eps, W, ldw, bias, res, ldr, y, ldy, M, (int)N, K, act);
  return true;
}

}  // namespace dpa
