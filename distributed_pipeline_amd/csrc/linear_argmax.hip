// Fused linear + arg-max for decoding with a tied rounding head:
//
//   score[t][v] = x[t] . W[v] + c[v]         x: [N, E] bf16, W: [V, E] bf16, c: [V] fp32
//   idx[t]      = argmax_v score[t][v],      best[t] = score[t][idx[t]]
//
//   c = lm_head bias         -> the arg-max of the rounding logits (final decode);
//   c = -1/2 ||W[v]||^2      -> the nearest word embedding of x[t] (DiffuSeq's clamping
//                               trick: argmin_v ||x - W[v]||^2), row_half_sqnorm below.
//
// The [N, V] scores are never written.  The sweep (csrc/vocab_sweep.h) is shared with the
// forward of csrc/xent.hip: a workgroup is 128 tokens and walks (a split of) the vocabulary in 64-row W tiles staged
// through the swizzled LDS image; S = W x^T puts the token on the MFMA lane and the
// vocabulary in the accumulator registers, which start at c (fp32, never rounded to bf16:
// ||W[v]||^2 at bf16 precision would move the arg-min).  Where xent.hip keeps an online
// log-sum-exp per lane, this keeps a (best, idx) pair: a max tree over the tile's 32
// registers, and only a lane whose tile maximum beats its running best looks for the
// register that holds it.
//
// Tie rule: equal scores resolve to the LOWEST vocabulary index.  It is applied in all three
// places a winner is chosen:
//   * in registers  - tiles are walked in ascending row order and the running pair changes
//                     only on a strict >; inside a tile the registers are scanned from the
//                     highest row down, so the lowest row equal to the maximum is kept;
//   * half merge    - the two lane halves that share a token hold interleaved rows: the
//                     other half wins on > or on == with a lower index;
//   * split merge   - the combine kernel walks the vocabulary splits in ascending order and
//                     replaces only on a strict >.
//
// Output range: idx is in [0, V) for every row and any input.  The running index starts at
// the first row of the split; rows past the vocabulary or the split end start at -inf (a
// zero-padded W row can never win); a NaN score compares false and is skipped, so a row of
// NaN (or of all -inf) scores returns the first row with best = -inf.
#include "common.h"
#include "launchers.h"
#include "mfma.h"
#include "vocab_sweep.h"

namespace dpa {

// ---------------------------------------------------------------------------
// Sweep
// ---------------------------------------------------------------------------
template <int E>
__global__ void __launch_bounds__(256) linear_argmax_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ W, const float* __restrict__ c, int N,
    int V, int v_per_split, int64_t* __restrict__ idx_out, float* __restrict__ best_out,
    float* __restrict__ part_best, int* __restrict__ part_idx, int xsplit) {
  constexpr int KS = E / 16, ROWB = E * 2;
  __shared__ __attribute__((aligned(16))) char smem[64 * ROWB + 64 * 4];
  char* wt = smem;
  float* ct = reinterpret_cast<float*>(smem + 64 * ROWB);

  const auto [split, tblk, nsplit] = sweep_block(xsplit);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5;
  const int t = tblk * 128 + w * 32 + (lane & 31);
  const bool tok_ok = t < N;
  bf16x8 xf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) xf[s] = token_frag<E>(x, t, tok_ok, s, h);

  const int vbeg = split * v_per_split;  // < V: the launcher makes no empty split
  const int vend = min(V, vbeg + v_per_split);
  float best = -INFINITY;
  int bidx = vbeg;

  WTile<E, 256> stage;
  if (vbeg < vend) stage.load(W, vbeg, V, tid);
  for (int v0 = vbeg; v0 < vend; v0 += 64) {
    stage.store(wt, tid);
    stage_offsets(ct, v0, vend, tid, [c](int v) { return c ? c[v] : 0.f; });
    __syncthreads();
    if (v0 + 64 < vend) stage.load(W, v0 + 64, V, tid);  // prefetch next tile behind the MFMAs

    // Accumulators start at the offset of their vocabulary rows (-inf for rows past the
    // split / vocabulary), so no per-element add or tail test remains.
    f32x16 acc[2];
#pragma unroll
    for (int vt = 0; vt < 2; ++vt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 cv = *reinterpret_cast<const f32x4*>(ct + vt * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[vt][4 * g + r] = cv[r];
      }
#pragma unroll
      for (int s = 0; s < KS; ++s)
        acc[vt] = mfma32(lds_frag<ROWB>(wt, vt * 32 + (lane & 31), 2 * s + h), xf[s], acc[vt]);
    }
    // fmaxf drops a NaN operand, so NaN scores never reach tmax
    float tmax = -INFINITY;
#pragma unroll
    for (int vt = 0; vt < 2; ++vt)
#pragma unroll
      for (int i = 0; i < 16; i += 2) tmax = fmaxf(tmax, fmaxf(acc[vt][i], acc[vt][i + 1]));
    if (tmax > best) {
      // register k = 16 vt + i holds row vt*32 + acc_row(i, h): ascending in k, so the
      // downward scan leaves the lowest row equal to the maximum
      int k = 0;
#pragma unroll
      for (int vt = 1; vt >= 0; --vt)
#pragma unroll
        for (int i = 15; i >= 0; --i) k = (acc[vt][i] == tmax) ? 16 * vt + i : k;
      best = tmax;
      bidx = v0 + (k >> 4) * 32 + acc_row(k & 15, h);
    }
    __syncthreads();
  }
  // merge the two lane halves that share a token
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bidx, 32, 64);
  if (ob > best || (ob == best && oi < bidx)) {
    best = ob;
    bidx = oi;
  }
  if (h == 0 && tok_ok) {
    if (nsplit == 1) {
      idx_out[t] = bidx;
      best_out[t] = best;
    } else {
      part_best[(int64_t)split * N + t] = best;
      part_idx[(int64_t)split * N + t] = bidx;
    }
  }
}

// Merge of the vocabulary splits, in split (= ascending row) order.
__global__ void __launch_bounds__(256) linear_argmax_combine_kernel(
    const float* __restrict__ part_best, const int* __restrict__ part_idx, int N, int S,
    int64_t* __restrict__ idx_out, float* __restrict__ best_out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N) return;
  float best = part_best[t];
  int bidx = part_idx[t];
  for (int s = 1; s < S; ++s) {
    const float pb = part_best[(int64_t)s * N + t];
    if (pb > best) {
      best = pb;
      bidx = part_idx[(int64_t)s * N + t];
    }
  }
  idx_out[t] = bidx;
  best_out[t] = best;
}

// c[v] = -1/2 sum_k W[v][k]^2 in fp32 from the bf16 W: E / 8 lanes per row, 16 bytes each.
template <int E>
__global__ void __launch_bounds__(256) row_half_sqnorm_kernel(const bf16_t* __restrict__ W, int V,
                                                              float* __restrict__ c) {
  constexpr int LPR = E / 8, RPB = 256 / LPR;  // lanes per row (16 / 32), rows per block
  const int v = blockIdx.x * RPB + threadIdx.x / LPR;
  const int ch = threadIdx.x % LPR;
  float s = 0.f;
  if (v < V) {
    const uint4 q = *reinterpret_cast<const uint4*>(W + (int64_t)v * E + ch * 8);
    const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lo = __uint_as_float(u[j] << 16), hi = __uint_as_float(u[j] & 0xffff0000u);
      s = fmaf(lo, lo, s);
      s = fmaf(hi, hi, s);
    }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (v < V && ch == 0) c[v] = -0.5f * s;
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
// Vocabulary splits, chosen as launch_lxent_fwd chooses its own: enough workgroups to fill
// the chip (1024), so from 1024 token blocks (N > 130944) one workgroup sweeps the whole
// vocabulary; below that the split count is a multiple of 8 (one split per XCD).
static SweepPlan argmax_plan(int N, int V) { return sweep_plan(N, V, 1024, XcdRound::if_split); }

// ws layout: Sx x N split maxima (float), Sx x N split indices (int)
int64_t linear_argmax_workspace_floats(int N, int V) {
  const int Sx = argmax_plan(N, V).Sx;
  return Sx > 1 ? 2 * (int64_t)Sx * N : 0;
}

// ws: linear_argmax_workspace_floats(N, V) floats of scratch (the splits' (best, idx) partials)
void launch_linear_argmax(const uint16_t* x, const uint16_t* W, const float* c, int N, int V, int E,
                          int64_t* idx, float* best, float* ws, hipStream_t s) {
  const SweepPlan p = argmax_plan(N, V);
  float* pb = ws;
  int* pi = reinterpret_cast<int*>(ws + (p.Sx > 1 ? (int64_t)p.Sx * N : 0));
  const bool per_xcd = p.Sx == 8;  // one split per XCD: 1-D grid, split = blockIdx % 8
  const dim3 grid = per_xcd ? dim3(p.tb * 8) : dim3(p.tb, p.Sx);
  for_head_width(E, [&](auto e) {
    hipLaunchKernelGGL(linear_argmax_kernel<e()>, grid, dim3(256), 0, s, x, W, c, N, V, p.vps, idx, best, pb, pi,
                       per_xcd ? 8 : 0);
  });
  if (p.Sx > 1)
    hipLaunchKernelGGL(linear_argmax_combine_kernel, dim3((N + 255) / 256), dim3(256), 0, s, pb, pi, N, p.Sx,
                       idx, best);
}

void launch_row_half_sqnorm(const uint16_t* W, int V, int E, float* c, hipStream_t s) {
  if (E == 128)
    hipLaunchKernelGGL(row_half_sqnorm_kernel<128>, dim3((V + 15) / 16), dim3(256), 0, s, W, V, c);
  else
    hipLaunchKernelGGL(row_half_sqnorm_kernel<256>, dim3((V + 7) / 8), dim3(256), 0, s, W, V, c);
}

}  // namespace dpa
