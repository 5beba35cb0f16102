// DiffuSeq decoding: one reverse-process update outside the model as one kernel.
//
// Every sampler the decoder offers (ancestral or DDIM, full or respaced chain) reduces, on the
// target positions, to
//
//   x_{t-1} = a x0_hat + b x_t + s z          (a, b, s: one value per step, kernel arguments)
//
// with the source positions held at x_start.  x0_hat is the model's bf16 prediction, or - at the
// steps where DiffuSeq rounds it to its nearest word embedding - scale * W[idx] gathered from the
// fp32 table, so the rounded [N, E] tensor never exists.  The output is written in fp32 (the
// chain's state) and, on request, in bf16 (the next model input).
//
// The multistep DPM-Solver++ (2M) samplers add the previous update's x0_hat,
//
//   x_{t-1} = a x0_hat + a_prev x0_hat_prev + b x_t + s z
//
// from a second source of the same two kinds (PREV instantiations); it draws no noise.  Without
// it (a_prev == 0) the kernel is the three-term one, instruction for instruction.
//
// Noise contract: z depends on (seed, step, global row, column) only.  One Philox block serves a
// group of 4 columns; its key is (seed, step) and its counter the 64-bit global group index
// ((row_base + n) E + c) / 4.  Nothing of the launch geometry, of the batch a row happens to be
// in, or of training's RNG state (common.h g_rng_base is NOT added) enters, so a row decodes to
// the same bits in whatever batch it is placed.  With tau > 0, z is the standard normal
// truncated to [-tau, tau], drawn by inverse CDF (DiffuSeq's top_p re-draw loop produces this
// distribution; here there is no loop and no host synchronisation).
//
// Layout as emb_qsample_fwd (diffusion.hip): E/4 consecutive lanes own a row, 16-byte fp32
// vectors, grid-stride loop, 256-thread blocks; bandwidth-bound, no LDS, no atomics.
#include "common.h"
#include "launchers.h"

namespace dpa {

// distinguishes the decoding noise from every training stream drawn under the same seed
constexpr uint32_t RS_DOMAIN = 0x52657653u;

template <bool TRUNC>
__device__ __forceinline__ void rs_noise4(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint64_t grp,
                                          float tau, float erf_tau, float out[4]) {
  uint32_t r[4];
  philox4(seed_lo, step, (uint32_t)grp, (uint32_t)(grp >> 32), seed_hi, RS_DOMAIN, r);
  if (TRUNC) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // 2u - 1 for the centred 24-bit u = ((r >> 8) + 1/2) / 2^24 in (0, 1): an odd integer of
      // magnitude < 2^24 (exact in fp32) over 2^24, so |v| < erf_tau <= 1
      const int m = (int)(r[k] >> 8) * 2 + 1 - 16777216;
      const float v = (float)m * (1.0f / 16777216.0f) * erf_tau;
      const float z = 1.4142135623730951f * erfinvf(v);
      out[k] = fminf(fmaxf(z, -tau), tau);  // the last ulps of erf_tau / erfinvf stay inside
    }
  } else {
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // Box-Muller, as normal4 (diffusion.hip)
      const float u1 = ((float)(r[2 * k] >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
      const float u2 = (float)(r[2 * k + 1] >> 8) * (1.0f / 16777216.0f);
      const float rad = sqrtf(-2.0f * __logf(u1));
      float sn, cs;
      __sincosf(6.283185307179586f * u2, &sn, &cs);
      out[2 * k] = rad * cs;
      out[2 * k + 1] = rad * sn;
    }
  }
}

// x0_hat of one 4-column group from its source: the bf16 prediction, else scale * W[idx[row]] (an
// id outside [0, V): a zero row), else zero.
__device__ __forceinline__ f32x4 rs_x0(const bf16_t* __restrict__ pred, const int64_t* __restrict__ idx,
                                       const float* __restrict__ W, int64_t row, int g, int64_t o, int E, int V,
                                       float scale) {
  f32x4 x0 = {0.f, 0.f, 0.f, 0.f};
  if (pred) {
    const uint2 raw = *reinterpret_cast<const uint2*>(pred + o);
    x0[0] = __uint_as_float(raw.x << 16);
    x0[1] = __uint_as_float(raw.x & 0xffff0000u);
    x0[2] = __uint_as_float(raw.y << 16);
    x0[3] = __uint_as_float(raw.y & 0xffff0000u);
  } else if (idx) {
    const int64_t id = idx[row];
    if (id >= 0 && id < V) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(W + id * E + g * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) x0[k] = scale * w[k];
    }
  }
  return x0;
}

// x (b != 0), pred or idx + W (a != 0), mask + x_start and out16 are optional (null).  PREV: the
// launcher guarantees a_prev != 0 and pred_prev or idx_prev + W; otherwise the three are not read.
template <bool TRUNC, bool PREV>
__global__ void __launch_bounds__(256) reverse_step_kernel(
    const float* __restrict__ x, const bf16_t* __restrict__ pred, const int64_t* __restrict__ idx,
    const float* __restrict__ W, const float* __restrict__ x_start, const int64_t* __restrict__ mask,
    int64_t N, int E, int V, float scale, float a, float b, float s, uint32_t seed_lo, uint32_t seed_hi,
    uint32_t step, uint64_t row_base, float tau, float erf_tau, float* __restrict__ out,
    bf16_t* __restrict__ out16, const bf16_t* __restrict__ pred_prev, const int64_t* __restrict__ idx_prev,
    float a_prev) {
  const int vpr = E >> 2;  // 16-byte vectors per row
  const int64_t n = N * vpr;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = q / vpr;
    const int g = (int)(q - row * vpr);
    const int64_t o = row * E + g * 4;
    f32x4 y;
    if (mask && mask[row] == 0) {
      y = *reinterpret_cast<const f32x4*>(x_start + o);
    } else {
      f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, xt = {0.f, 0.f, 0.f, 0.f};
      if (a != 0.f) x0 = rs_x0(pred, idx, W, row, g, o, E, V, scale);
      if (b != 0.f) xt = *reinterpret_cast<const f32x4*>(x + o);
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (s != 0.f) {
        const uint64_t grp = (row_base + (uint64_t)row) * (uint64_t)vpr + (uint64_t)g;
        rs_noise4<TRUNC>(seed_lo, seed_hi, step, grp, tau, erf_tau, z);
      }
      if (PREV) {
        const f32x4 x0p = rs_x0(pred_prev, idx_prev, W, row, g, o, E, V, scale);
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fmaf(a, x0[k], fmaf(a_prev, x0p[k], fmaf(b, xt[k], s * z[k])));
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fmaf(a, x0[k], fmaf(b, xt[k], s * z[k]));
      }
    }
    *reinterpret_cast<f32x4*>(out + o) = y;
    if (out16) {
      uint2 raw;
      raw.x = pack_bf2(y[0], y[1]);
      raw.y = pack_bf2(y[2], y[3]);
      *reinterpret_cast<uint2*>(out16 + o) = raw;
    }
  }
}

bool launch_reverse_step(const float* x, const uint16_t* pred, const int64_t* idx, const float* W,
                         const float* x_start, const int64_t* mask, int64_t N, int E, int V, float scale,
                         float a, float b, float s, uint64_t seed, uint32_t step, uint64_t row_base,
                         float tau, float erf_tau, float* out, uint16_t* out16, hipStream_t st,
                         const uint16_t* pred_prev, const int64_t* idx_prev, float a_prev) {
  if (E <= 0 || E % 4 != 0 || N <= 0 || out == nullptr) return false;
  if (b != 0.f && x == nullptr) return false;
  if (a != 0.f && pred == nullptr && (idx == nullptr || W == nullptr)) return false;
  if (a_prev != 0.f && pred_prev == nullptr && (idx_prev == nullptr || W == nullptr)) return false;
  if (mask != nullptr && x_start == nullptr) return false;
  int64_t g = (N * (E / 4) + 255) / 256;
  if (g > 256 * 16) g = 256 * 16;
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  const bool trunc = tau > 0.f, prev = a_prev != 0.f;  // a_prev == 0: the three-term kernel, no previous source read
  auto kern = trunc ? (prev ? reverse_step_kernel<true, true> : reverse_step_kernel<true, false>)
                    : (prev ? reverse_step_kernel<false, true> : reverse_step_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(256), 0, st, x, (const bf16_t*)pred, idx, W, x_start, mask, N, E, V,
                     scale, a, b, s, lo, hi, step, row_base, tau, erf_tau, out, (bf16_t*)out16,
                     prev ? (const bf16_t*)pred_prev : nullptr, prev ? idx_prev : nullptr, a_prev);
  return true;
}

}  // namespace dpa
