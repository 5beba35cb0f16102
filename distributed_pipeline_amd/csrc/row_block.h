// Shared by the kernels that hold one logits row in the registers of a 1024-thread workgroup
// (sample.hip, beam_step.hip): the order-preserving float keys, the wave reductions without
// lane-address registers, and block reductions whose result every thread gets.
#pragma once
#include "common.h"

namespace dpa {

constexpr int SM_THREADS = 1024;
constexpr int SM_WAVES = SM_THREADS / DPA_WAVE;

// order-preserving float <-> uint32 (no NaN and no -0 reaches them)
__device__ __forceinline__ uint32_t sm_key(float s) {
  const uint32_t b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sm_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Wave reductions without lane-address registers (six of them, live through the whole kernel,
// are what __shfl_xor costs, and these kernels have none to spare): five xor steps inside each half
// of the wave by ds_swizzle, whose pattern is an immediate, then the two halves from lanes 0 and 32.
// Every lane is active wherever these run, and every lane ends with the same bits.
template <int X>
__device__ __forceinline__ uint32_t sm_swz(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (X << 10));  // lane ^ X within 32 lanes
}
#define SM_HALF_STEPS(STEP) STEP(16) STEP(8) STEP(4) STEP(2) STEP(1)
__device__ __forceinline__ uint32_t sm_lane(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ uint32_t sm_wave_umax(uint32_t v) {
#define SM_STEP(X) v = max(v, sm_swz<X>(v));
  SM_HALF_STEPS(SM_STEP)
#undef SM_STEP
  return max(sm_lane(v, 0), sm_lane(v, 32));
}
__device__ __forceinline__ int sm_wave_count(int v) {
#define SM_STEP(X) v += (int)sm_swz<X>((uint32_t)v);
  SM_HALF_STEPS(SM_STEP)
#undef SM_STEP
  return (int)sm_lane((uint32_t)v, 0) + (int)sm_lane((uint32_t)v, 32);
}
__device__ __forceinline__ float sm_wave_mass(float v) {
#define SM_STEP(X) v += __uint_as_float(sm_swz<X>(__float_as_uint(v)));
  SM_HALF_STEPS(SM_STEP)
#undef SM_STEP
  return __uint_as_float(sm_lane(__float_as_uint(v), 0)) + __uint_as_float(sm_lane(__float_as_uint(v), 32));
}
// arg-max of (s, lowest i) over the wave: every lane ends with the winner
__device__ __forceinline__ void sm_wave_argmax(float& bs, int& bi) {
#define SM_STEP(X)                                                        \
  {                                                                       \
    const float os = __uint_as_float(sm_swz<X>(__float_as_uint(bs)));     \
    const int oi = (int)sm_swz<X>((uint32_t)bi);                          \
    if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }           \
  }
  SM_HALF_STEPS(SM_STEP)
#undef SM_STEP
  const int half = (threadIdx.x & 32) ? 0 : 32;  // the other half's result
  const float os = __uint_as_float(half ? sm_lane(__float_as_uint(bs), 32) : sm_lane(__float_as_uint(bs), 0));
  const int oi = (int)(half ? sm_lane((uint32_t)bi, 32) : sm_lane((uint32_t)bi, 0));
  if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
}

// Block reductions whose result every thread gets, one barrier each: consecutive calls alternate
// between the two rows of `red`, so a wave that runs ahead into the next call writes the other row.
typedef uint32_t sm_red_t[2][SM_WAVES];

__device__ __forceinline__ uint32_t sm_block_umax(uint32_t v, sm_red_t red, int& ph) {
  v = sm_wave_umax(v);
  if ((threadIdx.x & 63) == 0) red[ph][threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t r = 0;
#pragma unroll
  for (int w = 0; w < SM_WAVES; ++w) r = max(r, red[ph][w]);
  ph ^= 1;
  return r;
}
// for a count that is already its wave's (equal in every lane)
__device__ __forceinline__ int sm_block_wave_count(int v, sm_red_t red, int& ph) {
  if ((threadIdx.x & 63) == 0) red[ph][threadIdx.x >> 6] = (uint32_t)v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int w = 0; w < SM_WAVES; ++w) r += (int)red[ph][w];
  ph ^= 1;
  return r;
}
__device__ __forceinline__ int sm_block_count(int v, sm_red_t red, int& ph) {
  return sm_block_wave_count(sm_wave_count(v), red, ph);
}
__device__ __forceinline__ float sm_block_mass(float v, sm_red_t red, int& ph) {
  v = sm_wave_mass(v);
  if ((threadIdx.x & 63) == 0) red[ph][threadIdx.x >> 6] = __float_as_uint(v);
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int w = 0; w < SM_WAVES; ++w) r += __uint_as_float(red[ph][w]);  // wave order
  ph ^= 1;
  return r;
}

}  // namespace dpa
