// Shared by the KV-cache decode attention kernels (attn_decode.hip: one query per row;
// attn_decode_block.hip: a block of T queries per row): the lane-group online-softmax state, its
// dot and fold steps, and the launchers' argument check.  Both files fold a key in the same
// (wave, lane group, iteration) with these functions, which is what makes their results comparable
// bit for bit.
#pragma once
#include <math.h>

#include "common.h"

namespace dpa {

constexpr int AD_U = 4;      // wave loads of K (and of V) in flight per register set
constexpr int AD_WAVES = 4;

__device__ __forceinline__ void ad_unpack8(const uint4 r, float f[8]) {
  f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
  f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
  f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
  f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
}

// this lane group's running (m, l, o[8]); m in the exp2 domain, -inf while the group has no key
struct AdState {
  float m, l, o[8];
};

// q . k over the G lanes of a group (every lane of the group gets the sum)
template <int G>
__device__ __forceinline__ float ad_dot(const float q[8], const uint4 kr) {
  float kf[8];
  ad_unpack8(kr, kf);
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
#pragma unroll
  for (int off = G >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
  return d;
}

// fold N scored keys (s[u] = -inf: not a key) with their V slices into the state
template <int N>
__device__ __forceinline__ void ad_update(AdState& st, const float s[N], const uint4 vr[N]) {
  float mx = s[0];
#pragma unroll
  for (int u = 1; u < N; ++u) mx = fmaxf(mx, s[u]);
  const float mn = fmaxf(st.m, mx);
  const float ms = mn == -INFINITY ? 0.f : mn;  // no key yet: every exponent below is -inf, never NaN
  const float alpha = fexp2(st.m - ms);
  st.l *= alpha;
#pragma unroll
  for (int i = 0; i < 8; ++i) st.o[i] *= alpha;
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const float p = fexp2(s[u] - ms);
    float vf[8];
    ad_unpack8(vr[u], vf);
    st.l += p;
#pragma unroll
    for (int i = 0; i < 8; ++i) st.o[i] = fmaf(p, vf[i], st.o[i]);
  }
  st.m = mn;
}

inline bool ad_args_ok(const uint16_t* qkv_new, int64_t qkv_stride, const uint16_t* k_cache, const uint16_t* v_cache,
                       int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* lens, int B, int H,
                       int Lmax, int D, const uint16_t* out) {
  if ((D != 64 && D != 128) || B <= 0 || H <= 0 || Lmax <= 0 || (int64_t)B * H > 0x7fffffffLL) return false;
  if (!qkv_new || !k_cache || !v_cache || !lens || !out) return false;
  // 16-byte rows: every row start is a multiple of 8 elements from a 16-byte aligned base
  return !(qkv_stride % 8 || k_sb % 8 || k_sh % 8 || v_sb % 8 || v_sh % 8);
}

}  // namespace dpa
