// GPT-2 generation over a one-byte K/V cache: the quantizing append and the single-query attention
// of one decode step as one kernel (K-M25), and the quantizing store of a prefill's K and V.
//
// The format.  A cached row is the D values of one (K or V, batch row, head, position): D OCP
// e4m3fn codes and one int8 exponent e.  With a = max |x_i| over the row: e = 0 for a == 0, else
// (m, p) = frexp(a) and e = max(p - 9 + (m > 0.875), -127), so that a 2^-e lies in (224, 448] and no
// element saturates; code_i = e4m3fn(x_i 2^-e), round to nearest even, subnormals kept;
// x^_i = float(code_i) 2^e.  The scaling is by a power of two and exact for bf16 inputs wherever a
// code depends on it, so codes and exponent are a function of the input bits alone.  The conversions
// are gfx950's v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8.  Non-finite inputs: memory safe, values
// unspecified.
//
//   qkv_new [B][3][H][D] bf16     the new token's packed projection (rows qkv_stride apart)
//   k8 / v8                       code rows of D bytes at (b, h, key): base + b * sb + h * sh + key * D
//   ke / ve                       one int8 per row at (b, h, key): base + b * esb + h * esh + key
//   lens [B] int32                keys already cached per row, before the call (not modified)
//   out [B][H][D] bf16            softmax(q K^^T / sqrt D) V^ over the keys 0 .. lens[b], rounded once
//
// A row with 0 <= lens[b] < Lmax quantizes the new k and v, stores codes and exponents at cache row
// lens[b] and attends over the lens[b] cached keys plus the new one - its dequantized value, taken
// from registers and never re-read, so "append, then attend over the cache" is one definition
// whatever the step.  Any other lens[b]: nothing is stored, codes and exponents included, and the
// out row is zeros.  Rows at or beyond lens[b] are never loaded, whatever they hold.
//
// Structure: attn_decode.hip's (K-M18) - one workgroup of 4 waves per (b, h), fp32 online softmax in
// the exp2 domain, two register sets in ping-pong, lane groups merged by shuffles and the waves
// through LDS, one writer per element, no atomics, bitwise reproducible.  Lane mapping: D / 8 lanes
// own a key row in 8-byte loads, so a wave load covers KPW = 512 / D whole keys (512 contiguous
// bytes) and a lane's slice is the 8 elements it has in K-M18: AdState, the merges and the epilogue
// are that kernel's.  16-byte loads would halve the load count but give a lane 16 elements of o (24
// more live VGPRs) and half as many keys per wave iteration for the same bytes in flight; with the
// exponent bytes there are 4 loads per key and lane either way.  The exponents cost no multiply
// per element: the dot product is scaled once per key by 2^e_k (v_ldexp_f32, exact) and 2^e_v goes
// into the probability in front of the PV accumulation.  Where e_v lies near -127 - a V row whose
// values are themselves below about 2^-118 - that product is an fp32 subnormal and loses bits of p.
#include <math.h>

#include "attn_decode.h"
#include "common.h"
#include "launchers.h"

namespace dpa {

// ---- the format ---------------------------------------------------------------------------------

// the largest |bf16| of 8 packed values, as its 15 magnitude bits (integer order = value order)
__device__ __forceinline__ uint32_t kv8_amax8(const uint4 r) {
  uint32_t m = 0u;
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) m = max(m, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));
  return m;
}

// the row exponent from the magnitude bits of its largest element: a normal a = 1.f 2^(E - 127) has
// frexp (1.f / 2, E - 126), and m > 0.875 is f > 0x60; a bf16 subnormal lies below the clamp
__device__ __forceinline__ int kv8_exp(const uint32_t amax) {
  const int E = (int)(amax >> 7), f = (int)(amax & 0x7fu);
  return amax == 0u ? 0 : max(E - 135 + (f > 0x60 ? 1 : 0), -127);
}

// 8 bf16 -> 8 codes of x 2^-e; 2^-e = 2^-120 .. 2^127 is a normal fp32
__device__ __forceinline__ uint2 kv8_quant8(const uint4 raw, const int e) {
  float f[8];
  ad_unpack8(raw, f);
  const float sc = __uint_as_float((uint32_t)(127 - e) << 23);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * sc, f[1] * sc, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * sc, f[3] * sc, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * sc, f[5] * sc, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * sc, f[7] * sc, hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

__device__ __forceinline__ void kv8_unpack8(const uint2 r, float f[8]) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)r.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)r.x, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)r.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)r.y, true);
  f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
  f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
}

// the exponent of the row whose slices the G lanes of a group hold (every lane gets it)
template <int G>
__device__ __forceinline__ int kv8_row_exp(const uint4 raw) {
  uint32_t m = kv8_amax8(raw);
#pragma unroll
  for (int off = G >> 1; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
  return kv8_exp(m);
}

// ---- the quantizing store -------------------------------------------------------------------------
// Row r = ((b L + l) NW + w) H + h of the source: D bf16 at src + b * s_b + l * s_l + ((first + w) H + h) D,
// stored - where l < lens[b], or everywhere without lens - as codes at dst_w + b * sb + h * sh + l * D
// and exponent at exp_w + b * esb + h * esh + l.  D / 8 lanes per row, 16-byte loads, 8-byte stores.
struct Kv8Dst {
  uint8_t* codes;
  int8_t* exps;
  int64_t sb, sh, esb, esh;
};

template <int D>
__global__ void __launch_bounds__(256) kv8_store_kernel(const bf16_t* __restrict__ src, int64_t s_b, int64_t s_l,
                                                         int first, int NW, int L, int H,
                                                         const int* __restrict__ lens, Kv8Dst d0, Kv8Dst d1,
                                                         int64_t rows) {
  constexpr int G = D / 8;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / G;
  const int c = (int)(t - row * G);
  const bool inside = row < rows;
  const int64_t r = inside ? row : rows - 1;  // a whole lane group is inside or not: G divides 256
  const int h = (int)(r % H);
  const int w = (int)(r / H % NW);
  const int l = (int)(r / H / NW % L);
  const int64_t b = r / H / NW / L;
  const bool live = inside && (!lens || l < lens[b]);
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  if (live) raw = *reinterpret_cast<const uint4*>(src + b * s_b + (int64_t)l * s_l + ((int64_t)(first + w) * H + h) * D + c * 8);
  const int e = kv8_row_exp<G>(raw);
  if (live) {
    const Kv8Dst d = w == 0 ? d0 : d1;
    *reinterpret_cast<uint2*>(d.codes + b * d.sb + (int64_t)h * d.sh + (int64_t)l * D + c * 8) = kv8_quant8(raw, e);
    if (c == 0) d.exps[b * d.esb + (int64_t)h * d.esh + l] = (int8_t)e;
  }
}

// ---- the decode step ------------------------------------------------------------------------------

// q . code over the G lanes of a group (every lane of the group gets the sum)
template <int G>
__device__ __forceinline__ float ad8_dot(const float q[8], const uint2 kr) {
  float kf[8];
  kv8_unpack8(kr, kf);
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
#pragma unroll
  for (int off = G >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
  return d;
}

// ad_update over code rows: 2^ev[u] goes into the probability in front of the PV sum
template <int N>
__device__ __forceinline__ void ad8_update(AdState& st, const float s[N], const uint2 vr[N], const int ev[N]) {
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
    kv8_unpack8(vr[u], vf);
    st.l += p;
    const float pv = ldexpf(p, ev[u]);
#pragma unroll
    for (int i = 0; i < 8; ++i) st.o[i] = fmaf(pv, vf[i], st.o[i]);
  }
  st.m = mn;
}

template <int D>
__global__ void __launch_bounds__(64 * AD_WAVES) attn_decode_fp8_kernel(
    const bf16_t* __restrict__ qkv, int64_t qkv_stride, uint8_t* __restrict__ k8, int8_t* __restrict__ ke,
    uint8_t* __restrict__ v8, int8_t* __restrict__ ve, int64_t k_sb, int64_t k_sh, int64_t ke_sb, int64_t ke_sh,
    int64_t v_sb, int64_t v_sh, int64_t ve_sb, int64_t ve_sh, const int* __restrict__ lens, int H, int Lmax,
    bf16_t* __restrict__ out) {
  constexpr int G = D / 8;               // lanes per key row
  constexpr int KPW = 64 / G;            // keys per wave load
  constexpr int U = AD_U;
  constexpr int WK = U * KPW;            // keys per wave per iteration
  constexpr int IT = AD_WAVES * WK;      // keys per workgroup iteration
  __shared__ float sm_o[AD_WAVES][D];
  __shared__ float sm_ml[AD_WAVES][2];

  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane / G, c = lane - g * G;
  const int n = lens[b];  // cached keys; the new one becomes key n
  bf16_t* orow = out + ((int64_t)b * H + h) * D;
  if (n < 0 || n >= Lmax) {  // inactive row (uniform over the workgroup)
    if (tid < D / 2) reinterpret_cast<uint32_t*>(orow)[tid] = 0u;
    return;
  }

  const bf16_t* qrow = qkv + (int64_t)b * qkv_stride + (int64_t)h * D + c * 8;
  const uint4 qraw = *reinterpret_cast<const uint4*>(qrow);
  const uint4 kraw = *reinterpret_cast<const uint4*>(qrow + (int64_t)H * D);
  const uint4 vraw = *reinterpret_cast<const uint4*>(qrow + 2 * (int64_t)H * D);
  const uint8_t* kb = k8 + (int64_t)b * k_sb + (int64_t)h * k_sh + c * 8;
  const uint8_t* vb = v8 + (int64_t)b * v_sb + (int64_t)h * v_sh + c * 8;
  const int8_t* keb = ke + (int64_t)b * ke_sb + (int64_t)h * ke_sh;
  const int8_t* veb = ve + (int64_t)b * ve_sb + (int64_t)h * ve_sh;
  // the new row, quantized: every lane group holds all of it
  const int ek_new = kv8_row_exp<G>(kraw), ev_new = kv8_row_exp<G>(vraw);
  const uint2 knew = kv8_quant8(kraw, ek_new), vnew = kv8_quant8(vraw, ev_new);
  if (wave == 0 && g == 0) {  // the append: n < Lmax
    *reinterpret_cast<uint2*>(k8 + (int64_t)b * k_sb + (int64_t)h * k_sh + (int64_t)n * D + c * 8) = knew;
    *reinterpret_cast<uint2*>(v8 + (int64_t)b * v_sb + (int64_t)h * v_sh + (int64_t)n * D + c * 8) = vnew;
    if (c == 0) {
      ke[(int64_t)b * ke_sb + (int64_t)h * ke_sh + n] = (int8_t)ek_new;
      ve[(int64_t)b * ve_sb + (int64_t)h * ve_sh + n] = (int8_t)ev_new;
    }
  }

  float q[8];
  ad_unpack8(qraw, q);
  constexpr float qscale = (D == 64 ? 0.125f : 0.08838834764831845f) * LOG2E;  // 1 / sqrt D, exp2 domain
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] *= qscale;

  AdState st;
  st.m = -INFINITY;
  st.l = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) st.o[i] = 0.f;

  // keys base + u * KPW + g, u < U, of this wave; rows >= n are not loaded
  auto load = [&](int base, uint2 kr[U], uint2 vr[U], int ek[U], int ev[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * KPW + g;
      kr[u] = make_uint2(0u, 0u);
      vr[u] = make_uint2(0u, 0u);
      ek[u] = 0;
      ev[u] = 0;
      if (key < n) {
        kr[u] = *reinterpret_cast<const uint2*>(kb + (int64_t)key * D);
        vr[u] = *reinterpret_cast<const uint2*>(vb + (int64_t)key * D);
        ek[u] = keb[key];
        ev[u] = veb[key];
      }
    }
  };
  auto fold = [&](int base, const uint2 kr[U], const uint2 vr[U], const int ek[U], const int ev[U]) {
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float d = ldexpf(ad8_dot<G>(q, kr[u]), ek[u]);
      s[u] = (base + u * KPW + g < n) ? d : -INFINITY;
    }
    ad8_update<U>(st, s, vr, ev);
  };

  int base = wave * WK;  // wave-uniform, as is every branch on it
  if (base < n) {
    uint2 ka[U], va[U], kb2[U], vb2[U];
    int eka[U], eva[U], ekb[U], evb[U];
    load(base, ka, va, eka, eva);
    for (;;) {
      if (base + IT < n) load(base + IT, kb2, vb2, ekb, evb);
      fold(base, ka, va, eka, eva);
      base += IT;
      if (base >= n) break;
      if (base + IT < n) load(base + IT, ka, va, eka, eva);
      fold(base, kb2, vb2, ekb, evb);
      base += IT;
      if (base >= n) break;
    }
  }

  {  // the new key, dequantized from registers: group 0 of wave 0 takes it
    const float d = ldexpf(ad8_dot<G>(q, knew), ek_new);
    const float s[1] = {(wave == 0 && g == 0) ? d : -INFINITY};
    const uint2 v1[1] = {vnew};
    const int e1[1] = {ev_new};
    ad8_update<1>(st, s, v1, e1);
  }

  // merge the wave's lane groups (same d slice, different keys)
#pragma unroll
  for (int off = G; off < 64; off <<= 1) {
    const float m2 = __shfl_xor(st.m, off, 64), l2 = __shfl_xor(st.l, off, 64);
    const float mn = fmaxf(st.m, m2);
    const float ms = mn == -INFINITY ? 0.f : mn;
    const float a1 = fexp2(st.m - ms), a2 = fexp2(m2 - ms);
    st.l = st.l * a1 + l2 * a2;
#pragma unroll
    for (int i = 0; i < 8; ++i) st.o[i] = st.o[i] * a1 + __shfl_xor(st.o[i], off, 64) * a2;
    st.m = mn;
  }
  if (g == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) sm_o[wave][c * 8 + i] = st.o[i];
    if (c == 0) {
      sm_ml[wave][0] = st.m;
      sm_ml[wave][1] = st.l;
    }
  }
  __syncthreads();
  if (tid < D / 2) {  // wave 0 holds the new key, so the maximum is finite
    float mx = sm_ml[0][0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) mx = fmaxf(mx, sm_ml[w][0]);
    float l = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) {
      const float a = fexp2(sm_ml[w][0] - mx);
      l = fmaf(sm_ml[w][1], a, l);
      o0 = fmaf(sm_o[w][2 * tid], a, o0);
      o1 = fmaf(sm_o[w][2 * tid + 1], a, o1);
    }
    reinterpret_cast<uint32_t*>(orow)[tid] = pack_bf2(o0 / l, o1 / l);
  }
}

// ---- launchers ------------------------------------------------------------------------------------

static inline bool kv8_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static inline bool kv8_cache_ok(const uint8_t* codes, const int8_t* exps, int64_t sb, int64_t sh) {
  // 16-byte rows: every code row starts a multiple of 16 bytes from a 16-byte aligned base
  return codes && exps && kv8_aligned(codes) && sb % 16 == 0 && sh % 16 == 0;
}

bool launch_attn_decode_fp8(const uint16_t* qkv_new, int64_t qkv_stride, uint8_t* k8, int8_t* ke, uint8_t* v8,
                            int8_t* ve, int64_t k_sb, int64_t k_sh, int64_t ke_sb, int64_t ke_sh, int64_t v_sb,
                            int64_t v_sh, int64_t ve_sb, int64_t ve_sh, const int* lens, int B, int H, int Lmax, int D,
                            uint16_t* out, hipStream_t s) {
  if ((D != 64 && D != 128) || B <= 0 || H <= 0 || Lmax <= 0 || (int64_t)B * H > 0x7fffffffLL) return false;
  if (!qkv_new || !lens || !out || !kv8_aligned(qkv_new) || qkv_stride % 8) return false;
  if (!kv8_cache_ok(k8, ke, k_sb, k_sh) || !kv8_cache_ok(v8, ve, v_sb, v_sh)) return false;
  const dim3 grid((unsigned)(B * H)), block(64 * AD_WAVES);
  if (D == 64)
    hipLaunchKernelGGL((attn_decode_fp8_kernel<64>), grid, block, 0, s, qkv_new, qkv_stride, k8, ke, v8, ve, k_sb,
                       k_sh, ke_sb, ke_sh, v_sb, v_sh, ve_sb, ve_sh, lens, H, Lmax, out);
  else
    hipLaunchKernelGGL((attn_decode_fp8_kernel<128>), grid, block, 0, s, qkv_new, qkv_stride, k8, ke, v8, ve, k_sb,
                       k_sh, ke_sb, ke_sh, v_sb, v_sh, ve_sb, ve_sh, lens, H, Lmax, out);
  return true;
}

static bool kv8_launch_store(const uint16_t* src, int64_t s_b, int64_t s_l, int first, int NW, int64_t B, int L, int H,
                             int D, const int* lens, const Kv8Dst& d0, const Kv8Dst& d1, hipStream_t s) {
  const int64_t rows = B * L * NW * H;
  const int64_t blocks = (rows * (D / 8) + 255) / 256;
  if (blocks > 0x7fffffffLL) return false;
  const dim3 grid((unsigned)blocks), block(256);
  if (D == 64)
    hipLaunchKernelGGL((kv8_store_kernel<64>), grid, block, 0, s, src, s_b, s_l, first, NW, L, H, lens, d0, d1, rows);
  else
    hipLaunchKernelGGL((kv8_store_kernel<128>), grid, block, 0, s, src, s_b, s_l, first, NW, L, H, lens, d0, d1, rows);
  return true;
}

bool launch_kv8_store(const uint16_t* qkv, int64_t qkv_sb, int64_t qkv_sl, const int* lens, uint8_t* k8, int8_t* ke,
                      uint8_t* v8, int8_t* ve, int64_t k_sb, int64_t k_sh, int64_t ke_sb, int64_t ke_sh, int64_t v_sb,
                      int64_t v_sh, int64_t ve_sb, int64_t ve_sh, int B, int L, int H, int Lmax, int D, hipStream_t s) {
  if ((D != 64 && D != 128) || B <= 0 || L <= 0 || H <= 0 || L > Lmax) return false;  // position l < L goes to cache row l
  if (!qkv || !lens || !kv8_aligned(qkv) || qkv_sb % 8 || qkv_sl % 8) return false;
  if (!kv8_cache_ok(k8, ke, k_sb, k_sh) || !kv8_cache_ok(v8, ve, v_sb, v_sh)) return false;
  return kv8_launch_store(qkv, qkv_sb, qkv_sl, 1, 2, B, L, H, D, lens, Kv8Dst{k8, ke, k_sb, k_sh, ke_sb, ke_sh},
                          Kv8Dst{v8, ve, v_sb, v_sh, ve_sb, ve_sh}, s);
}

bool launch_kv8_quantize(const uint16_t* x, int64_t rows, int D, uint8_t* codes, int8_t* exps, hipStream_t s) {
  if ((D != 64 && D != 128) || rows <= 0 || !x || !codes || !exps || !kv8_aligned(x) || !kv8_aligned(codes))
    return false;
  const Kv8Dst d{codes, exps, (int64_t)D, 0, 1, 0};
  return kv8_launch_store(x, D, 0, 0, 1, rows, 1, 1, D, nullptr, d, d, s);
}

}  // namespace dpa
