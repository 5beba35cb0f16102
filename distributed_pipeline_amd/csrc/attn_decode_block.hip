// GPT-2 generation: the KV-cache append and the attention of a block of T new tokens per row as one
// kernel, in one pass over K and V (lookahead decoding: a committed token and T - 1 guessed ones).
//
//   qkv_new [B][T][3][H][D] bf16  the block's packed projections (row b, token j at b * sb + j * st)
//   k_cache / v_cache             bf16 rows of D at (b, h, key): base + b * sb + h * sh + key * D
//   lens [B] int32                keys already cached per row, before the call (not modified)
//   counts [B] int32 or null      tokens of the block that are real, per row (null: T)
//   out [B][T][H][D] bf16
//
// With c_b = 0 for an inactive row (lens[b] outside [0, Lmax)) and otherwise
// c_b = clamp(counts[b], 0, min(T, Lmax - lens[b])), the call is T successive calls of
// attn_decode.hip, call j on token j with lens_j[b] = lens[b] + j if j < c_b and -1 otherwise: query
// j < c_b stores its k and v (the bits of qkv_new) at cache row lens[b] + j and attends over the keys
// 0 .. lens[b] + j; query j >= c_b stores nothing and returns zeros.  Cache rows at or beyond
// lens[b] + c_b are neither loaded nor stored.
//
// The structure is the plain kernel's - one workgroup of 4 waves per (b, h), D / 8 lanes per key row
// in 16-byte loads, U = 4 wave loads of K and of V per register set, two sets, ping-pong - with T
// online-softmax states per lane group: each K/V register set is loaded once and folded into the
// states of all the queries it is a key of.  Fold order per query is the plain kernel's for lens + j:
// a key goes to the (wave, lane group, iteration) its position gives it there, and the query's own
// key is folded last, by group 0 of wave 0.  The keys of the block that lie before a query
// (positions lens .. lens + j - 1) are folded at their positions like cached ones, but loaded from
// qkv_new, whose bits they are: the workgroup never reads back its own stores, so no ordering of
// them matters.  A wave iteration that lies wholly below lens is a key of every query and needs no
// mask; one that reaches into the block masks per query, scores and V alike, so that what a later
// query's keys hold never reaches an earlier one.
//
// TT is the instantiation (2, 4, 8); T <= TT is the block's real length, and the queries j >= T are
// handled as inactive ones whose rows of qkv_new and out do not exist.
#include <math.h>

#include "attn_decode.h"
#include "common.h"
#include "launchers.h"

namespace dpa {

template <int D, int TT>
__global__ void __launch_bounds__(64 * AD_WAVES) attn_decode_block_kernel(
    const bf16_t* __restrict__ qkv, int64_t qkv_sb, int64_t qkv_st, bf16_t* __restrict__ kc,
    bf16_t* __restrict__ vc, int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* __restrict__ lens,
    const int* __restrict__ counts, int T, int H, int Lmax, bf16_t* __restrict__ out) {
  constexpr int G = D / 8;               // lanes per key row
  constexpr int KPW = 64 / G;            // keys per wave load
  constexpr int U = AD_U;
  constexpr int WK = U * KPW;            // keys per wave per iteration
  constexpr int IT = AD_WAVES * WK;      // keys per workgroup iteration
  constexpr int NT = 64 * AD_WAVES;
  __shared__ float sm_o[TT][AD_WAVES][D];
  __shared__ float sm_ml[TT][AD_WAVES][2];

  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane / G, c = lane - g * G;
  const int n = lens[b];  // cached keys; token j becomes key n + j
  int cnt = 0;            // c_b: the queries j < cnt are active (uniform over the workgroup)
  if (n >= 0 && n < Lmax) cnt = max(0, min(counts ? counts[b] : T, min(T, Lmax - n)));
  bf16_t* orow = out + ((int64_t)b * T * H + h) * D;  // query j: + j * H * D
  const int64_t o_st = (int64_t)H * D;
  if (cnt == 0) {
    for (int i = tid; i < T * (D / 2); i += NT)
      reinterpret_cast<uint32_t*>(orow + (i / (D / 2)) * o_st)[i % (D / 2)] = 0u;
    return;
  }

  // token j's q; its k and v stand H D and 2 H D elements behind
  const bf16_t* qrow = qkv + (int64_t)b * qkv_sb + (int64_t)h * D + c * 8;
  const bf16_t* knew = qrow + (int64_t)H * D;
  const bf16_t* vnew = qrow + 2 * (int64_t)H * D;
  const bf16_t* kb = kc + (int64_t)b * k_sb + (int64_t)h * k_sh + c * 8;
  const bf16_t* vb = vc + (int64_t)b * v_sb + (int64_t)h * v_sh + c * 8;
  // the appends: rows n .. n + cnt - 1 < Lmax, token j by group 0 of wave j mod 4
#pragma unroll
  for (int j = 0; j < TT; ++j)
    if (j < cnt && wave == (j & (AD_WAVES - 1)) && g == 0) {
      *reinterpret_cast<uint4*>(kc + (int64_t)b * k_sb + (int64_t)h * k_sh + (int64_t)(n + j) * D + c * 8) =
          *reinterpret_cast<const uint4*>(knew + j * qkv_st);
      *reinterpret_cast<uint4*>(vc + (int64_t)b * v_sb + (int64_t)h * v_sh + (int64_t)(n + j) * D + c * 8) =
          *reinterpret_cast<const uint4*>(vnew + j * qkv_st);
    }

  constexpr float qscale = (D == 64 ? 0.125f : 0.08838834764831845f) * LOG2E;  // 1 / sqrt D, exp2 domain
  float q[TT][8];
  AdState st[TT];
#pragma unroll
  for (int j = 0; j < TT; ++j) {
    uint4 qraw = make_uint4(0u, 0u, 0u, 0u);
    if (j < cnt) qraw = *reinterpret_cast<const uint4*>(qrow + j * qkv_st);
    ad_unpack8(qraw, q[j]);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[j][i] *= qscale;
    st[j].m = -INFINITY;
    st[j].l = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) st[j].o[i] = 0.f;
  }

  // The last active query has nl cached keys: the n of the cache and the block's first cnt - 1.
  const int nl = n + cnt - 1;
  // keys base + u * KPW + g, u < U, of this wave: below n from the cache, below nl from qkv_new;
  // rows >= nl are not loaded
  auto load = [&](int base, uint4 kr[U], uint4 vr[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * KPW + g;
      kr[u] = make_uint4(0u, 0u, 0u, 0u);
      vr[u] = make_uint4(0u, 0u, 0u, 0u);
      if (key < nl) {
        const bf16_t* kp = key < n ? kb + (int64_t)key * D : knew + (int64_t)(key - n) * qkv_st;
        const bf16_t* vp = key < n ? vb + (int64_t)key * D : vnew + (int64_t)(key - n) * qkv_st;
        kr[u] = *reinterpret_cast<const uint4*>(kp);
        vr[u] = *reinterpret_cast<const uint4*>(vp);
      }
    }
  };
  // Query j folds the iteration at `base` iff the plain kernel would with n + j cached keys.
  auto fold = [&](int base, const uint4 kr[U], const uint4 vr[U]) {
    if (base + WK <= n) {  // every key of the wave's iteration is cached: a key of every query
#pragma unroll
      for (int j = 0; j < TT; ++j)
        if (j < cnt) {
          float s[U];
#pragma unroll
          for (int u = 0; u < U; ++u) s[u] = ad_dot<G>(q[j], kr[u]);
          ad_update<U>(st[j], s, vr);
        }
    } else {
#pragma unroll
      for (int j = 0; j < TT; ++j)
        if (j < cnt && base < n + j) {
          float s[U];
          uint4 vm[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool is_key = base + u * KPW + g < n + j;
            const float d = ad_dot<G>(q[j], kr[u]);
            s[u] = is_key ? d : -INFINITY;
            vm[u] = is_key ? vr[u] : make_uint4(0u, 0u, 0u, 0u);
          }
          ad_update<U>(st[j], s, vm);
        }
    }
  };

  int base = wave * WK;  // wave-uniform, as is every branch on it
  if (base < nl) {
    uint4 ka[U], va[U], kb2[U], vb2[U];
    load(base, ka, va);
    for (;;) {
      if (base + IT < nl) load(base + IT, kb2, vb2);
      fold(base, ka, va);
      base += IT;
      if (base >= nl) break;
      if (base + IT < nl) load(base + IT, ka, va);
      fold(base, kb2, vb2);
      base += IT;
      if (base >= nl) break;
    }
  }

#pragma unroll
  for (int j = 0; j < TT; ++j) {
    if (j >= cnt) continue;
    AdState& sj = st[j];
    {  // the query's own key: group 0 of wave 0 takes it
      const uint4 kn = *reinterpret_cast<const uint4*>(knew + j * qkv_st);
      const uint4 vn = *reinterpret_cast<const uint4*>(vnew + j * qkv_st);
      const float d = ad_dot<G>(q[j], kn);
      const float s[1] = {(wave == 0 && g == 0) ? d : -INFINITY};
      const uint4 v1[1] = {vn};
      ad_update<1>(sj, s, v1);
    }
    // merge the wave's lane groups (same d slice, different keys)
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
      const float m2 = __shfl_xor(sj.m, off, 64), l2 = __shfl_xor(sj.l, off, 64);
      const float mn = fmaxf(sj.m, m2);
      const float ms = mn == -INFINITY ? 0.f : mn;
      const float a1 = fexp2(sj.m - ms), a2 = fexp2(m2 - ms);
      sj.l = sj.l * a1 + l2 * a2;
#pragma unroll
      for (int i = 0; i < 8; ++i) sj.o[i] = sj.o[i] * a1 + __shfl_xor(sj.o[i], off, 64) * a2;
      sj.m = mn;
    }
    if (g == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_o[j][wave][c * 8 + i] = sj.o[i];
      if (c == 0) {
        sm_ml[j][wave][0] = sj.m;
        sm_ml[j][wave][1] = sj.l;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < T * (D / 2); i += NT) {
    const int j = i / (D / 2), t = i - j * (D / 2);
    uint32_t r = 0u;
    if (j < cnt) {  // wave 0 holds the query's own key, so the maximum is finite
      float mx = sm_ml[j][0][0];
#pragma unroll
      for (int w = 1; w < AD_WAVES; ++w) mx = fmaxf(mx, sm_ml[j][w][0]);
      float l = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
      for (int w = 0; w < AD_WAVES; ++w) {
        const float a = fexp2(sm_ml[j][w][0] - mx);
        l = fmaf(sm_ml[j][w][1], a, l);
        o0 = fmaf(sm_o[j][w][2 * t], a, o0);
        o1 = fmaf(sm_o[j][w][2 * t + 1], a, o1);
      }
      r = pack_bf2(o0 / l, o1 / l);
    }
    reinterpret_cast<uint32_t*>(orow + j * o_st)[t] = r;
  }
}

template <int D, int TT>
static void adb_launch(const uint16_t* qkv_new, int64_t qkv_sb, int64_t qkv_st, uint16_t* k_cache, uint16_t* v_cache,
                       int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* lens, const int* counts,
                       int B, int T, int H, int Lmax, uint16_t* out, hipStream_t s) {
  const dim3 grid((unsigned)(B * H)), block(64 * AD_WAVES);
  hipLaunchKernelGGL((attn_decode_block_kernel<D, TT>), grid, block, 0, s, qkv_new, qkv_sb, qkv_st, k_cache, v_cache,
                     k_sb, k_sh, v_sb, v_sh, lens, counts, T, H, Lmax, out);
}

bool launch_attn_decode_block(const uint16_t* qkv_new, int64_t qkv_sb, int64_t qkv_st, uint16_t* k_cache,
                              uint16_t* v_cache, int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh,
                              const int* lens, const int* counts, int B, int T, int H, int Lmax, int D,
                              uint16_t* out, hipStream_t s) {
  if (T < 1 || T > 8 || qkv_st % 8) return false;
  if (!ad_args_ok(qkv_new, qkv_sb, k_cache, v_cache, k_sb, k_sh, v_sb, v_sh, lens, B, H, Lmax, D, out))
    return false;
  if (T == 1 && !counts)  // the plain kernel itself: out [B][1][H][D] is its [B][H][D]
    return launch_attn_decode(qkv_new, qkv_sb, k_cache, v_cache, k_sb, k_sh, v_sb, v_sh, lens, B, H, Lmax, D, out, s);
#define ADB_GO(DD, TT_) \
  adb_launch<DD, TT_>(qkv_new, qkv_sb, qkv_st, k_cache, v_cache, k_sb, k_sh, v_sb, v_sh, lens, counts, B, T, H, Lmax, out, s)
  if (D == 64) {
    if (T <= 2) ADB_GO(64, 2); else if (T <= 4) ADB_GO(64, 4); else ADB_GO(64, 8);
  } else {
    if (T <= 2) ADB_GO(128, 2); else if (T <= 4) ADB_GO(128, 4); else ADB_GO(128, 8);
  }
#undef ADB_GO
  return true;
}

}  // namespace dpa
