// K-M28.  GPT-2 generation, parallel sampling: one decode step of R = B G rows, where the G rows of a
// group continue one prompt.  The prompt's keys are held once per group (the prefix cache) and every row
// has a cache of its own for what it has generated since (the suffix cache):
//
//   qkv_new [R][3][H][D] bf16     the rows' packed projections (row r at r * qkv_sb)
//   kp / vp                       prefix: bf16 rows of D at (b, h, key): base + b * sb + h * sh + key * D
//   plens [B] int32               prefix keys per group (not modified)
//   ks / vs                       suffix: rows of D at (r, h, key), r = b G + g
//   slens [R] int32               suffix keys per row, before the call (not modified)
//   out [R][H][D] bf16
//
// Row r = b G + g is active iff 0 <= slens[r] < Ls and 0 <= plens[b] <= Lp.  An active row stores the bits
// of its k and v at suffix row slens[r] and returns softmax(q K^T / sqrt D) V over the prefix keys
// 0 .. plens[b] - 1, its suffix keys 0 .. slens[r] - 1 and its new key, which is taken from qkv_new and
// never read back.  An inactive row stores nothing and returns zeros.  The prefix is never written;
// prefix rows at or beyond plens[b] and suffix rows at or beyond slens[r] are never loaded.
//
// Work split.  One workgroup of 4 waves per (b, h, slice of QS consecutive queries of the group), QS in
// {4, 8, 16, 32}: the slice's queries are the B columns of S^T = K Q^T on v_mfma_f32_32x32x16_bf16, so
// a prefix key is loaded once per slice and meets up to 32 queries.  Every slice of a (b, h) reads the
// prefix again, which is what QS trades against the number of workgroups (the launcher's rule: the
// largest QS that still fills the chip).  The tile routine - K fragments of 16 contiguous bytes straight
// from global memory on a clamped key, masked weights, a lane per query column with max and sum per
// lane plus one exchange between the lane halves, P rounded to bf16 once, O^T += V^T P^T on the same
// MFMA with V through a swizzled wave-private LDS tile, two stages of K and V registers, the scale
// 1 / sqrt D * log2 e inside the exponent's FMA - is attn_extend.hip's (K-M27), whose header explains it.
//
// Three kinds of 32-key tile go through that routine:
//   prefix   keys 32 i .. of (b, h); every column keeps every key.  Only the tile that holds key
//            plens[b] - 1 runs a mask.  A column without an active query has q = 0: its weights are
//            finite and its state is thrown away at the store.
//   suffix   keys 32 i .. of one row's own cache; only that row's column keeps them, every other column
//            is masked to weight 0.  The MFMA columns this wastes cost nothing next to the loads.
//   new      key j is the new key of the slice's query j, from qkv_new; column j keeps key j alone.  An
//            inactive query's row is replaced by the first active one's (masked), so nothing a parked row
//            holds reaches a product.
//
// Deviation from a plain round-robin over one tile list: the bits of a row must not depend on QS or on
// the other rows of its slice, so the wave that folds a tile, and the order of a column's tiles inside
// that wave, are functions of the row alone.  With np = ceil(plens[b] / 32): prefix tile i goes to wave
// i % 4; suffix tile i of group member g goes to wave (np + 1 + g + i) % 4, so the rows' tiles spread over
// the waves behind the prefix; the new tile goes to wave np % 4, the one the next prefix tile would have
// gone to.  A wave runs its prefix tiles, then its suffix tiles in query order, then the new tile.  A
// tile of another row is an exact no-op on a column (alpha = 1, weights 0), so a column sees its own
// tiles in the same waves and the same order whatever else the slice holds.  (QS is a multiple of 4,
// so g % 4 is the query's place in the slice % 4.)
//
// Merge and stores: as K-M27 - the waves add their scaled O^T into one [32][D] fp32 LDS image in wave
// order, a barrier apart, one writer per output element; the appends are 16-byte stores by the
// workgroup that owns the query.  No atomics, no workspace: two calls agree bit for bit.
#include <math.h>

#include "attn_decode.h"
#include "common.h"
#include "launchers.h"
#include "mfma.h"

namespace dpa {

constexpr int AG_KT = 32;     // keys per wave tile
constexpr int AG_QMAX = 32;   // queries per workgroup at most (the MFMA's columns)

// a wave's place in its tile list: kind 0 prefix tile i, 1 suffix tile i of query q, 2 the new tile, 3 end
struct AgCur {
  int kind, q, i;
};

template <int D>
__global__ void __launch_bounds__(64 * AD_WAVES) attn_decode_grouped_kernel(
    const bf16_t* __restrict__ qkv, int64_t qkv_sb, const bf16_t* __restrict__ kp, const bf16_t* __restrict__ vp,
    int64_t kp_sb, int64_t kp_sh, int64_t vp_sb, int64_t vp_sh, const int* __restrict__ plens, int Lp,
    bf16_t* __restrict__ ks, bf16_t* __restrict__ vs, int64_t ks_sb, int64_t ks_sh, int64_t vs_sb, int64_t vs_sh,
    const int* __restrict__ slens, int Ls, int G, int H, int QS, int NSL, bf16_t* __restrict__ out) {
  constexpr int CH = D / 8;               // 16-byte chunks per row
  constexpr int VU = AG_KT * CH / 64;     // chunks of a V tile per lane
  constexpr int KS = D / 16;              // k-steps of S
  constexpr int ND = D / 32;              // 32-row tiles of O^T
  constexpr int NT = 64 * AD_WAVES;
  constexpr int VBYTES = AG_KT * 2 * D;   // a wave's V tile
  constexpr int OP = D + 4;               // floats per query in the merge buffer (padded against bank conflicts)
  constexpr int MBYTES = AG_QMAX * OP * 4;
  // the V tiles while the waves stream, the merge image afterwards
  __shared__ __attribute__((aligned(16))) char smem[MBYTES > AD_WAVES * VBYTES ? MBYTES : AD_WAVES * VBYTES];
  __shared__ float sm_ml[AD_WAVES][AG_QMAX][2];
  __shared__ int sm_sl[AG_QMAX];  // suffix keys of the slice's queries, 0 for an inactive one

  const int sl = blockIdx.x % NSL, bh = blockIdx.x / NSL;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int g0 = sl * QS;
  const int nq = min(QS, G - g0);             // the slice's queries (>= 1 by the grid)
  const int64_t row0 = (int64_t)b * G + g0;   // query j of the slice is row row0 + j
  const int pl = plens[b];
  const bool pok = pl >= 0 && pl <= Lp;
  // this lane's query column (both lane halves hold it)
  const int myn = r < nq ? slens[row0 + r] : -1;
  const bool act = pok && myn >= 0 && myn < Ls;
  const uint32_t amask = (uint32_t)__ballot(act);  // lanes 0 .. 31: the slice's active queries (uniform)
  bf16_t* orow = out + (row0 * H + h) * D;         // query j: + j * H * D
  const int64_t o_st = (int64_t)H * D;
  if (amask == 0u) {
    for (int i = tid; i < nq * (D / 2); i += NT)
      reinterpret_cast<uint32_t*>(orow + (i / (D / 2)) * o_st)[i % (D / 2)] = 0u;
    return;
  }
  const int qfirst = __ffs(amask) - 1;
  if (tid < AG_QMAX) sm_sl[tid] = act ? myn : 0;

  // query j's q; its k and v stand H D and 2 H D elements behind
  const bf16_t* qnew = qkv + row0 * qkv_sb + (int64_t)h * D;
  const bf16_t* knew = qnew + (int64_t)H * D;
  const bf16_t* vnew = qnew + 2 * (int64_t)H * D;
  const bf16_t* kpb = kp + (int64_t)b * kp_sb + (int64_t)h * kp_sh;
  const bf16_t* vpb = vp + (int64_t)b * vp_sb + (int64_t)h * vp_sh;
  bf16_t* ksb = ks + row0 * ks_sb + (int64_t)h * ks_sh;  // query j: + j * ks_sb
  bf16_t* vsb = vs + row0 * vs_sb + (int64_t)h * vs_sh;
  // the appends: suffix row slens < Ls of every active query of the slice
  for (int i = tid; i < nq * CH; i += NT) {
    const int j = i / CH, c = i - j * CH;
    if ((amask >> j) & 1u) {
      const int at = slens[row0 + j];
      *reinterpret_cast<uint4*>(ksb + j * ks_sb + (int64_t)at * D + c * 8) =
          *reinterpret_cast<const uint4*>(knew + j * qkv_sb + c * 8);
      *reinterpret_cast<uint4*>(vsb + j * vs_sb + (int64_t)at * D + c * 8) =
          *reinterpret_cast<const uint4*>(vnew + j * qkv_sb + c * 8);
    }
  }
  __syncthreads();  // sm_sl

  bf16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    qf[s] = __builtin_bit_cast(bf16x8, (u32x4){0u, 0u, 0u, 0u});
    if (act) qf[s] = ld_frag(qnew + r * qkv_sb + 16 * s + 8 * hf);
  }

  // this wave's tile list (header): everything below is wave-uniform
  const int np = (pl + AG_KT - 1) / AG_KT;
  const int nst = (act ? myn + AG_KT - 1 : 0) / AG_KT;  // suffix tiles of this lane's query
  const uint32_t smask = (uint32_t)__ballot(((wave - r - np - 1) & 3) < nst);  // queries with a tile in this wave
  auto advance = [&](AgCur c) -> AgCur {
    if (c.kind == 0) {
      c.i += AD_WAVES;
      if (c.i < np) return c;
      c.kind = 1;
      c.q = -1;
    }
    if (c.kind == 1) {
      if (c.q >= 0) {
        c.i += AD_WAVES;
        if (c.i * AG_KT < sm_sl[c.q]) return c;
      }
      const uint32_t rest = c.q >= 31 ? 0u : smask & (~0u << (c.q + 1));
      if (rest) {
        c.q = __ffs(rest) - 1;
        c.i = (wave - c.q - np - 1) & 3;
        return c;
      }
      c.kind = wave == (np & 3) ? 2 : 3;
      return c;
    }
    c.kind = 3;
    return c;
  };

  // Lane-side view of a tile: key x of the tile (0 .. 31) stands at kb + x' * st with x' = x clamped to
  // the tile's last key and, in the new tile, redirected to an active query.
  auto load = [&](const AgCur c, bf16x8 kr[KS], bf16x8 vr[VU]) {
    const bf16_t *kb, *vb;
    int64_t st = D;
    int nk;
    uint32_t ok = ~0u;
    if (c.kind == 0) {
      kb = kpb + (int64_t)c.i * AG_KT * D;
      vb = vpb + (int64_t)c.i * AG_KT * D;
      nk = min(AG_KT, pl - c.i * AG_KT);
    } else if (c.kind == 1) {
      kb = ksb + c.q * ks_sb + (int64_t)c.i * AG_KT * D;
      vb = vsb + c.q * vs_sb + (int64_t)c.i * AG_KT * D;
      nk = min(AG_KT, sm_sl[c.q] - c.i * AG_KT);
    } else {
      kb = knew;
      vb = vnew;
      st = qkv_sb;
      nk = nq;
      ok = amask;
    }
    auto at = [&](int x) {
      x = min(x, nk - 1);
      return (ok >> x) & 1u ? x : qfirst;
    };
    const bf16_t* kq = kb + at(r) * st + 8 * hf;
#pragma unroll
    for (int s = 0; s < KS; ++s) kr[s] = ld_frag(kq + 16 * s);
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int ch = lane + 64 * u;
      vr[u] = ld_frag(vb + at(ch / CH) * st + (ch % CH) * 8);
    }
  };

  constexpr float qscale = (D == 64 ? 0.125f : 0.08838834764831845f) * LOG2E;  // 1 / sqrt D, exp2 domain
  char* vl = smem + wave * VBYTES;
  float m = -INFINITY, l = 0.f;  // m in the exp2 domain; l: this lane half's part of the sum
  f32x16 o[ND];                  // O^T: register i of tile dt is d = 32 dt + acc_row(i, hf) of query r
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();

  auto fold = [&](const AgCur c, const bf16x8 kr[KS], const bf16x8 vr[VU]) {
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int ch = lane + 64 * u;
      *reinterpret_cast<bf16x8*>(vl + swz<2 * D>(ch / CH, ch % CH)) = vr[u];
    }
    f32x16 acc = zero16();
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = mfma32(kr[s], qf[s], acc);
    // this column keeps the tile's keys lo .. hi - 1
    int lo = 0, hi = pl - c.i * AG_KT;
    if (c.kind == 1) hi = r == c.q ? sm_sl[c.q] - c.i * AG_KT : 0;
    if (c.kind == 2) {
      lo = r;
      hi = act ? r + 1 : 0;
    }
    if (c.kind != 0 || (c.i + 1) * AG_KT > pl) {  // wave-uniform
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int x = acc_row(i, hf);
        if (x < lo || x >= hi) acc[i] = -INFINITY;
      }
    }
    float tm = acc[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) tm = fmaxf(tm, acc[i]);
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64)) * qscale;
    const float mn = fmaxf(m, tm);
    const float ms = mn == -INFINITY ? 0.f : mn;  // no key yet: every exponent below is -inf, never NaN
    const float alpha = fexp2(m - ms);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
    uint32_t pk[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pk[j] = pack_bf2(fexp2(fmaf(acc[2 * j], qscale, -ms)), fexp2(fmaf(acc[2 * j + 1], qscale, -ms)));
      l += __uint_as_float(pk[j] << 16) + __uint_as_float(pk[j] & 0xffff0000u);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 pf = __builtin_bit_cast(bf16x8, (u32x4){pk[4 * s], pk[4 * s + 1], pk[4 * s + 2], pk[4 * s + 3]});
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) o[dt] = mfma32(lds_tr_frag<2 * D>(vl, 16 * s, dt * 32, lane), pf, o[dt]);
    }
  };

  AgCur c = advance(AgCur{0, -1, wave - AD_WAVES});
  if (c.kind != 3) {
    bf16x8 ka[KS], va[VU], kb[KS], vb[VU];
    load(c, ka, va);
    for (;;) {
      const AgCur n = advance(c);
      if (n.kind != 3) load(n, kb, vb);
      fold(c, ka, va);
      if (n.kind == 3) break;
      c = advance(n);
      if (c.kind != 3) load(c, ka, va);
      fold(n, kb, vb);
      if (c.kind == 3) break;
    }
  }

  // The merge (K-M27's).  A wave that had no tile for a column holds m = -inf there and adds zeros.
  l += __shfl_xor(l, 32, 64);
  if (hf == 0) {
    sm_ml[wave][r][0] = m;
    sm_ml[wave][r][1] = l;
  }
  __syncthreads();  // every wave has left its V tile: the image takes the space
  float mx = sm_ml[0][r][0];
#pragma unroll
  for (int w = 1; w < AD_WAVES; ++w) mx = fmaxf(mx, sm_ml[w][r][0]);
  // an active query's own key lies in some wave's tile, so its maximum is finite; an inactive column
  // of a group without prefix has none, and what it computes is not stored
  if (mx == -INFINITY) mx = 0.f;
  float ls = 0.f;
#pragma unroll
  for (int w = 0; w < AD_WAVES; ++w) ls = fmaf(sm_ml[w][r][1], fexp2(sm_ml[w][r][0] - mx), ls);
  const float a = fexp2(m - mx), inv = 1.f / ls;
  float* so = reinterpret_cast<float*>(smem) + r * OP;
#pragma unroll
  for (int w = 0; w < AD_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4* p = reinterpret_cast<f32x4*>(so + dt * 32 + 8 * g + 4 * hf);
          f32x4 v = (f32x4){o[dt][4 * g] * a, o[dt][4 * g + 1] * a, o[dt][4 * g + 2] * a, o[dt][4 * g + 3] * a};
          if (w > 0) v += *p;
          if (w == AD_WAVES - 1) v *= inv;
          *p = v;
        }
    }
    __syncthreads();
  }
  for (int i = tid; i < nq * (D / 2); i += NT) {
    const int q = i / (D / 2), d2 = i - q * (D / 2);
    uint32_t res = 0u;
    if ((amask >> q) & 1u) {
      const float* ow = reinterpret_cast<const float*>(smem) + q * OP + 2 * d2;
      res = pack_bf2(ow[0], ow[1]);
    }
    reinterpret_cast<uint32_t*>(orow + q * o_st)[d2] = res;
  }
}

int attn_decode_grouped_qs(int64_t BH, int G, int ncu) {
  for (int qs = 32; qs > 4; qs >>= 1)
    if (BH * ((G + qs - 1) / qs) >= ncu) return qs;
  return 4;
}

bool launch_attn_decode_grouped(const uint16_t* qkv_new, int64_t qkv_sb, const uint16_t* kp, const uint16_t* vp,
                                int64_t kp_sb, int64_t kp_sh, int64_t vp_sb, int64_t vp_sh, const int* plens, int Lp,
                                uint16_t* ks, uint16_t* vs, int64_t ks_sb, int64_t ks_sh, int64_t vs_sb,
                                int64_t vs_sh, const int* slens, int Ls, int B, int G, int H, int D, int qs,
                                uint16_t* out, hipStream_t s) {
  if (G < 1 || G > AG_QMAX || B < 1 || (int64_t)B * G > 0x7fffffffLL) return false;
  if (qs != 0 && qs != 4 && qs != 8 && qs != 16 && qs != 32) return false;
  if (!ad_args_ok(qkv_new, qkv_sb, kp, vp, kp_sb, kp_sh, vp_sb, vp_sh, plens, B, H, Lp, D, out) ||
      !ad_args_ok(qkv_new, qkv_sb, ks, vs, ks_sb, ks_sh, vs_sb, vs_sh, slens, B * G, H, Ls, D, out))
    return false;
  if (qs == 0) qs = attn_decode_grouped_qs((int64_t)B * H, G, device_cu_count());
  const int nsl = (G + qs - 1) / qs;
  if ((int64_t)B * H * nsl > 0x7fffffffLL) return false;
  const dim3 grid((unsigned)(B * H * nsl)), block(64 * AD_WAVES);
  if (D == 64)
    hipLaunchKernelGGL((attn_decode_grouped_kernel<64>), grid, block, 0, s, qkv_new, qkv_sb, kp, vp, kp_sb, kp_sh,
                       vp_sb, vp_sh, plens, Lp, ks, vs, ks_sb, ks_sh, vs_sb, vs_sh, slens, Ls, G, H, qs, nsl, out);
  else
    hipLaunchKernelGGL((attn_decode_grouped_kernel<128>), grid, block, 0, s, qkv_new, qkv_sb, kp, vp, kp_sb, kp_sh,
                       vp_sb, vp_sh, plens, Lp, ks, vs, ks_sb, ks_sh, vs_sb, vs_sh, slens, Ls, G, H, qs, nsl, out);
  return true;
}

}  // namespace dpa
