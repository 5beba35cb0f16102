// K-M27.  GPT-2 generation: append a run of T new tokens per row (1 <= T <= 128) to a K/V cache that
// may already hold something, and attend each of them over the cache and the run in front of it -
// chunked prefill, continuing from a warm cache, verifying a long draft.  The matrix-core sibling of
// attn_decode_block.hip, whose arguments and rule it shares:
//
//   qkv_new [B][T][3][H][D] bf16  the run's packed projections (row b, token j at b * sb + j * st)
//   k_cache / v_cache             bf16 rows of D at (b, h, key): base + b * sb + h * sh + key * D
//   lens [B] int32                keys already cached per row, before the call (not modified)
//   counts [B] int32 or null      tokens of the run that are real, per row (null: T)
//   out [B][T][H][D] bf16
//
// c_b = 0 for a row with lens[b] outside [0, Lmax), otherwise clamp(counts[b], 0, min(T, Lmax - lens[b])).
// Query j < c_b stores the bits of its k and v at cache row lens[b] + j and returns
// softmax(q_j K^T / sqrt D) V over the keys 0 .. lens[b] + j; query j >= c_b stores nothing and returns
// zeros.  Cache rows at or beyond lens[b] + c_b are neither loaded nor stored.
//
// Work split.  One workgroup of 4 waves per (b, h, tile of 32 queries); a tile without an active query
// zeroes its rows of out and leaves.  The 32-key tiles of [0, lens + the tile's last active query] go
// round-robin to the waves, each wave keeps an online-softmax state of its own, and the four states
// are merged once through LDS in wave order, one writer per output element at a time - the decode
// kernels' split, so a (b, h) with few queries still streams its cache with four waves.  The merge
// adds the waves' scaled O^T into one [32][D] image, a barrier per wave, where the decode kernels
// keep four images: four of them at D = 128 would take more than 64 KiB of LDS.  No atomics, no
// workspace: two calls agree bit for bit.
//
// Scores.  S^T = K Q^T on v_mfma_f32_32x32x16_bf16 with K as the A operand: a lane's fragment is 16
// contiguous bytes of one key row, loaded from global memory straight into registers.  Every load is
// unconditional, on a key clamped to the tile's last one; the weight is masked afterwards.  Q is the B
// operand, loaded once and kept in registers.  A lane then owns one query column: running max and sum
// are per lane, plus one exchange between the lane halves (16 keys of the tile each).
// The scale 1 / sqrt D * log2 e is applied to the fp32 scores inside the exponent's FMA and not to Q:
// a Q rounded to bf16 a second time would put an error of 2^-9 relative on every score for the price
// of nothing - the FMA is needed for the subtraction of the maximum anyway.
//
// Output.  P is rounded to bf16 once and O^T += V^T P^T runs on the same MFMA, so O's columns stay on
// the lanes that own the queries and the rescale by exp2(m_old - m_new) is a per-lane factor.  The S
// accumulator serves as the P operand as it stands: its registers 8s .. 8s + 7 are the keys
// 16 s + 8 (j >> 2) + 4 half + (j & 3), and V's fragment is read from LDS in that key order
// (lds_tr_frag) - a sum over keys has no order to keep.  V goes through a swizzled, wave-private LDS
// tile because the A fragment needs 8 keys of one d.  The row sum adds up the rounded weights, the
// ones that O is made of.  Two stages: while a wave folds one tile, the K and V registers of its next
// one are in flight.
//
// The run's own keys (positions lens .. lens + j) are loaded from qkv_new, whose bits they are; a
// workgroup never reads back a store of the call, its own or another tile's.  The causal mask runs
// only in key tiles that reach beyond lens + the tile's first query.  The appends of the whole run are
// done by the workgroup of query tile 0 with 16-byte stores.  A masked weight is an exact zero, but V
// is not masked per query: a non-finite value in the k or v of a later token of the run reaches the
// earlier queries of its 32-key tile (the VALU kernels mask V too; finite inputs cannot tell).
#include <math.h>

#include "attn_decode.h"
#include "common.h"
#include "launchers.h"
#include "mfma.h"

namespace dpa {

constexpr int AX_QT = 32;     // queries per workgroup
constexpr int AX_KT = 32;     // keys per wave tile
constexpr int AX_T_MAX = 128;

template <int D>
__global__ void __launch_bounds__(64 * AD_WAVES) attn_extend_kernel(
    const bf16_t* __restrict__ qkv, int64_t qkv_sb, int64_t qkv_st, bf16_t* __restrict__ kc,
    bf16_t* __restrict__ vc, int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* __restrict__ lens,
    const int* __restrict__ counts, int T, int H, int Lmax, int NQT, bf16_t* __restrict__ out) {
  constexpr int CH = D / 8;               // 16-byte chunks per row
  constexpr int VU = AX_KT * CH / 64;     // chunks of a V tile per lane
  constexpr int KS = D / 16;              // k-steps of S
  constexpr int ND = D / 32;              // 32-row tiles of O^T
  constexpr int NT = 64 * AD_WAVES;
  constexpr int VBYTES = AX_KT * 2 * D;   // a wave's V tile
  constexpr int OP = D + 4;               // floats per query in the merge buffer (padded against bank conflicts)
  constexpr int MBYTES = AX_QT * OP * 4;
  // the V tiles while the waves stream, the merge image afterwards
  __shared__ __attribute__((aligned(16))) char smem[MBYTES > AD_WAVES * VBYTES ? MBYTES : AD_WAVES * VBYTES];
  __shared__ float sm_ml[AD_WAVES][AX_QT][2];

  const int qt = blockIdx.x % NQT, bh = blockIdx.x / NQT;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int n = lens[b];  // cached keys; token j becomes key n + j
  int cnt = 0;            // c_b (uniform over the workgroup)
  if (n >= 0 && n < Lmax) cnt = max(0, min(counts ? counts[b] : T, min(T, Lmax - n)));
  const int j0 = qt * AX_QT;
  const int jn = min(AX_QT, T - j0);  // the tile's rows of out
  bf16_t* orow = out + (((int64_t)b * T + j0) * H + h) * D;  // query j0 + q: + q * H * D
  const int64_t o_st = (int64_t)H * D;
  if (j0 >= cnt) {
    for (int i = tid; i < jn * (D / 2); i += NT)
      reinterpret_cast<uint32_t*>(orow + (i / (D / 2)) * o_st)[i % (D / 2)] = 0u;
    return;
  }

  // token j's q; its k and v stand H D and 2 H D elements behind
  const bf16_t* qnew = qkv + (int64_t)b * qkv_sb + (int64_t)h * D;
  const bf16_t* knew = qnew + (int64_t)H * D;
  const bf16_t* vnew = qnew + 2 * (int64_t)H * D;
  bf16_t* kbase = kc + (int64_t)b * k_sb + (int64_t)h * k_sh;
  bf16_t* vbase = vc + (int64_t)b * v_sb + (int64_t)h * v_sh;
  if (qt == 0)  // the appends of the whole run: rows n .. n + cnt - 1 < Lmax
    for (int i = tid; i < cnt * CH; i += NT) {
      const int j = i / CH, c = i - j * CH;
      *reinterpret_cast<uint4*>(kbase + (int64_t)(n + j) * D + c * 8) =
          *reinterpret_cast<const uint4*>(knew + (int64_t)j * qkv_st + c * 8);
      *reinterpret_cast<uint4*>(vbase + (int64_t)(n + j) * D + c * 8) =
          *reinterpret_cast<const uint4*>(vnew + (int64_t)j * qkv_st + c * 8);
    }

  const int jlast = min(j0 + AX_QT, cnt) - 1;  // the tile's last active query
  const int klast = n + jlast;                 // its last key, the tile's last
  const int ntile = klast / AX_KT + 1;
  // this lane's query; the lanes behind the last active one repeat it (their rows of out get zeros)
  const int jq = min(j0 + r, jlast);
  const int qpos = n + jq;  // the query's last key
  bf16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = ld_frag(qnew + (int64_t)jq * qkv_st + 16 * s + 8 * hf);

  // rows of K (V) of the keys <= klast: below n from the cache, from n on out of qkv_new
  auto krow = [&](int key) { return key < n ? kbase + (int64_t)key * D : knew + (int64_t)(key - n) * qkv_st; };
  auto vrow = [&](int key) { return key < n ? vbase + (int64_t)key * D : vnew + (int64_t)(key - n) * qkv_st; };
  auto load = [&](int t, bf16x8 kr[KS], bf16x8 vr[VU]) {
    const bf16_t* kp = krow(min(t * AX_KT + r, klast)) + 8 * hf;
#pragma unroll
    for (int s = 0; s < KS; ++s) kr[s] = ld_frag(kp + 16 * s);
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int c = lane + 64 * u;
      vr[u] = ld_frag(vrow(min(t * AX_KT + c / CH, klast)) + (c % CH) * 8);
    }
  };

  constexpr float qscale = (D == 64 ? 0.125f : 0.08838834764831845f) * LOG2E;  // 1 / sqrt D, exp2 domain
  char* vl = smem + wave * VBYTES;
  float m = -INFINITY, l = 0.f;  // m in the exp2 domain; l: this lane half's part of the sum
  f32x16 o[ND];                  // O^T: register i of tile dt is d = 32 dt + acc_row(i, hf) of query r
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();

  auto fold = [&](int t, const bf16x8 kr[KS], const bf16x8 vr[VU]) {
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int c = lane + 64 * u;
      *reinterpret_cast<bf16x8*>(vl + swz<2 * D>(c / CH, c % CH)) = vr[u];
    }
    f32x16 acc = zero16();
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = mfma32(kr[s], qf[s], acc);
    const int k0 = t * AX_KT;
    if (k0 + AX_KT - 1 > n + j0) {  // wave-uniform: the tile reaches beyond the first query's last key
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (k0 + acc_row(i, hf) > qpos) acc[i] = -INFINITY;
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

  int t = wave;  // wave-uniform, as is every branch on it
  if (t < ntile) {
    bf16x8 ka[KS], va[VU], kb[KS], vb[VU];
    load(t, ka, va);
    for (;;) {
      if (t + AD_WAVES < ntile) load(t + AD_WAVES, kb, vb);
      fold(t, ka, va);
      t += AD_WAVES;
      if (t >= ntile) break;
      if (t + AD_WAVES < ntile) load(t + AD_WAVES, ka, va);
      fold(t, kb, vb);
      t += AD_WAVES;
      if (t >= ntile) break;
    }
  }

  // The merge.  Every wave scales its O^T by exp2(m_wave - max over the waves) and the waves add
  // theirs into one [32][D] fp32 image in wave order, a barrier apart: an element has one writer at a
  // time and one order of summation.  A wave that had no tile holds m = -inf and adds zeros.
  l += __shfl_xor(l, 32, 64);
  if (hf == 0) {
    sm_ml[wave][r][0] = m;
    sm_ml[wave][r][1] = l;
  }
  __syncthreads();  // every wave has left its V tile: the image takes the space
  // the query's own key lies in some wave's tile, so the maximum is finite
  float mx = sm_ml[0][r][0];
#pragma unroll
  for (int w = 1; w < AD_WAVES; ++w) mx = fmaxf(mx, sm_ml[w][r][0]);
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
  for (int i = tid; i < jn * (D / 2); i += NT) {
    const int q = i / (D / 2), d2 = i - q * (D / 2);
    uint32_t res = 0u;
    if (j0 + q < cnt) {
      const float* ow = reinterpret_cast<const float*>(smem) + q * OP + 2 * d2;
      res = pack_bf2(ow[0], ow[1]);
    }
    reinterpret_cast<uint32_t*>(orow + q * o_st)[d2] = res;
  }
}

bool launch_attn_extend(const uint16_t* qkv_new, int64_t qkv_sb, int64_t qkv_st, uint16_t* k_cache,
                        uint16_t* v_cache, int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* lens,
                        const int* counts, int B, int T, int H, int Lmax, int D, uint16_t* out, hipStream_t s) {
  if (T < 1 || T > AX_T_MAX || qkv_st % 8) return false;
  if (!ad_args_ok(qkv_new, qkv_sb, k_cache, v_cache, k_sb, k_sh, v_sb, v_sh, lens, B, H, Lmax, D, out))
    return false;
  const int nqt = (T + AX_QT - 1) / AX_QT;
  if ((int64_t)B * H * nqt > 0x7fffffffLL) return false;
  const dim3 grid((unsigned)(B * H * nqt)), block(64 * AD_WAVES);
  if (D == 64)
    hipLaunchKernelGGL((attn_extend_kernel<64>), grid, block, 0, s, qkv_new, qkv_sb, qkv_st, k_cache, v_cache, k_sb,
                       k_sh, v_sb, v_sh, lens, counts, T, H, Lmax, nqt, out);
  else
    hipLaunchKernelGGL((attn_extend_kernel<128>), grid, block, 0, s, qkv_new, qkv_sb, qkv_st, k_cache, v_cache, k_sb,
                       k_sh, v_sb, v_sh, lens, counts, T, H, Lmax, nqt, out);
  return true;
}

}  // namespace dpa
