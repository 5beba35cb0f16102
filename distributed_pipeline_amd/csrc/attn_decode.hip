// GPT-2 generation: the KV-cache append and the single-query attention of one decode step as one
// kernel.
//
//   qkv_new [B][3][H][D] bf16   the new token's packed projection (rows qkv_stride apart)
//   k_cache / v_cache           bf16 rows of D at (b, h, key): base + b * sb + h * sh + key * D
//   lens [B] int32              keys already cached per row, before the call (not modified)
//   out [B][H][D] bf16          softmax(q K^T / sqrt D) V over the keys 0 .. lens[b], rounded once
//
// A row with 0 <= lens[b] < Lmax stores the new k and v (the bits of qkv_new) at cache row lens[b]
// and attends over the lens[b] cached keys plus the new one, which is taken from registers and
// never re-read.  Any other lens[b] marks an inactive (parked) row: nothing is stored and its out
// row is zeros.  Cache rows at or beyond lens[b] are never loaded, whatever they hold.
//
// The step is a memory-bound read of 2 * len * D * 2 bytes per (b, h) at one query row, so there
// is nothing for the matrix cores and nothing to share through LDS: one workgroup of 4 waves per
// (b, h); D / 8 lanes own a key row in 16-byte loads, so one wave load covers KPW = 512 / D whole
// keys (1 KB, contiguous); a wave takes U = 4 such loads of K and of V (U * KPW consecutive keys)
// per iteration and issues the next iteration's loads before it computes on this one's (two
// register sets, ping-pong).  Each lane group keeps an fp32 online-softmax triple (m, l, o slice)
// in the exp2 domain; probabilities and the PV sum stay in fp32 on the VALU.  The lane groups of a
// wave merge by shuffles, the four waves once through 4 * (D + 2) floats of LDS.  No atomics, one
// writer per output element: results are bitwise reproducible.
//
// The grid is B * H workgroups; there is no split over keys across workgroups, so a small batch
// does not fill the chip.
//
// The AdTable instantiations are the same step for beam search: rows come in groups of W (row
// b W + w is slot w of prompt b) and a uint8 table src [B][Lmax] names, per row and cached position,
// the slot of the row's group that holds that key - hypotheses are re-parented by rewriting W Lmax
// bytes per prompt instead of gathering the caches.  The AdNoTable instantiations carry none of
// it: their instruction stream is what it was without the table.
#include <math.h>

#include <type_traits>

#include "attn_decode.h"
#include "common.h"
#include "launchers.h"

namespace dpa {

// TAB = AdTable: cached key t of row b is read from cache row (b / W) W + min(src[b][t], W - 1) - a
// slot of the row's own group of W rows, whatever the byte - while the append still goes to the
// row's own slot.  The table bytes of an iteration are fetched one iteration ahead of its K/V loads
// (which depend on them), beside the ping-pong prefetch: a wave load is then KPW rows of 2 D bytes,
// each anywhere in the group, instead of 1 KB contiguous.  The fold order over keys, lane groups and
// waves is the same, so an identity table gives the plain kernel's bits.  Caller's contract: no
// active row reads a (slot, position) that another active row of the same call appends to (true
// whenever the active rows of a group have equal lens).
struct AdNoTable {};
struct AdTable {
  const uint8_t* src;  // [B][Lmax] bytes, rows `stride` apart
  int64_t stride;
  int W;
};

template <int D, typename TAB>
__global__ void __launch_bounds__(64 * AD_WAVES) attn_decode_kernel(
    const bf16_t* __restrict__ qkv, int64_t qkv_stride, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
    int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* __restrict__ lens, int H, int Lmax,
    bf16_t* __restrict__ out, TAB tab) {
  constexpr bool BEAM = !std::is_same<TAB, AdNoTable>::value;
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
  const uint4 knew = *reinterpret_cast<const uint4*>(qrow + (int64_t)H * D);
  const uint4 vnew = *reinterpret_cast<const uint4*>(qrow + 2 * (int64_t)H * D);
  const bf16_t* kb = kc + (int64_t)b * k_sb + (int64_t)h * k_sh + c * 8;
  const bf16_t* vb = vc + (int64_t)b * v_sb + (int64_t)h * v_sh + c * 8;
  if (wave == 0 && g == 0) {  // the append: n < Lmax
    *reinterpret_cast<uint4*>(kc + (int64_t)b * k_sb + (int64_t)h * k_sh + (int64_t)n * D + c * 8) = knew;
    *reinterpret_cast<uint4*>(vc + (int64_t)b * v_sb + (int64_t)h * v_sh + (int64_t)n * D + c * 8) = vnew;
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
  auto load = [&](int base, uint4 kr[U], uint4 vr[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * KPW + g;
      kr[u] = make_uint4(0u, 0u, 0u, 0u);
      vr[u] = make_uint4(0u, 0u, 0u, 0u);
      if (key < n) {
        kr[u] = *reinterpret_cast<const uint4*>(kb + (int64_t)key * D);
        vr[u] = *reinterpret_cast<const uint4*>(vb + (int64_t)key * D);
      }
    }
  };
  auto fold = [&](int base, const uint4 kr[U], const uint4 vr[U]) {
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float d = ad_dot<G>(q, kr[u]);
      s[u] = (base + u * KPW + g < n) ? d : -INFINITY;
    }
    ad_update<U>(st, s, vr);
  };

  int base = wave * WK;  // wave-uniform, as is every branch on it
  if constexpr (BEAM) {
    const int W = tab.W;
    const int gb = b / W * W;  // the group's first cache row
    const bf16_t* kg = kc + (int64_t)gb * k_sb + (int64_t)h * k_sh + c * 8;
    const bf16_t* vg = vc + (int64_t)gb * v_sb + (int64_t)h * v_sh + c * 8;
    const uint8_t* srow = tab.src + (int64_t)b * tab.stride;
    // Every load of this variant is unconditional, on a key clamped to n - 1: a lane whose key lies
    // at or beyond n reads the byte and the rows of key n - 1 (never anything at or beyond n) and the
    // fold gives them weight 0, as it gives the zeros of the plain kernel.  Without a branch around
    // each load the compiler counts the loads in flight exactly, instead of draining them in front
    // of every dependent load.
    auto slots = [&](int base, int sl[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) sl[u] = (int)srow[min(base + u * KPW + g, n - 1)];
    };
    auto gload = [&](int base, const int sl[U], uint4 kr[U], uint4 vr[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int key = min(base + u * KPW + g, n - 1);
        const int slot = min(sl[u], W - 1);  // inside the group, whatever the table holds
        kr[u] = *reinterpret_cast<const uint4*>(kg + (int64_t)slot * k_sb + (int64_t)key * D);
        vr[u] = *reinterpret_cast<const uint4*>(vg + (int64_t)slot * v_sb + (int64_t)key * D);
      }
    };
    if (base < n) {  // n >= 1
      // Loads return in issue order, so the bytes an iteration's K/V loads wait for must be older
      // than the K/V loads in flight: the bytes of iteration i + 2 are issued in front of the K/V
      // loads of iteration i + 1 (two byte sets, ping-pong like the K/V sets).  Issued behind them,
      // the wait for the bytes would drain the K/V loads too - one exposed memory latency per
      // iteration instead of half of one.  The loads of the iterations past the end (clamped, all
      // on key n - 1) are issued and never used.
      uint4 ka[U], va[U], kb2[U], vb2[U];
      int sla[U], slb[U];
      slots(base, slb);
      slots(base + IT, sla);
      __builtin_amdgcn_sched_barrier(0);
      gload(base, slb, ka, va);
      for (;;) {
        slots(base + 2 * IT, slb);
        __builtin_amdgcn_sched_barrier(0);
        gload(base + IT, sla, kb2, vb2);
        fold(base, ka, va);
        base += IT;
        if (base >= n) break;
        slots(base + 2 * IT, sla);
        __builtin_amdgcn_sched_barrier(0);
        gload(base + IT, slb, ka, va);
        fold(base, kb2, vb2);
        base += IT;
        if (base >= n) break;
      }
    }
  } else if (base < n) {
    uint4 ka[U], va[U], kb2[U], vb2[U];
    load(base, ka, va);
    for (;;) {
      if (base + IT < n) load(base + IT, kb2, vb2);
      fold(base, ka, va);
      base += IT;
      if (base >= n) break;
      if (base + IT < n) load(base + IT, ka, va);
      fold(base, kb2, vb2);
      base += IT;
      if (base >= n) break;
    }
  }

  {  // the new key, from registers: group 0 of wave 0 takes it
    const float d = ad_dot<G>(q, knew);
    const float s[1] = {(wave == 0 && g == 0) ? d : -INFINITY};
    const uint4 v1[1] = {vnew};
    ad_update<1>(st, s, v1);
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

bool launch_attn_decode_beam(const uint16_t* qkv_new, int64_t qkv_stride, uint16_t* k_cache, uint16_t* v_cache,
                             int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* lens,
                             const uint8_t* src, int64_t src_stride, int W, int B, int H, int Lmax, int D,
                             uint16_t* out, hipStream_t s) {
  if (!ad_args_ok(qkv_new, qkv_stride, k_cache, v_cache, k_sb, k_sh, v_sb, v_sh, lens, B, H, Lmax, D, out))
    return false;
  if (!src || W < 1 || W > 255 || B % W || src_stride < Lmax || Lmax > (1 << 30)) return false;
  const dim3 grid((unsigned)(B * H)), block(64 * AD_WAVES);
  const AdTable tab{src, src_stride, W};
  if (D == 64)
    hipLaunchKernelGGL((attn_decode_kernel<64, AdTable>), grid, block, 0, s, qkv_new, qkv_stride, k_cache, v_cache,
                       k_sb, k_sh, v_sb, v_sh, lens, H, Lmax, out, tab);
  else
    hipLaunchKernelGGL((attn_decode_kernel<128, AdTable>), grid, block, 0, s, qkv_new, qkv_stride, k_cache, v_cache,
                       k_sb, k_sh, v_sb, v_sh, lens, H, Lmax, out, tab);
  return true;
}

bool launch_attn_decode(const uint16_t* qkv_new, int64_t qkv_stride, uint16_t* k_cache, uint16_t* v_cache,
                        int64_t k_sb, int64_t k_sh, int64_t v_sb, int64_t v_sh, const int* lens, int B, int H,
                        int Lmax, int D, uint16_t* out, hipStream_t s) {
  if (!ad_args_ok(qkv_new, qkv_stride, k_cache, v_cache, k_sb, k_sh, v_sb, v_sh, lens, B, H, Lmax, D, out))
    return false;
  const dim3 grid((unsigned)(B * H)), block(64 * AD_WAVES);
  if (D == 64)
    hipLaunchKernelGGL((attn_decode_kernel<64, AdNoTable>), grid, block, 0, s, qkv_new, qkv_stride, k_cache, v_cache,
                       k_sb, k_sh, v_sb, v_sh, lens, H, Lmax, out, AdNoTable{});
  else
    hipLaunchKernelGGL((attn_decode_kernel<128, AdNoTable>), grid, block, 0, s, qkv_new, qkv_stride, k_cache, v_cache,
                       k_sb, k_sh, v_sb, v_sh, lens, H, Lmax, out, AdNoTable{});
  return true;
}

}  // namespace dpa
