// The vocabulary sweep shared by the head kernels of xent.hip (lxent_fwd, lxent_dx,
// lxent_fwd_dx) and linear_argmax.hip: a workgroup of 256 threads is 128 tokens (token on the
// MFMA lane, x fragments in registers) and walks (a split of) the vocabulary in 64-row W tiles
// staged through one swizzled LDS image; the 32x32 logit accumulators start at a per-row
// offset staged beside the tile.  Device pieces first, then the host plan that every launcher
// and its workspace size are derived from.  The logit tile itself (accumulators from the staged
// offsets, then E / 16 MFMAs from lds_frag) stays written out in each kernel: as a function it
// costs registers in every one of them (profiles/head_sweep_refactor_resources.txt).
#pragma once
#include <type_traits>

#include "common.h"
#include "mfma.h"

namespace dpa {

// ---------------------------------------------------------------------------
// W-tile staging (64 rows x E) into a swizzled LDS image, register-staged; the kernels read
// it with lds_frag / lds_tr_frag.
// ---------------------------------------------------------------------------
template <int E, int NT>
struct WTile {
  static constexpr int CH = E / 8;             // 16-byte chunks per row
  static constexpr int ROWB = E * 2;
  static constexpr int PER = 64 * CH / NT;     // chunks per thread
  uint4 r[PER];

  __device__ __forceinline__ void load(const bf16_t* __restrict__ W, int v0, int V, int tid) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = tid + i * NT;
      const int row = c / CH, ch = c % CH;
      const int v = v0 + row;
      if (v < V)
        r[i] = *reinterpret_cast<const uint4*>(W + (int64_t)v * E + ch * 8);
      else
        r[i] = make_uint4(0, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void store(char* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = tid + i * NT;
      const int row = c / CH, ch = c % CH;
      *reinterpret_cast<uint4*>(lds + swz<ROWB>(row, ch)) = r[i];
    }
  }
};

// This lane's fragment of token t for k-step s (columns 16 s + 8 h ..), zero for t >= N.  One
// fragment per call, the loop over s stays in the kernel: a helper that fills the whole
// xf[KS] is simplified on its own before it is inlined and changes the kernels' code.
template <int E>
__device__ __forceinline__ bf16x8 token_frag(const bf16_t* __restrict__ x, int t, bool tok_ok, int s, int h) {
  bf16x8 f;
  if (tok_ok) f = ld_frag(x + (int64_t)t * E + 16 * s + 8 * h);
  else for (int j = 0; j < 8; ++j) f[j] = 0;
  return f;
}

// Offsets of the tile's 64 rows: offset(v) for v < vend, -inf for rows past the split /
// vocabulary (their zero-padded W rows then never count).  Before the tile's barrier.
template <class F>
__device__ __forceinline__ void stage_offsets(float* bt, int v0, int vend, int tid, F offset) {
  if (tid < 64) {
    const int v = v0 + tid;
    bt[tid] = (v < vend) ? offset(v) : -INFINITY;
  }
}

// Vocabulary split and token block of this workgroup.  xsplit > 1: 1-D grid, split =
// blockIdx.x % xsplit, i.e. (with the round-robin workgroup -> XCD dispatch) every XCD sweeps
// only its 1/8 of W, which then stays resident in that XCD's L2 instead of streaming all of W
// from the MALL per workgroup; otherwise a 2-D grid (token block, split).
struct SweepBlock {
  int split, tblk, nsplit;
};
__device__ __forceinline__ SweepBlock sweep_block(int xsplit) {
  SweepBlock b;
  b.split = xsplit > 1 ? (int)(blockIdx.x % xsplit) : (int)blockIdx.y;
  b.tblk = xsplit > 1 ? (int)(blockIdx.x / xsplit) : (int)blockIdx.x;
  b.nsplit = xsplit > 1 ? xsplit : (int)gridDim.y;
  return b;
}

// ---------------------------------------------------------------------------
// Host plan
// ---------------------------------------------------------------------------
// splits of `chunks` units so that blocks x splits reaches ~target_wgs workgroups
inline int pick_splits(int blocks, int chunks, int target_wgs) {
  int s = (target_wgs + blocks - 1) / blocks;
  if (s < 1) s = 1;
  if (s > chunks) s = chunks;
  return s;
}

// Rounding of the split count to a multiple of 8 (one split per XCD, see sweep_block) once
// the vocabulary has 8 x 64 rows: never, only when the shape is split at all, or always.
enum class XcdRound { none, if_split, always };

struct SweepPlan {
  int tb;   // token blocks of 128
  int Sx;   // vocabulary splits, none empty
  int vps;  // rows per split, a multiple of 64
};

// Enough splits for ~target_wgs workgroups (0: no split).
inline SweepPlan sweep_plan(int N, int V, int target_wgs, XcdRound xcd) {
  const int tb = (N + 127) / 128, vchunks = (V + 63) / 64;
  int S = pick_splits(tb, vchunks, target_wgs);
  if (vchunks >= 8 && (xcd == XcdRound::always || (xcd == XcdRound::if_split && S > 1))) S = (S + 7) / 8 * 8;
  const int vps = ((vchunks + S - 1) / S) * 64;
  return {tb, (V + vps - 1) / vps, vps};
}

// f(std::integral_constant<int, E>) for the embedding widths the kernels are built for
template <class F>
inline void for_head_width(int E, F f) {
  if (E == 128) f(std::integral_constant<int, 128>{});
  else f(std::integral_constant<int, 256>{});
}

}  // namespace dpa
