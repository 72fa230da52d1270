// The LDS-tiled fp32 MFMA main loop of conv_gemm.hip (tile geometry, variants, K loop), shared with the kernels that wrap it
// with an operand mapping of their own (similarity_grouped.hip).  One definition = one k order: every kernel built on it
// sums the channels in the same sequence and is bit-identical to the others on equal operands.
#pragma once
#include "common.h"
#include "gemm_loader.h"

namespace {

// Template int VAR — variants selectable through wd_conv_gemm_tuned for on-device A/B runs
// (profiles/r01_gemm_ab.txt records what was measured).
constexpr int VAR_PRIO = 1;        // s_setprio(1) over the MFMA cluster (measured: null)
constexpr int VAR_PIN = 2;         // sched_barrier fences: loads first, MFMAs, then wait + LDS store
                                   // (measured: +8 % on small low-occupancy problems, -4..-10 % on saturated ones)
constexpr int VAR_XCD = 256;       // XCD-aware tile order: each XCD's L2 sees whole A row panels (+0..5 %)
// timing-only ablations (WRONG results by construction): skip the in-loop global loads / LDS
// stores / barrier / the epilogue
constexpr int ABL_NOLOAD = 4, ABL_NOBAR = 8, ABL_NOEPI = 16, ABL_NOLDS = 32;
// Tried and dropped in round 1 (all bit-exact, none faster): prefetch two K steps ahead with two
// register sets (-6..-13 %), hoisting / prefetching the epilogue operands (-9 %), staggering the
// co-resident workgroups (0 %), sched_group_barrier interleave (0 %), v_mfma_f32_32x32x2_f32
// tiles (0..-6 %), 4-wave 64x64 wave tiles and K step 32/64 (-10..-30 %), 6/10/12-wave workgroups
// (96/160/192-row tiles, -10..-25 %: waves no longer spread evenly over the 4 SIMDs).


template <int TM, int TN, int WM, int WN, int BK_ = 32>
struct Tile {
  static constexpr int BK = BK_;
  // Row pitch in floats.  BK + 8 (10 / 6 sixteen-byte slots for BK = 32 / 16), not BK + 4: ds_read_b128 is served in four
  // groups of 16 lanes — {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 — over a 256-byte bank row of sixteen
  // 16-byte slots; a fragment read puts lane (i = lane & 15, g = lane >> 4) at slot (pitch * i + g) mod 16.  With a pitch of
  // 9 (or 5) slots seven slots of every group are hit twice (two LDS cycles per group: SQ_LDS_BANK_CONFLICT was 35 % of
  // SQ_LDS_IDX_ACTIVE on the similarity GEMM, round-3 review); 10 and 6 are the smallest pitches with 16 distinct slots in
  // all four groups.  The staging ds_write_b128 (8 consecutive lanes = one row's 8 consecutive chunks) is conflict-free at
  // any pitch.  Same arithmetic: results are bit-identical.
  static constexpr int LD = BK + 8;
  static constexpr int KCH = BK / 4;                     // float4 chunks per row per K step
  static constexpr int BM = 16 * TM * WM;
  static constexpr int BN = 16 * TN * WN;
  static constexpr int NT = 64 * WM * WN;
  static constexpr int A_PT = (BM * KCH) / NT;           // float4 chunks of A per thread per K step
  static constexpr int B_PT = (BN * KCH + NT - 1) / NT;
  static constexpr int RSTEP = NT / KCH;
  static constexpr int BN_LDS = B_PT * RSTEP;            // >= BN: every thread stores unconditionally
  static constexpr int LDS_BYTES = 2 * (BM + BN_LDS) * LD * 4;
  static_assert((BM * KCH) % NT == 0, "A tile must split evenly over the threads");
  static_assert(NT % KCH == 0, "threads must tile the K chunks");
};

// ---------------------------------------------------------------------------------------
// Main loop shared by all kernels: acc[tm][tn] (+)= X[m, :] . W[n, :]
// ---------------------------------------------------------------------------------------
template <class T, int TM, int TN, int WN, int VAR, class AL, class PreLast>
__device__ __forceinline__ void gemm_mainloop(const AL& al, const float* __restrict__ w, int n0, int N, int K,
                                              f32x4 (&acc)[TM][TN], float* smem, PreLast&& pre_last) {
  constexpr int BK = T::BK, LD = T::LD, KCH = T::KCH;
  constexpr int BM = T::BM, A_PT = T::A_PT, B_PT = T::B_PT, RSTEP = T::RSTEP, BN_LDS = T::BN_LDS;
  float* As = smem;
  float* Bs = smem + 2 * BM * LD;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int kc = t % KCH, r0 = t / KCH;
  const int nk = (K + BK - 1) / BK;

  f32x4 areg[A_PT], breg[B_PT];
  size_t boff[B_PT];
  bool bok[B_PT];
#pragma unroll
  for (int j = 0; j < B_PT; ++j) {
    const int n = n0 + r0 + j * RSTEP;
    bok[j] = (r0 + j * RSTEP) < T::BN && n < N;
    boff[j] = bok[j] ? (size_t)n * K : 0;
  }

  auto load_b = [&](int k) {
    const bool kok = k < K;
    const int kk = kok ? k : 0;
#pragma unroll
    for (int j = 0; j < B_PT; ++j)
      breg[j] = *reinterpret_cast<const f32x4*>((bok[j] && kok) ? w + boff[j] + kk : g_zero4);
  };
  auto store = [&](int buf) {
    float* ad = As + buf * BM * LD + r0 * LD + kc * 4;
#pragma unroll
    for (int i = 0; i < A_PT; ++i) *reinterpret_cast<f32x4*>(ad + i * RSTEP * LD) = areg[i];
    float* bd = Bs + buf * BN_LDS * LD + r0 * LD + kc * 4;
#pragma unroll
    for (int j = 0; j < B_PT; ++j) *reinterpret_cast<f32x4*>(bd + j * RSTEP * LD) = breg[j];
  };
  auto compute = [&](int buf) {
    const float* as = As + buf * BM * LD + (wm * TM * 16 + (lane & 15)) * LD + 4 * (lane >> 4);
    const float* bs = Bs + buf * BN_LDS * LD + (wn * TN * 16 + (lane & 15)) * LD + 4 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      f32x4 xf[TM], wf[TN];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) xf[tm] = *reinterpret_cast<const f32x4*>(as + tm * 16 * LD + ks * 16);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) wf[tn] = *reinterpret_cast<const f32x4*>(bs + tn * 16 * LD + ks * 16);
      if (VAR & VAR_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[tn][r], xf[tm][r], acc[tm][tn], 0, 0, 0);
      if (VAR & VAR_PRIO) __builtin_amdgcn_s_setprio(0);
    }
  };

#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

  al.template load<BK>(0, kc * 4, areg);
  load_b(kc * 4);
  store(0);
  __syncthreads();

  int cur = 0;
  for (int kt = 1; kt < nk; ++kt) {
    const int k = kt * BK + kc * 4;
    if (!(VAR & ABL_NOLOAD)) {
      al.template load<BK>(kt * BK, kc * 4, areg);   // tile kt: global -> VGPR, in flight during the MFMAs of tile kt-1
      load_b(k);
    }
    // Without these fences hipcc sinks the two global loads down to their only consumer (the
    // ds_write at the end of the step) and waits for them on the spot, exposing the whole
    // memory round trip every K step; pinned, the loads fly during this step's MFMAs.
    if (VAR & VAR_PIN) __builtin_amdgcn_sched_barrier(0);
    compute(cur);
    if (VAR & VAR_PIN) __builtin_amdgcn_sched_barrier(0);
    if (!(VAR & ABL_NOLDS)) store(cur ^ 1);
    if (!(VAR & ABL_NOBAR)) __syncthreads();
    cur ^= 1;
  }
  pre_last();          // epilogue operand loads (bias, residual) fly during the last K step's MFMAs
  compute(cur);
}

}  // namespace
