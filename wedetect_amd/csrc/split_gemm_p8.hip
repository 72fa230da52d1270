// split_gemm_p8.hip — fp16x3 GEMM for the big plain layers with pre-split operands (the ConvNeXt
// pointwise MLPs, mm_backbone.py:115-124): 256 x 256 output tile, K tiles of 32, eight waves in two
// row groups running half a phase apart, four phases per K tile.
//
// Why another structure.  The 128 x 128 direct-to-LDS kernel (split_gemm_pre.hip) pays one
// workgroup barrier and one full vmcnt(0) drain per 12 MFMAs and reads 8 ds_read_b128 per 12
// MFMAs; its matrix pipe is busy a third of the time.  Here a wave owns 128 x 64 outputs (eight
// 32 x 32 accumulators = 128 registers), so a K tile of 32 costs 24 ds_read_b128 per 48 MFMAs,
// and global -> LDS traffic per MFMA halves.  The K loop never drains the DMA queue:
//
//   * LDS (144 KB): two K-tile buffers of 48 KB, each cut into three 16 KB regions (128 rows x 128 B)
//       A0 / A1 = activation rows {0-63, 128-191} / {64-127, 192-255} of the tile (the first / second
//                 64 rows of each row group),  W1 = weight rows {64 wn + 32-63},
//     plus a ring of THREE 16 KB slots for W0 = weight rows {64 wn + 0-31} (K tile t lives in slot t % 3).
//   * a K tile is consumed in four phases, one 64 x 32 output quadrant of the wave per phase
//     (12 MFMAs = 2 row blocks x 2 k16 steps x {lo.hi, hi.lo, hi.hi}):
//       phase 1  read A0 (8 x ds_read_b128) + W0 (4)   quadrant (rows 0-63,  cols 0-31)
//       phase 2  read W1 (4)                           quadrant (rows 0-63,  cols 32-63)
//       phase 3  read A1 (8)                           quadrant (rows 64-127, cols 32-63)
//       phase 4  (W0 is still in registers)            quadrant (rows 64-127, cols 0-31)
//     One activation and two weight fragment sets (64 registers) next to the 128 accumulator registers (198 in
//     all; the persistent form 234, no scratch).  W0 keeps its three-slot ring from the form that re-read it in
//     phase 4 (same speed within noise, 4 more reads per K tile): a request two K tiles ahead never waits for a slot.
//     The per-accumulator MFMA sequence (k ascending, lo.hi -> hi.lo -> hi.hi inside a k16 step) is the
//     one of every other fp16x3 kernel: results are bit-identical to theirs.
//   * every phase also re-fills one region that went dead two phases earlier (tile t: phase 1: A1 of tile
//     t+1, 2: W0 of t+2, 3: A0 of t+2, 4: W1 of t+2): 16 one-KB global_load_lds_dwordx4 per region, two per
//     wave, issued from inline asm so that hipcc does not serialise them against the ds_reads.  A region is
//     read six or seven phases after it was requested; each wave retires its own requests with a COUNTED
//     s_waitcnt vmcnt(10) (the five newest regions stay in flight across the barriers) and never waits
//     vmcnt(0) in steady state.
//   * phase = [ds_reads, DMA issue, vmcnt] s_barrier [12 MFMAs] s_barrier.  The two row groups
//     (waves 0-3 / 4-7; waves w and w + 4 share a SIMD) are offset by one barrier, so a SIMD's
//     matrix pipe is fed by one wave while its partner reads and requests.  A region is re-filled
//     two phases after its last read: the other group's reads of it (issued up to one barrier later,
//     completed before its MFMAs) are over before the DMA can be issued.
//   * LDS rows are unpadded 128 B with the 16-byte slot XOR-swizzled by (row / 2) & 7 — applied on the
//     GLOBAL side of the DMA and on the ds_read address (LDS-DMA writes lane-linear); out-of-range
//     rows are clamped to the last valid row (their outputs are never stored), so no zero page.
//
// Tried and dropped (round 2, profiles/r02_p8_sched.txt): the same four phases software-pipelined INSIDE the wave —
// fragment registers used as two half sets (k16 step 0 / 1), the ds_reads of one step in flight behind the six MFMAs
// of the other (inline-asm reads, hand-counted lgkmcnt), one barrier per phase placed between the 9th and 10th MFMA,
// all eight waves in step (or the second row group's barrier three MFMAs later).  Bit-identical, no spills (208
// registers), and 7-8 % SLOWER (stage-3 pwconv2 321-333 us against 298): with both waves of a SIMD in the same
// position of the same stream, their read / DMA-issue bursts (an LDS-DMA instruction costs 60-185 issue cycles)
// coincide instead of hiding behind the partner's MFMAs.  The staggered two-barrier form below keeps one wave of
// every SIMD in its MFMA run while the other issues memory work, which is what the matrix pipe needs.
//
// The epilogue is the template parameter EPI: P8Store = the storing epilogues of split_gemm_impl.h (the VAR bits choose among them), or
// the argument struct of an epilogue that scores the product instead of storing it — retrieval max, best class, candidates, top-n,
// prompt groups, each defined in front of the kernel; their launch wrappers are at the end of this file (p8_score_launch.h declares them).
#include <stdlib.h>
#include "p8_score_launch.h"
#include "split_gemm_impl.h"
#include "topn_key.h"

long long wd_p8_workspace_floats();

namespace {

constexpr int P8_ROWB = 128, P8_REGION = 128 * P8_ROWB, P8_TILE = 3 * P8_REGION, P8_LDS = 2 * P8_TILE + 3 * P8_REGION;
constexpr int P8_A0 = 0, P8_W1 = P8_REGION, P8_A1 = 2 * P8_REGION, P8_W0RING = 2 * P8_TILE;   // W0 of K tile t: P8_W0RING + (t % 3) * P8_REGION

#define P8_KBARRIER() do { if (!(ABL & 8)) WD_WG_BARRIER(); } while (0)

// ABL: timing-only ablations for on-device diagnosis (WRONG results by construction; compiled only with
// -DWD_DEBUG_ABLATIONS, reachable through cfg 640 + ABL): 1 = no DMA in the K loop, 2 = no ds_reads in the K loop,
// 4 = no epilogue, 8 = no barriers in the K loop, 16 = both wave groups in step (no stagger).
//
// PERSIST (cfg 65): one workgroup per CU walks a contiguous range of (tile, K tile) work units instead of
// owning whole output tiles, so 400 tiles on 256 CUs cost 1.5625 tile times, not 2 (and the epilogues of
// different CUs stop happening in the same microseconds).  Round 4: the units are dealt to GANGS of ngrp workgroups,
// not to single workgroups.  The round-2/3 form gave every workgroup its own contiguous run of tiles: the column tiles
// of one row panel, which the tile form runs on neighbouring CUs of an XCD at the same time (the activation panel is
// fetched once and hits in L2 for the others), were then walked by ONE workgroup one after the other while its 31
// neighbours walked 31 other panels — 32 panels live per 4 MB L2 instead of 4, and the PMC pass says what that costs
// (profiles/r04_persist_pmc.txt, stage-3 pwconv1 / pwconv2: FETCH_SIZE 1.35 / 1.34 GB per launch against 0.33 / 0.58 GB
// for the tile form, TCC misses 2.4 x) — hidden by the Infinity Cache in a one-kernel loop, 12 % slower inside the step.
// A gang = ngrp workgroups with consecutive slots on one XCD; member j owns column tile j of every gang tile (= the ngrp
// column tiles of a row panel, exactly the tiles the tile form runs side by side) and all members share the same unit
// range, so the gang moves through K in step and the panel is fetched once.  The gang-tile list is cut into 8 chunks,
// one per XCD (workgroup b runs on XCD b % 8), each chunk's units are dealt evenly to the XCD's gangs.  A gang's
// range therefore starts and / or ends inside a tile.  The head of a tile [0, e) is computed FIRST, its raw accumulators are parked in the workspace and a
// flag is published (agent-scope release); whole tiles follow; LAST comes the tail [o, nk) of the tile the
// previous workgroup of the chain began: wait for that flag (set long before), acquire, reload the
// accumulators and continue the K loop where it stopped — the same MFMA chain, only carried by two CUs, so the
// result is bit-identical to the one-workgroup-per-tile kernels.  A workgroup waits only on the same member of the
// previous gang of its XCD chain (block b - 8 ngrp, dispatched earlier), and only at the very end of its own work; the
// first gang of a chain never waits.  Needs at least one whole gang tile per gang on every XCD.
constexpr long long P8_PARK_BYTES = 8ll * 32768;       // per workgroup: 8 accumulators x 512 lanes x 64 B
struct P8Persist {
  float* acc;            // [workgroup][512 lanes][128 floats]: parked accumulators of the tile a workgroup shares with its successor
  unsigned* flag;        // [workgroup]: 1 = parked; reset to 0 by the consumer
  const float* zero;     // 512 bytes of zeros
  int ntiles;            // gang tiles: row panels x column groups
};

constexpr int P8VAR_DIRECT = 8192;      // with SVAR_CSPLIT: the direct (no LDS transpose) hi/lo epilogue; GELU / no activation only

// ---- the epilogues that do not store the product: one argument struct each (the kernel's template parameter EPI and its argument
// `ep`) and a function  p8_*_epilogue(p, args, unscale, mw, nw, lane, acc[, patch])  for one wave's 128 x 64 piece of the tile (rows from mw,
// columns from nw), which the struct's run() hands on to.  PADS_COLUMN_TILES: the launch pads its column tiles to whole groups of eight
// and the kernel skips them.  A further mode adds its struct and function here and a launcher below; the kernel does not change.
struct P8Store { static constexpr bool PADS_COLUMN_TILES = false; };

// ---- retrieval scoring on this kernel (round 5; wd_retrieval_max_split, retrieval_metric.py:367-377) ----------------------
// The GEMM is run with the operand ROLES SWAPPED: the text bank is the "activation" operand (p.a, p.m = classes of this
// launch) and the region rows of all images, back to back, are the "weight" operand (wsp, p.n = region rows).  In the
// accumulator layout of v_mfma_f32_32x32x16 the activation row is the LANE and the weight row the REGISTER, so a lane then
// holds, for ONE class, 32 of the wave's 64 region rows: the max over an image's regions is 31 in-register v_max plus one
// lane exchange (the form on the 256 x 128 ping-pong kernel — classes in registers, rows in lanes — paid a five-step
// segmented shuffle reduction PER VALUE: ~28 VALU instructions per accumulator element).  sigmoid is monotone, so it is
// applied once to the maximum of the affine logits instead of to every (row, class): max_r s(x_r) = s(max_r x_r).
// Tile order: region-row tiles in groups of eight, four bank blocks x eight row tiles live per XCD at a time (the gang
// order of the MLP launches): per 32 tiles an L2 fetches 12 operand panels instead of 33, the bank streams from HBM once per
// row-tile group (five times for 32 images x 300 regions), the region rows (29 MB) stay in the Infinity Cache.
struct P8RetrMax {
  static constexpr bool PADS_COLUMN_TILES = true;
  const float* scale;    // [region rows]: logit scale, applied as exp(scale)
  const float* bias;     // [region rows]
  const int* count;      // [images]: valid rows of an image (the first count[i] of its rows_per_img)
  float* out;            // [images][ldo], zero-filled: max over an image's valid rows of sigmoid(<e, t> exp(scale) + bias)
  int rows_per_img, ldo;
  template <int TM, int TN> static __device__ __forceinline__ void run(const WdConvGemm& p, const P8RetrMax& a, float unscale, int mw, int nw, int lane,
      const f32x16 (&acc)[TM][TN], float* patch) { p8_retr_epilogue(p, a, unscale, mw, nw, lane, acc); }
};
template <int TM, int TN>
__device__ __forceinline__ void p8_retr_epilogue(const WdConvGemm& p, const P8RetrMax& rt, float unscale, int mw, int nw, int lane,
                                                 const f32x16 (&acc)[TM][TN]) {
  const int nrows = p.n;
  if (nw >= nrows || mw >= p.m) return;                            // wave-uniform
  const int half = lane >> 5;
  if (p.range_flag) {                                              // an fp16 half that overflowed to inf: inf / NaN accumulators
    bool bad = false;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          bad |= wd_any_nonfinite4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
    if (bad) *p.range_flag = 1u;
  }
  // this lane's rows: row(j, r) = nw + 32 j + 8 (r >> 2) + 4 half + (r & 3).  Their exp(scale) * unscale and bias are
  // loaded per (image, j) — 32 live registers next to the 128 accumulators; holding all 64 spilled (the build refuses scratch)
  const float ninf = -__builtin_inff();
  const int rpi = rt.rows_per_img;
  const int last = (nw + 63 < nrows ? nw + 63 : nrows - 1);
  const int img_last = last / rpi;
  for (int img = nw / rpi; img <= img_last; ++img) {               // usually one image, two where a wave's 64 rows straddle
    int cnt = rt.count[img];
    cnt = cnt < rpi ? cnt : rpi;
    if (cnt <= 0) continue;
    const int d = nw - img * rpi + 4 * half;                       // row(j, r) - first row of the image = d + const(j, r)
    float v[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) v[i] = ninf;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      float e_[16], b_[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int base = nw + 32 * j + 8 * g + 4 * half;
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, b4 = {0.f, 0.f, 0.f, 0.f};
        if (base + 3 < nrows) {
          s4 = *reinterpret_cast<const f32x4*>(rt.scale + base);
          b4 = *reinterpret_cast<const f32x4*>(rt.bias + base);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (base + q < nrows) { s4[q] = rt.scale[base + q]; b4[q] = rt.bias[base + q]; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool in = (unsigned)(d + 32 * j + 8 * g + q) < (unsigned)cnt;
          e_[4 * g + q] = in ? expf(s4[q]) * unscale : 0.0f;       // rows of other images / beyond the count: 0 * acc - inf
          b_[4 * g + q] = in ? b4[q] : ninf;
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) v[i] = fmaxf(v[i], fmaf(acc[i][j][r], e_[r], b_[r]));
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float o = __shfl_xor(v[i], 32, 64);                    // the other four rows of every group of eight
      const float m = fmaxf(v[i], o);
      const int cls = mw + 32 * i + (lane & 31);
      if ((i & 1) == half && cls < p.m && m > ninf)                // sigmoid > 0 and out starts at 0: uint order = float order
        atomicMax(reinterpret_cast<unsigned int*>(rt.out + (size_t)img * rt.ldo + cls), __float_as_uint(wd_sigmoid(m)));
    }
  }
}

// ---- what the four epilogues of the similarity launch share ---------------------------------------------------------------------
// Operands NOT swapped: in the accumulator layout the region row is the LANE (lane & 31) and the class the REGISTER — element
// e = 16 j + 4 g + q of row tile i is register 4 g + q of acc[i][j] and column p8_col(e) past the lane's first one,
// c_lane = nw + 4 (lane >> 5) — so a lane holds 32 of the wave's 64 classes for each of its TM rows, and both half-waves hold the
// same 32 rows of tile i.

// The score of accumulator element v of a row: the expressions of the materialising epilogue (epi_quad<WD_ACT_NONE, true>), so the
// bits it would have stored.
__device__ __forceinline__ float p8_score(float v, float unscale, const EpiRow& er) {
  float x = fmaf(v, unscale, 0.0f);                                // unscale is a power of two: exact
  x = fmaf(x, er.oscale, er.obias);
  return wd_sigmoid_fast(x);
}

__device__ __forceinline__ unsigned long long p8_umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned p8_col(int e) { return (unsigned)(32 * (e >> 4) + 8 * ((e >> 2) & 3) + (e & 3)); }

// key of element e = score bits << 32 | (0xFFFFFFFF - class), inv0 = 0xFFFFFFFF - cls_offset - c_lane: scores are >= +0, so the
// unsigned order of the keys is (score ascending, class descending) and a 64-bit max keeps the LOWEST class among equal scores
__device__ __forceinline__ unsigned long long p8_key(unsigned score_bits, unsigned inv0, int e) {
  return ((unsigned long long)score_bits << 32) | (unsigned long long)(inv0 - p8_col(e));
}

// The 32 scores of (lane, row tile i), a = acc[i]: each(e, score, column valid) per element, e ascending; returns whether a valid
// quad of the row holds a non-finite accumulator (an fp16 half that overflowed).  Fully unrolled: e and every register index are
// compile-time constants in the caller, nothing is indexed dynamically.  P8Sparse and P8Topn open with it; P8Best writes the same walk
// out (one register less), P8Group has another shape.
template <int TN, typename F>
__device__ __forceinline__ bool p8_score_tile(const WdConvGemm& p, const f32x16 (&a)[TN], float unscale, const EpiRow& er, bool row_ok,
                                              int c_lane, F&& each) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cq = c_lane + 32 * j + 8 * g;
      if (cq < p.n && row_ok) bad |= wd_any_nonfinite4(a[j][4 * g], a[j][4 * g + 1], a[j][4 * g + 2], a[j][4 * g + 3]);
#pragma unroll
      for (int q = 0; q < 4; ++q) each(16 * j + 4 * g + q, p8_score(a[j][4 * g + q], unscale, er), cq + q < p.n);
    }
  return bad;
}

// ---- best class per region row on this kernel (wd_best_similarity_split, include/wedetect_hip_best.h) -----------------------
// The similarity launch with another epilogue.  Every valid element gets the score the materialising epilogue would have stored
// (epi_quad<WD_ACT_NONE, true>: fmaf(v, unscale, 0), fmaf(x, oscale, obias), wd_sigmoid_fast — the same expressions, so the same
// bits), packed as p8_key.  31 in-register maxima, one exchange with the other half-wave, then ONE 64-bit vector atomic max per
// (row, wave) into key[row] — max is order-independent: the result does not depend on the tile order or on how the bank is cut into
// launches.  A row with a non-finite accumulator (an fp16 half that overflowed) gets NaN score bits, which beat every score: the
// unpacked score is then non-finite and wd_topk_candidates reports the image.
struct P8Best {
  static constexpr bool PADS_COLUMN_TILES = false;
  unsigned long long* key;     // [region rows]
  int cls_offset;              // the class of the launch's first bank row
  template <int TM, int TN> static __device__ __forceinline__ void run(const WdConvGemm& p, const P8Best& a, float unscale, int mw, int nw, int lane,
      const f32x16 (&acc)[TM][TN], float* patch) { p8_best_epilogue(p, a, unscale, mw, nw, lane, acc); }
};
template <int TM, int TN>
__device__ __forceinline__ void p8_best_epilogue(const WdConvGemm& p, const P8Best& a, float unscale, int mw, int nw, int lane,
                                                 const f32x16 (&acc)[TM][TN]) {
  if (mw >= p.m || nw >= p.n) return;                              // wave-uniform
  unsigned long long* __restrict__ key = a.key;
  const int half = lane >> 5;
  const int c_lane = nw + 4 * half;
  const unsigned inv0 = 0xFFFFFFFFu - (unsigned)a.cls_offset - (unsigned)c_lane;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = mw + 32 * i + (lane & 31);
    const EpiRow er = epi_row<true>(p, m < p.m ? m : p.m - 1);      // rows past the end: what the padded buffer holds there is not ours to judge
    unsigned long long best = 0ull;                                // 0 = no class seen
    bool bad = false;        // p8_score_tile written out (through it this kernel needs 215 registers, so 214): a change there is mirrored HERE
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cq = c_lane + 32 * j + 8 * g;
        if (cq < p.n && m < p.m) bad |= wd_any_nonfinite4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned long long kq = p8_key(__float_as_uint(p8_score(acc[i][j][4 * g + q], unscale, er)), inv0, 16 * j + 4 * g + q);
          best = p8_umax64(best, cq + q < p.n ? kq : 0ull);
        }
      }
    if (bad) {
      if (p.range_flag) *p.range_flag = 1u;
      best = (0x7FC00000ull << 32) | (unsigned long long)inv0;
    }
    const unsigned olo = __shfl_xor((unsigned)best, 32, 64), ohi = __shfl_xor((unsigned)(best >> 32), 32, 64);
    best = p8_umax64(best, ((unsigned long long)ohi << 32) | olo);
    if ((i & 1) == half && m < p.m && best != 0ull) atomicMax(key + m, best);
  }
}

// ---- candidates above a threshold on this kernel (wd_sparse_similarity_split, include/wedetect_hip_sparse.h) ----------------
// Every valid element gets the score the materialising epilogue would have stored (the same three expressions, so the same bits);
// the 32 scores of (lane, i) replace their accumulators (every index is a compile-time constant: the loops are unrolled, nothing
// is indexed dynamically) and a 32-bit mask records which of them pass score > thr.
// Slots: the lanes' popcounts become offsets by an inclusive wave prefix sum (six shuffles); where the wave's 32 rows lie inside ONE
// image, lane 0 draws the wave's total from state[b][0] with one vector atomic and broadcasts the base — one atomic per
// (wave, group) however many elements pass.  A group that straddles two images (rows_per_img = 8400 is no multiple of 32) lets
// every lane with candidates draw its own.  A wave without candidates issues no atomic and skips the stores.  Keys
// (~score bits << 32 | flat index) go out as plain 8-byte vector stores to list[b][slot] while slot < list_cap; the counter runs
// on past the cap, which is how wd_sparse_select sees an overflow.
struct P8Sparse {
  static constexpr bool PADS_COLUMN_TILES = false;
  unsigned long long* list;    // [images][list_cap]
  int* state;                  // [images][2]: candidates seen, non-finite seen
  int rows_per_img;
  int cls_offset, n_cls_total; // the class of the launch's first bank row; classes of the whole bank (the pitch of the flat index)
  int list_cap;
  float thr;
  template <int TM, int TN> static __device__ __forceinline__ void run(const WdConvGemm& p, const P8Sparse& a, float unscale, int mw, int nw, int lane,
      const f32x16 (&acc)[TM][TN], float* patch) { p8_sparse_epilogue(p, a, unscale, mw, nw, lane, acc); }
};
template <int TM, int TN>
__device__ __forceinline__ void p8_sparse_epilogue(const WdConvGemm& p, const P8Sparse& a, float unscale, int mw, int nw, int lane,
                                                   const f32x16 (&acc)[TM][TN]) {
  static_assert(TN * 16 == 32, "one 32-bit pass mask per (lane, row tile)");
  if (mw >= p.m || nw >= p.n) return;                              // wave-uniform
  unsigned long long* __restrict__ list = a.list;
  int* __restrict__ state = a.state;
  const int rpi = a.rows_per_img;
  const unsigned cap = (unsigned)a.list_cap;
  const float thr = a.thr;
  const int half = lane >> 5;
  const int c_lane = nw + 4 * half;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m_first = mw + 32 * i;
    if (m_first >= p.m) break;                                     // wave-uniform
    const int m_last = m_first + 31 < p.m ? m_first + 31 : p.m - 1;
    const int b_first = m_first / rpi;
    const bool one_image = m_last / rpi == b_first;                // wave-uniform
    const int m = m_first + (lane & 31);
    const bool row_ok = m < p.m;
    const int mc = row_ok ? m : p.m - 1;                           // rows past the end: what the padded buffer holds there is not ours to judge
    const EpiRow er = epi_row<true>(p, mc);
    const int b = one_image ? b_first : mc / rpi;
    const unsigned flat0 = (unsigned)(mc - b * rpi) * (unsigned)a.n_cls_total + (unsigned)a.cls_offset + (unsigned)c_lane;
    float sc[TN * 16];
    unsigned mask = 0u;
    const bool bad = p8_score_tile(p, acc[i], unscale, er, row_ok, c_lane, [&](int e, float x, bool col_ok) {
      sc[e] = x;
      mask |= (row_ok && col_ok && x > thr) ? (1u << e) : 0u;
    });
    if (bad) {
      if (p.range_flag) *p.range_flag = 1u;
      state[2 * b + 1] = 1;                                        // sticky, benign race
    }
    const unsigned cnt = (unsigned)__popc(mask);
    if (__ballot(cnt != 0u) == 0ull) continue;                     // wave-uniform: nothing passes in this group
    unsigned pos;
    if (one_image) {
      unsigned incl = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        incl += lane >= o ? up : 0u;
      }
      const unsigned total = __shfl(incl, 63, 64);
      unsigned base = 0u;
      if (lane == 0) base = (unsigned)atomicAdd(state + 2 * b_first, (int)total);
      base = __shfl(base, 0, 64);
      pos = base + incl - cnt;
    } else {
      pos = cnt ? (unsigned)atomicAdd(state + 2 * b, (int)cnt) : 0u;
    }
    unsigned long long* __restrict__ lb = list + (size_t)b * cap;
#pragma unroll
    for (int e = 0; e < TN * 16; ++e) {
      if ((mask >> e) & 1u) {
        if (pos < cap) lb[pos] = ((unsigned long long)(~__float_as_uint(sc[e])) << 32) | (unsigned long long)(flat0 + p8_col(e));
        ++pos;
      }
    }
  }
}

// ---- the n best classes per region row on this kernel (wd_topn_similarity_split, include/wedetect_hip_topn.h) ----------------
// The keys of P8Best.  A lane reads its row's last slot ONCE (device scope) as the bound, marks which of its 32 keys lie above it
// (after the first column tiles of a row almost none do, and a wave without one leaves here), then selects the marked keys in
// descending order — one pass over the 32 registers per key, every index a compile-time constant — and offers the t-th of them to
// the row at slot t (wd_topn_offer, topn_key.h), reading the bound again in between: the other column tiles of the row raise it.
// A row with a non-finite accumulator gets NaN score bits in slot 0, as in P8Best.
struct P8Topn {
  static constexpr bool PADS_COLUMN_TILES = false;
  unsigned long long* key;     // [region rows][n_top]
  const float* row_scale;      // [region rows]: the per-row affine, applied as exp(row_scale); both null: the level affine of p
  const float* row_bias;
  int cls_offset;              // the class of the launch's first bank row
  int n_top;
  template <int TM, int TN> static __device__ __forceinline__ void run(const WdConvGemm& p, const P8Topn& a, float unscale, int mw, int nw, int lane,
      const f32x16 (&acc)[TM][TN], float* patch) { p8_topn_epilogue(p, a, unscale, mw, nw, lane, acc); }
};
template <int TM, int TN>
__device__ __forceinline__ void p8_topn_epilogue(const WdConvGemm& p, const P8Topn& a, float unscale, int mw, int nw, int lane,
                                                 const f32x16 (&acc)[TM][TN]) {
  static_assert(TN * 16 == 32, "one 32-bit mask per (lane, row tile)");
  if (mw >= p.m || nw >= p.n) return;                              // wave-uniform
  unsigned long long* key = a.key;
  const int n_top = a.n_top;
  const int half = lane >> 5;
  const int c_lane = nw + 4 * half;
  const unsigned inv0 = 0xFFFFFFFFu - (unsigned)a.cls_offset - (unsigned)c_lane;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    if (mw + 32 * i >= p.m) break;                                 // wave-uniform
    const int m = mw + 32 * i + (lane & 31);
    const bool row_ok = m < p.m;
    const int mc = row_ok ? m : p.m - 1;                           // rows past the end: what the padded buffer holds there is not ours to judge
    EpiRow er = epi_row<true>(p, mc);
    if (a.row_scale) { er.oscale = expf(a.row_scale[mc]); er.obias = a.row_bias[mc]; }    // wd_topn_affine_score: the same two expressions
    unsigned long long* slot = key + (size_t)mc * n_top;
    unsigned long long bound = wd_topn_bound(slot, n_top);
    unsigned sc[TN * 16];
    unsigned mask = 0u;
    const bool bad = p8_score_tile(p, acc[i], unscale, er, row_ok, c_lane, [&](int e, float x, bool col_ok) {
      sc[e] = __float_as_uint(x);
      mask |= (row_ok && col_ok && p8_key(sc[e], inv0, e) > bound) ? (1u << e) : 0u;
    });
    if (bad) {
      if (p.range_flag) *p.range_flag = 1u;
      atomicMax(slot, (0x7FC00000ull << 32) | (unsigned long long)inv0);
      mask = 0u;
    }
    if (__ballot(mask != 0u) == 0ull) continue;                    // wave-uniform: nothing of this group reaches a list
    unsigned long long prev = ~0ull;
    for (int t = 0; t < n_top && mask != 0u; ++t) {
      unsigned long long best = 0ull;
#pragma unroll
      for (int e = 0; e < TN * 16; ++e) {
        const unsigned long long ke = p8_key(sc[e], inv0, e);
        best = (((mask >> e) & 1u) && ke < prev && ke > best) ? ke : best;
      }
      if (t > 0) bound = p8_umax64(bound, wd_topn_bound(slot, n_top));
      if (best <= bound) break;                                    // descending: no later key of this lane is above the bound either
      wd_topn_offer(slot, n_top, t, best, bound);
      prev = best;
    }
  }
}

// ---- the best prompt of every class on this kernel (wd_group_similarity_split, include/wedetect_hip_groups.h) -----------------
// The layout and the scores of P8Best; the 32 bank rows nw + 32 j .. + 31 of accumulator tile (i, j) are ONE BIN of the packing
// (cls_offset and nw are multiples of 32), split between lane L and lane L ^ 32.  Which rows of a bin belong to which class depends
// on the column only: wave-uniform.
// Per bin (j): the wave reads the bin's classes [g0, g0 + ng) and its 32 group_of words (uniform loads).  The (row, class) pairs
// of a 32-row tile are dealt in passes of rp = min(32, 64 / ng) rows x ng classes: lane = (row r0 of the pass, class k = lane % ng),
// the SAME class in every pass, so a lane counts the columns in front of class g0 + k and those of it, (start, ln), once per bin;
// the longest class of the bin bounds the read loop.
// Per (i, j): every lane writes its 16 SCORES (p8_score per element: the materialised bits) to the wave's 32 x 36-float patch —
// the patch of the materialising epilogue, transposed the same way — then, per pass, a lane reads the columns of its class in its
// row from the patch, four independent reads at a time (a shorter class re-reads its last column: max is idempotent), and stores
// the maximum at out[row][g0 + k].  Consecutive lanes store consecutive classes of a row: row segments of ng floats, every element
// written exactly once, no atomics, nothing cleared.  (A first form dealt the pairs 64 per pass with the class changing per
// pass — a lane exchange and a serial read loop in every pass: 3.53 ms, this form 3.02 ms, against 2.39 ms of the materialising launch on the LVIS
// plan, profiles/prompt_groups.txt.)  A non-finite accumulator of (row, bin) raises the range flag and turns the row's 32 patch
// entries into NaN, so every class of the bin gets NaN in that row (fmaxf(NaN, NaN) = NaN).
// No register is indexed dynamically: i, j, g, q are unrolled, the pass loop touches the patch only.
struct P8Group {
  static constexpr bool PADS_COLUMN_TILES = false;
  const int* group_of;         // [bank rows of the whole bank]: the class of a bank row, non-decreasing
  const int* bin_first;        // [bins + 1]: the first class of a bin
  float* out;                  // [region rows][ldg]
  int cls_offset;              // the bank row of the launch's first one, a multiple of 32
  int ldg, n_groups;
  template <int TM, int TN> static __device__ __forceinline__ void run(const WdConvGemm& p, const P8Group& a, float unscale, int mw, int nw, int lane,
      const f32x16 (&acc)[TM][TN], float* patch) { p8_group_epilogue(p, a, unscale, mw, nw, lane, acc, patch); }
};
template <int TM, int TN>
__device__ __forceinline__ void p8_group_epilogue(const WdConvGemm& p, const P8Group& a, float unscale, int mw, int nw, int lane,
                                                  const f32x16 (&acc)[TM][TN], float* patch) {
  if (mw >= p.m || nw >= p.n) return;                              // wave-uniform
  const int half = lane >> 5, l31 = lane & 31;
  const float qnan = __uint_as_float(0x7FC00000u);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int c0 = nw + 32 * j;                                    // first bank row of the bin, in this launch
    if (c0 >= p.n) break;                                          // wave-uniform (p.n is a multiple of 32: a bin is in or out)
    const int abin = (a.cls_offset + c0) >> 5;
    const int g0 = a.bin_first[abin];
    int ng = a.bin_first[abin + 1] - g0;
    ng = (g0 < 0 || ng < 0) ? 0 : (ng > 32 ? 32 : ng);             // a table that is no plan's: nothing is stored
    ng = __builtin_amdgcn_readfirstlane(ng);
    if (ng == 0) continue;
    // the (row, class) pairs of a pass: rp = min(32, 64 / ng) rows of ng classes; lane = (row r0 of the pass, class k), the same
    // class in every pass, so its column range is found once per bin
    const int magic = (65536 + ng - 1) / ng;                       // x / ng = (x * magic) >> 16 for x < 1024, ng <= 32
    const int rp = ng <= 2 ? 32 : (64 * magic) >> 16;
    const int r0 = (lane * magic) >> 16;
    const int k = lane - r0 * ng;
    const int* __restrict__ go = a.group_of + a.cls_offset + c0;
    const int mine = g0 + k;
    int start = 0, end = 0, run = 0, maxl = 1, prev = 0;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      const int gc = go[c];
      start += gc < mine ? 1 : 0;
      end += gc <= mine ? 1 : 0;
      run = (c > 0 && gc == prev) ? run + 1 : 1;
      maxl = run > maxl ? run : maxl;
      prev = gc;
    }
    maxl = __builtin_amdgcn_readfirstlane(maxl);
    const int ln = end - start, last = ln > 0 ? ln - 1 : 0;        // columns of class g0 + k: [start, start + ln); ln = 0: a table that is no plan's
    const bool lane_ok = r0 < rp && ln > 0 && g0 + k < a.n_groups;
    const int o1 = last < 1 ? last : 1, o2 = last < 2 ? last : 2, o3 = last < 3 ? last : 3;
    const int lane_off = (r0 < 32 ? r0 : 0) * EPI_LDT + start;     // start + last <= 31; ln = 0: start <= 32, inside the 36-float pitch
    float* const outk = a.out + g0 + k;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m_first = mw + 32 * i;
      if (m_first >= p.m) break;                                   // wave-uniform
      const int m = m_first + l31;
      const bool row_ok = m < p.m;
      const EpiRow er = epi_row<true>(p, row_ok ? m : p.m - 1);     // rows past the end: what the padded buffer holds there is not ours to judge
      bool bad = false;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        bad |= wd_any_nonfinite4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
      bad = bad && row_ok;
      bad = bad || (__shfl_xor((int)bad, 32, 64) != 0);            // the other 16 bank rows of the bin
      if (bad && p.range_flag) *p.range_flag = 1u;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 s;
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = bad ? qnan : p8_score(acc[i][j][4 * g + q], unscale, er);
        *reinterpret_cast<f32x4*>(patch + l31 * EPI_LDT + 8 * g + 4 * half) = s;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int rb = 0; rb < 32; rb += rp) {
        const int r = rb + r0;                                     // row of the tile
        const float* src = patch + (r < 32 ? rb : 0) * EPI_LDT + lane_off;
        // four independent reads (a class of fewer columns re-reads its last one: max is idempotent), then the rare long classes
        const float v0 = src[0], v1 = src[o1], v2 = src[o2], v3 = src[o3];
        float v = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
        for (int t = 4; t < maxl; t += 4) {
          const float w0 = src[t < last ? t : last], w1 = src[t + 1 < last ? t + 1 : last], w2 = src[t + 2 < last ? t + 2 : last],
                      w3 = src[t + 3 < last ? t + 3 : last];
          v = fmaxf(v, fmaxf(fmaxf(w0, w1), fmaxf(w2, w3)));
        }
        const int mm = m_first + r;
        if (lane_ok && r < 32 && mm < p.m) outk[(size_t)mm * a.ldg] = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

template <int VAR, typename EPI = P8Store, int ABL = 0, bool PERSIST = false>
__global__ void __launch_bounds__(512, 2)
split_gemm_p8_kernel(const WdConvGemm p, const unsigned char* __restrict__ wsp, int k16, float unscale, int nbn,
                     int vec_c, int vec_res, int vec_bias, int ngrp, int nbm, const P8Persist ps, int stagger,
                     int arows, int wrows, const EPI ep) {
  constexpr int TM = 4, TN = 2, BM = 256, BN = 256, ROWB = P8_ROWB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int group = wave >> 2, wn = wave & 3;
  const int nk = p.k >> 5;
  const int gsz = ngrp * nbm;

  // Experiment ($WD_P8_STAGGER, tile form, -DWD_DEBUG_ABLATIONS builds; measured: no gain, profiles/r05_p8_epilogue_ablation.txt): every tile costs the same, so all CUs reach their epilogues — 256 KB of stores each —
  // in the same microseconds of every round.  Delaying the first tile of every other CU by `stagger` x ~4 us takes the two
  // halves of the chip out of phase for the whole launch.
  if (!PERSIST && stagger > 0 && blockIdx.x < 256u && ((blockIdx.x >> 3) & 1))
    for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);
  // ---- work assignment
  int seg_first_tile, seg_o, seg_last_tile, seg_e;   // units [first_tile * nk + o, last_tile * nk + e)
  if (PERSIST) {
    // gang = slot / ngrp, member = slot % ngrp; gang tile gt <-> tiles gt * ngrp + member of the tile form's list
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3, per = (gridDim.x >> 3) / ngrp, gang = slot / ngrp;
    const long long t0 = (long long)ps.ntiles * xcd / 8, t1 = (long long)ps.ntiles * (xcd + 1) / 8;
    const long long units = (t1 - t0) * nk;
    const long long u0 = t0 * nk + units * gang / per, u1 = t0 * nk + units * (gang + 1) / per;
    seg_first_tile = (int)(u0 / nk); seg_o = (int)(u0 - (long long)seg_first_tile * nk);
    seg_last_tile = (int)(u1 / nk); seg_e = (int)(u1 - (long long)seg_last_tile * nk);
  } else {
    // wd_xcd_tile (gemm_prims.h), spelled out: through the call hipcc assigns this kernel's scalar registers differently
    int tile = blockIdx.x;
    const int nwg = gridDim.x, xcd = tile & 7, idx = tile >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    seg_first_tile = tile; seg_o = 0; seg_last_tile = tile + 1; seg_e = 0;
  }
  // segments in execution order: [head of the last tile] [whole tiles] [tail of the first tile]
  const int has_head = seg_e > 0, has_tail = seg_o > 0;
  const int full0 = seg_first_tile + has_tail, nfull = seg_last_tile - full0;
  const int nseg = has_head + nfull + has_tail;

  const unsigned char* abase = reinterpret_cast<const unsigned char*>(p.a);
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem_raw;
  const unsigned dma_dst = lds0 + wave * 1024;                   // + region offset + j * 8192: instruction j of wave w fills slots [(w + 8 j) * 8, + 8)
  // ---- fragment addresses (byte offsets inside a region): slot * 128 + ((logical ^ f(slot)) << 4), logical =
  // 4 ks + 2 (hi / lo) + hsel.  With g = hsel ^ f(slot) the four (ks, hi / lo) variants of a lane are
  // base ^ {0, 32, 64, 96}, base = slot * 128 + (g << 4): ONE register per operand (the second activation row
  // block is + 4096), the variants cost one v_xor each.
  const int hsel = lane >> 5;
  int abase_off, wbase_off;
  {
    const int slot = group * 64 + (lane & 31);
    abase_off = slot * ROWB + ((hsel ^ ((slot >> 1) & 7)) << 4);
  }
  {
    const int slot = wn * 32 + (lane & 31);
    wbase_off = slot * ROWB + ((hsel ^ ((slot >> 1) & 7)) << 4);
  }

  // lane part of the DMA source offset: row (lane >> 3) of the 8-row group + the swizzled 16-byte chunk.  With slots
  // dealt as (wave + 8 j) * 8 + r8 the swizzle term f(slot) = ((wave & 1) * 4 + (r8 >> 1)) is the same for both DMAs.
  unsigned la, lw;
  {
    const int r8 = lane >> 3;
    const int logical = (lane & 7) ^ (((wave & 1) << 2) | (r8 >> 1));
    const int memchunk = (logical & ~3) | ((logical & 1) << 1) | ((logical >> 1) & 1);
    la = (unsigned)r8 * (unsigned)p.lda * 4u + memchunk * 16;
    lw = (unsigned)r8 * (unsigned)k16 * 4u + memchunk * 16;
  }

  for (int sg = 0; sg < nseg; ++sg) {
    // which piece: head (park the accumulators), whole tile, or tail (resume from parked accumulators)
    const bool is_head = has_head && sg == 0;
    const bool is_tail = has_tail && sg == nseg - 1;
    int tile = is_head ? seg_last_tile : (is_tail ? seg_first_tile : full0 + sg - has_head);
    if (PERSIST) tile = tile * ngrp + (int)(blockIdx.x >> 3) % ngrp;
    const int kb = is_tail ? seg_o : 0;
    const int nks = (is_head ? seg_e : nk) - kb;                  // K tiles of this piece (>= 1)
    const int grp = tile / gsz, rem = tile - grp * gsz;
    const int bm = rem / ngrp, bn = grp * ngrp + (rem - bm * ngrp);
    const int m0 = bm * BM, n0 = bn * BN;
    if (EPI::PADS_COLUMN_TILES && n0 >= p.n) continue;           // column tiles padded to whole groups of eight: nothing to do

    // request K tile kt (relative to kb) of one operand region into LDS offset `reg` (buffer / ring slot included):
    // two 1 KB DMAs per wave.  half: 0 = A0 / W0, 1 = A1 / W1.  The 8-row group's first row is wave-uniform and rides
    // on the scalar base together with the K offset; the lane part (la / lw) never changes.
    auto stage = [&](int kt, int reg, bool is_w, int half) {
      if (ABL & 1) return;
      const unsigned char* base = is_w ? wsp : abase;
      const unsigned pitch = (unsigned)(is_w ? k16 : p.lda) * 4u;
      // arows / wrows: rows the operand BUFFERS hold, whole groups of eight (= p.m / p.n for the plain launches, which require
      // multiples of eight; the similarity launches and the retrieval pad their buffers instead)
      const int limit = (is_w ? wrows : arows) - 8;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int row = is_w ? n0 + (2 * j + (wave >> 2)) * 64 + (wave & 3) * 8 + half * 32 : m0 + j * 128 + wave * 8 + half * 64;
        row = row < limit ? row : limit;                            // whole groups past the end re-read the last one
        const unsigned char* src = base + (size_t)row * pitch + (size_t)(kb + kt) * ROWB;
        wd_lds_dma_sbase(dma_dst + reg + j * 8192, is_w ? lw : la, src);
      }
    };

    f32x16 acc[TM][TN];
    // ---- prologue: K tiles 0 and 1 of the piece (the previous piece's epilogue is done with the LDS)
    WD_WG_BARRIER();
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
      if (kt < nks) {
        stage(kt, kt * P8_TILE + P8_A0, false, 0);
        stage(kt, P8_W0RING + kt * P8_REGION, true, 0);
        stage(kt, kt * P8_TILE + P8_W1, true, 1);
        stage(kt, kt * P8_TILE + P8_A1, false, 1);
      }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    // The tail of a tile resumes from the accumulators its head parked (written by the previous workgroup of the
    // chain at the START of its work).  They are NOT loaded here: each phase of the piece's first K tile loads the
    // two accumulators it is about to use (ldacc below) — 128 live accumulator registers from this point on make
    // hipcc spill inside the K loop, accumulators that become live one pair per phase do not.
    const unsigned char* park_src = nullptr;
    if (PERSIST && is_tail) {
      const int prev = blockIdx.x - 8 * ngrp;
      if (t == 0) {
        while (__hip_atomic_load(ps.flag + prev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 1u) __builtin_amdgcn_s_sleep(8);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      __syncthreads();
      park_src = reinterpret_cast<const unsigned char*>(ps.acc) + (size_t)prev * P8_PARK_BYTES + (unsigned)t * 512u;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    WD_WG_BARRIER();
    if (group == 1 && !(ABL & 24)) WD_WG_BARRIER();                // the second row group runs one barrier behind

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    h8 xh[2][2] = {}, xl[2][2] = {}, wh[2] = {}, wl[2] = {};       // activation fragments [row block][k16 step]; weights [k16 step]
    h8 w0h[2] = {}, w0l[2] = {};                                   // W0 stays in registers from phase 1 to phase 4
    auto read_a = [&](const unsigned char* region) {
      if (ABL & 2) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) asm volatile("" : "+v"(xh[i][ks]), "+v"(xl[i][ks]));
        return;
      }
      int b = abase_off;
      asm volatile("" : "+v"(b));                                  // keep the xor variants out of long-lived registers
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          xh[i][ks] = *reinterpret_cast<const h8*>(region + i * 4096 + (b ^ (ks * 64)));
          xl[i][ks] = *reinterpret_cast<const h8*>(region + i * 4096 + (b ^ (ks * 64 + 32)));
        }
    };
    auto read_w = [&](const unsigned char* region, h8 (&fh)[2], h8 (&fl)[2]) {
      if (ABL & 2) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) asm volatile("" : "+v"(fh[ks]), "+v"(fl[ks]));
        return;
      }
      int b = wbase_off;
      asm volatile("" : "+v"(b));
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        fh[ks] = *reinterpret_cast<const h8*>(region + (b ^ (ks * 64)));
        fl[ks] = *reinterpret_cast<const h8*>(region + (b ^ (ks * 64 + 32)));
      }
    };
    // 12 MFMAs of one quadrant: two 32 x 32 accumulators
    auto quadrant = [&](f32x16& c0, f32x16& c1, const h8 (&fh)[2], const h8 (&fl)[2]) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[ks], xh[0][ks], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[ks], xh[1][ks], c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks], xl[0][ks], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks], xl[1][ks], c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks], xh[0][ks], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[ks], xh[1][ks], c1, 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    };

    // One K tile = four phases.  Counted waits: in steady state the five newest region requests (10 DMA
    // instructions of this wave) stay in flight; the last two K tiles request less, so less may be left
    // outstanding (TAIL 1 = tile nks - 2, TAIL 2 = tile nks - 1).  S1 / S234: whether phase 1 / phases 2-4 request a
    // region (tile 0's phase 1 does not: the prologue already did; the last tiles have nothing left to request) —
    // compile-time, so the loop body is branch-free.  w0s = W0 ring slot of this K tile (kt % 3).
#define P8_WAIT(a, b, c)                                                                       \
    do {                                                                                         \
      if constexpr (TAIL == 0) asm volatile("s_waitcnt vmcnt(" #a ")" ::: "memory");             \
      else if constexpr (TAIL == 1) asm volatile("s_waitcnt vmcnt(" #b ")" ::: "memory");        \
      else asm volatile("s_waitcnt vmcnt(" #c ")" ::: "memory");                                 \
    } while (0)
    // accumulators a0 = i0 * TN + j0 and a1 of this lane <- parked block (64 bytes each), loads + wait in one statement
    auto ldacc = [&](f32x16& c0, f32x16& c1, int a0, int a1) {
      f32x4 q0, q1, q2, q3, q4, q5, q6, q7;
      const unsigned char* p0 = park_src + a0 * 64;
      const unsigned char* p1 = park_src + a1 * 64;
      asm volatile("global_load_dwordx4 %0, %8, off\n\tglobal_load_dwordx4 %1, %8, off offset:16\n\t"
                   "global_load_dwordx4 %2, %8, off offset:32\n\tglobal_load_dwordx4 %3, %8, off offset:48\n\t"
                   "global_load_dwordx4 %4, %9, off\n\tglobal_load_dwordx4 %5, %9, off offset:16\n\t"
                   "global_load_dwordx4 %6, %9, off offset:32\n\tglobal_load_dwordx4 %7, %9, off offset:48\n\t"
                   "s_waitcnt vmcnt(0)"
                   : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3), "=&v"(q4), "=&v"(q5), "=&v"(q6), "=&v"(q7)
                   : "v"(p0), "v"(p1) : "memory");
      c0 = __builtin_shufflevector(__builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7), __builtin_shufflevector(q2, q3, 0, 1, 2, 3, 4, 5, 6, 7),
                                   0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
      c1 = __builtin_shufflevector(__builtin_shufflevector(q4, q5, 0, 1, 2, 3, 4, 5, 6, 7), __builtin_shufflevector(q6, q7, 0, 1, 2, 3, 4, 5, 6, 7),
                                   0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    };
    bool resume = PERSIST && is_tail;                              // first K tile of a tail piece: load accumulators per phase
    int w0s = 0;
    auto ktile = [&](int kt, auto tail_c, auto s1_c, auto s234_c) {
      constexpr int TAIL = decltype(tail_c)::value;
      constexpr bool S1 = decltype(s1_c)::value, S234 = decltype(s234_c)::value;
      const int cur = (kt & 1) * P8_TILE, oth = P8_TILE - cur;
      const unsigned char* buf = smem_raw + cur;
      const unsigned char* w0 = smem_raw + P8_W0RING + w0s * P8_REGION;
      const int w0_free = P8_W0RING + (w0s == 0 ? 2 : w0s - 1) * P8_REGION;   // slot (kt + 2) % 3: its K tile kt - 1 is done
      // phase 1
      read_a(buf + P8_A0);
      read_w(w0, w0h, w0l);
      if constexpr (S1) stage(kt + 1, oth + P8_A1, false, 1);
      if (PERSIST && resume) ldacc(acc[0][0], acc[1][0], 0 * TN + 0, 1 * TN + 0);
      P8_WAIT(10, 10, 2);
      P8_KBARRIER();
      quadrant(acc[0][0], acc[1][0], w0h, w0l);
      P8_KBARRIER();
      // phase 2
      read_w(buf + P8_W1, wh, wl);
      if constexpr (S234) stage(kt + 2, w0_free, true, 0);
      if (PERSIST && resume) ldacc(acc[0][1], acc[1][1], 0 * TN + 1, 1 * TN + 1);
      P8_WAIT(10, 8, 0);
      P8_KBARRIER();
      quadrant(acc[0][1], acc[1][1], wh, wl);
      P8_KBARRIER();
      // phase 3
      read_a(buf + P8_A1);
      if constexpr (S234) stage(kt + 2, cur + P8_A0, false, 0);
      if (PERSIST && resume) ldacc(acc[2][1], acc[3][1], 2 * TN + 1, 3 * TN + 1);
      P8_WAIT(10, 6, 0);
      P8_KBARRIER();
      quadrant(acc[2][1], acc[3][1], wh, wl);
      P8_KBARRIER();
      // phase 4: W0 is still in registers
      if constexpr (S234) stage(kt + 2, cur + P8_W1, true, 1);
      if (PERSIST && resume) ldacc(acc[2][0], acc[3][0], 2 * TN + 0, 3 * TN + 0);
      P8_WAIT(10, 4, 0);
      P8_KBARRIER();
      quadrant(acc[2][0], acc[3][0], w0h, w0l);
      P8_KBARRIER();
      w0s = w0s == 2 ? 0 : w0s + 1;
      if (PERSIST && resume) {                                     // every parked value is in registers: release the slot
        resume = false;
        __syncthreads();
        if (t == 0) __hip_atomic_store(ps.flag + (blockIdx.x - 8 * ngrp), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    };

#undef P8_WAIT
    if (nks >= 3) {
      ktile(0, I0{}, std::false_type{}, std::true_type{});
      for (int kt = 1; kt + 2 < nks; ++kt) ktile(kt, I0{}, std::true_type{}, std::true_type{});
      ktile(nks - 2, I1{}, std::true_type{}, std::false_type{});
      ktile(nks - 1, I2{}, std::false_type{}, std::false_type{});
    } else if (nks == 2) {                                         // everything came with the prologue
      ktile(0, I1{}, std::false_type{}, std::false_type{});
      ktile(1, I2{}, std::false_type{}, std::false_type{});
    } else {
      ktile(0, I2{}, std::false_type{}, std::false_type{});
    }
    if (group == 0 && !(ABL & 24)) WD_WG_BARRIER();                // pairs with the extra barrier of group 1
    WD_WG_BARRIER();                                               // every read of the operand tiles is over: LDS becomes epilogue patches

    if (PERSIST && is_head) {
      // park the raw accumulators for the next workgroup of the chain: plain coalesced stores, drained, then ONE
      // agent-scope release and the flag (MI355X_MICROARCH.md, inter-workgroup visibility)
      f32x4* lp = reinterpret_cast<f32x4*>(reinterpret_cast<unsigned char*>(ps.acc) + (size_t)blockIdx.x * P8_PARK_BYTES +
                                           (unsigned)t * 512u);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            lp[(i * TN + j) * 4 + g] = f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          __builtin_amdgcn_sched_barrier(0);
        }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(ps.flag + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      continue;
    }
    if (ABL & 4) {                                                  // keep the accumulators live, store (almost) nothing
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) sum += acc[i][j][r];
      if (sum == 12345.678f) p.c[t] = sum;
      continue;
    }
    if constexpr (!std::is_same_v<EPI, P8Store>) {                  // the product is scored, not stored
      EPI::run(p, ep, unscale, m0 + group * 128, n0 + wn * 64, lane, acc, reinterpret_cast<float*>(smem_raw) + wave * 32 * EPI_LDT);
      continue;
    }
    const EpiVec ev{vec_c, vec_res, vec_bias, unscale};
    const int mw = m0 + group * 128, nw = n0 + wn * 64;
    float* patch = reinterpret_cast<float*>(smem_raw) + wave * 32 * EPI_LDT;
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));          // epilogue address arithmetic starts HERE (hipcc otherwise computes it before the K loop and keeps ~50 registers alive across it)
    static_assert(P8_LDS >= 8 * 32 * EPI_LDT * 4, "operand LDS must hold one patch per wave");
    if constexpr ((VAR & P8VAR_DIRECT) != 0) {                      // hi/lo output without the LDS transpose (experiment, see split_gemm_impl.h)
      if (p.act == WD_ACT_GELU) EpiCsplitDirectWalk<0, TM, TN, WD_ACT_GELU>::run(p, ev, mw, nw, lane_e, acc);
      else EpiCsplitDirectWalk<0, TM, TN, WD_ACT_NONE>::run(p, ev, mw, nw, lane_e, acc);
    } else if (VAR & SVAR_CSPLIT) {
      // (ABL & 96: the timing-only forms of the GELU arm, epi_lds_tile_csplit)
      WD_ACT_DISPATCH(p.act, EpiCsplitWalk<0, TM, TN, ACT, (ACT == WD_ACT_GELU ? (ABL & 96) : 0)>::run(p, ev, mw, nw, lane_e, acc, patch));
    } else if (epi_res_prefetch_ok(p, ev, nw, 64) && mw < p.m) {
      // (split_store_tail's chain, spelled out: the scored epilogue below sits between its two last links)
      split_epilogue_res_prefetch<TM, TN, 3>(p, ev, mw, nw, lane_e, acc, patch);
    } else if (!PERSIST && (p.seg_rows > 0 || p.sigmoid || p.out_scale != 1.0f || p.out_bias != 0.0f)) {
      // round 6 (wd_similarity_split): per-level affine + sigmoid of the region x text logits, ragged n; no activation
      split_epilogue_lds<TM, TN, WD_ACT_NONE, true>(p, ev, mw, nw, lane_e, acc, patch);
    } else {
      WD_ACT_DISPATCH(p.act, split_epilogue_lds<TM, TN, ACT, false>(p, ev, mw, nw, lane_e, acc, patch));
    }
  }
}

constexpr long long P8_PARK_FLOATS = P8_PARK_BYTES / 4;

// one workgroup per CU, the same number on every XCD — a fact of the CURRENT device (a process may drive several)
int p8_workgroups() {
  static int n[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  int& slot = n[dev & 63];
  if (!slot) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    slot = prop.multiProcessorCount / 8 * 8;
  }
  return slot;
}

int p8_stagger() {
#ifdef WD_DEBUG_ABLATIONS                               // the CU-phase experiment of profiles/r05_p8_epilogue_ablation.txt: ablation builds only
  const char* e = getenv("WD_P8_STAGGER");
  return e ? atoi(e) : 0;
#else
  return 0;
#endif
}

// gang size of the persistent form for nbn column tiles: the largest of 8 / 4 / 2 / 1 that divides nbn (and the 32
// workgroups of an XCD)
int p8_gang(int nbn) { return nbn % 8 == 0 ? 8 : nbn % 4 == 0 ? 4 : nbn % 2 == 0 ? 2 : 1; }

// arows / wrows: rows the operand buffers hold where that is not p.m / p.n; ep: the arguments of a scoring epilogue (EPI is deduced)
template <int VAR, int ABL = 0, bool PERSIST = false, typename EPI = P8Store>
int launch_p8(const WdConvGemm& p, const void* wsp, float unscale, hipStream_t st, float* ws = nullptr, long long ws_floats = 0,
              int arows = 0, int wrows = 0, const EPI& ep = EPI{}) {
  const int nbm = (p.m + 255) / 256;
  const int nbn = EPI::PADS_COLUMN_TILES ? ((p.n + 255) / 256 + 7) / 8 * 8 : (p.n + 255) / 256;
  const long long nblk = (long long)nbm * nbn;
  if (nblk <= 0 || nblk > 0x7fffffffLL) return WD_ERR_BAD_ARG;
  const int k16 = (p.k + 15) / 16 * 16;
  // 32-bit DMA offsets from the operand bases
  if (!wd_dma32_fits(arows > 0 ? arows : p.m, p.lda, wrows > 0 ? wrows : p.n, k16)) return WD_ERR_UNSUPPORTED;
  const WdEpiVecFlags vf = wd_epi_vec_flags(p, false);
  // Column tiles of one row block are walked together, up to eight at a time: the activation panel of a row block is then
  // fetched once for all of them (a pwconv1 with n = 2048 re-read it per pair before: 42.79 -> 42.05 ms per step, same
  // box, three rounds; pairs = 2, the round-2 default until then, and 4 / 8 equal).  Up to 2048 weight rows live per group.
  int ngrp = 8;
  if (ngrp > nbn || nbn % ngrp) ngrp = nbn;
  P8Persist ps{nullptr, nullptr, nullptr, (int)nblk};
  long long grid = nblk;
  if (PERSIST) {
    const int wgs = p8_workgroups();
    if (wgs <= 0) return WD_ERR_LAUNCH;
    ngrp = p8_gang(nbn);
    const int per = wgs / 8;
    if (per % ngrp) return WD_ERR_UNSUPPORTED;
    ps.ntiles = (int)(nblk / ngrp);                                // gang tiles
    if (ps.ntiles / 8 < per / ngrp) return WD_ERR_UNSUPPORTED;     // ranges shorter than a tile would chain serially
    if (!ws || ws_floats < wd_p8_workspace_floats()) return WD_ERR_WORKSPACE;
    ps.flag = reinterpret_cast<unsigned*>(ws);                     // first 4 KB: flags (zero between launches); [512, 516): zeros
    ps.zero = ws + 512;
    ps.acc = ws + 1024;
    grid = wgs;
  }
  auto k = split_gemm_p8_kernel<VAR, EPI, ABL, PERSIST>;
  static WdAttrOnce attr;
  if (wd_set_max_lds(attr, reinterpret_cast<const void*>(k), P8_LDS) != WD_OK) return WD_ERR_LAUNCH;
  WD_LAUNCH_GEMM(k, dim3((unsigned)grid), dim3(512), P8_LDS, st, p, static_cast<const unsigned char*>(wsp), k16, unscale, nbn,
                 vf.c, vf.res, vf.bias, ngrp, nbm, ps, p8_stagger(), arows > 0 ? arows : p.m, wrows > 0 ? wrows : p.n, ep);
  return wd_launch_status();
}

// the launches that pad their operand buffers to whole groups of eight rows instead of requiring p.m % 8 == p.n % 8 == 0: the
// similarity launch (EPI = P8Store) and every scoring epilogue.  Retrieval had a launcher of its own that passed stagger = 0 and
// vec_c = 0: here it gets p8_stagger() (0 but in WD_DEBUG_ABLATIONS builds, where $WD_P8_STAGGER now delays it too) and a vec_c it never reads.
template <typename EPI>
int launch_p8_padded(const WdConvGemm& p, const void* wsp, float unscale, hipStream_t st, const EPI& ep) {
  return launch_p8<0>(p, wsp, unscale, st, nullptr, 0, (p.m + 7) & ~7, (p.n + 7) & ~7, ep);
}

}  // namespace

// does the persistent form apply to an m x n problem on the current device?  (every gang of every XCD gets at least one
// whole gang tile)
bool wd_p8_persist_ok(int m, int n) {
  const int wgs = p8_workgroups();
  if (wgs <= 0 || n % 256) return false;
  const int nbm = (m + 255) / 256, nbn = n / 256, g = p8_gang(nbn), per = wgs / 8;
  if (per % g) return false;
  return (long long)nbm * (nbn / g) / 8 >= per / g;
}

// workspace of the persistent form: 1024 flag words + one parked accumulator set per workgroup (fp32 elements)
long long wd_p8_workspace_floats() {
  const int wgs = p8_workgroups();
  return wgs <= 0 ? 0 : 1024 + (long long)wgs * P8_PARK_FLOATS;
}

// cfg 64: plain 1x1 layer, both operands pre-split, K % 32 == 0.  csplit: output written as fp16 hi/lo groups.
// persist (cfg 65): the work-unit form; ws = caller's workspace, zero-filled once before its first use.
int wd_launch_p8(const WdConvGemm& p, const void* w, float unscale, bool csplit, hipStream_t st, int abl, bool persist,
                 float* ws, long long ws_floats) {
#ifdef WD_DEBUG_ABLATIONS
  if (abl && !persist) {
    if (csplit) return abl == 4 ? launch_p8<SVAR_CSPLIT, 4>(p, w, unscale, st) : abl == 32 ? launch_p8<SVAR_CSPLIT, 32>(p, w, unscale, st)
                     : abl == 64 ? launch_p8<SVAR_CSPLIT, 64>(p, w, unscale, st) : WD_ERR_UNSUPPORTED;
    switch (abl) {
      case 1: return launch_p8<0, 1>(p, w, unscale, st);
      case 2: return launch_p8<0, 2>(p, w, unscale, st);
      case 3: return launch_p8<0, 3>(p, w, unscale, st);
      case 4: return launch_p8<0, 4>(p, w, unscale, st);
      case 7: return launch_p8<0, 7>(p, w, unscale, st);
      case 15: return launch_p8<0, 15>(p, w, unscale, st);
      case 16: return launch_p8<0, 16>(p, w, unscale, st);
      default: return WD_ERR_UNSUPPORTED;
    }
  }
#endif
  if (abl) return WD_ERR_UNSUPPORTED;
  if (p.k % 32 || p.k < 32 || p.lda % 8 || p.m % 8 || p.n % 8 || p.m < 8 || p.n < 8 || !wd_aligned16(p.a) || !wd_aligned16(w))
    return WD_ERR_UNSUPPORTED;                                     // DMA row groups of 8 are clamped as a whole
  if (csplit) {
    if (p.res || p.n % 8 || p.ldc % 8 || (p.bias && !wd_aligned16(p.bias)) || !wd_aligned16(p.c)) return WD_ERR_BAD_ARG;
#ifdef WD_DEBUG_ABLATIONS       // the direct hi/lo epilogue (no LDS transpose): measured 1.5 - 3 x slower, profiles/r05_csplit_direct.txt; ablation builds only
    const char* e = getenv("WEDETECT_CSPLIT_DIRECT");
    if (e && e[0] == '1' && (p.act == WD_ACT_GELU || p.act == WD_ACT_NONE))
      return persist ? launch_p8<SVAR_CSPLIT | P8VAR_DIRECT, 0, true>(p, w, unscale, st, ws, ws_floats)
                     : launch_p8<SVAR_CSPLIT | P8VAR_DIRECT>(p, w, unscale, st);
#endif
    return persist ? launch_p8<SVAR_CSPLIT, 0, true>(p, w, unscale, st, ws, ws_floats) : launch_p8<SVAR_CSPLIT>(p, w, unscale, st);
  }
  return persist ? launch_p8<0, 0, true>(p, w, unscale, st, ws, ws_floats) : launch_p8<0>(p, w, unscale, st);
}

// wd_retrieval_max_split on the 256 x 256 kernel (operand roles swapped, see P8RetrMax): bank rows [n_cls][dim] as the
// activation operand, region rows [n_rows][dim] as the weight operand; out [images][ldo] must be zero.  Needs dim % 32 == 0,
// 16-byte aligned scale / bias, both split buffers padded to whole groups of eight rows (wd_split_weights does that).
int wd_launch_p8_retrieval(const void* t_split, int n_cls, const void* e_split, int n_rows, int dim, float unscale,
                           const float* scale, const float* bias, const int* count, int rows_per_img, float* out, int ldo,
                           unsigned* range_flag, hipStream_t st) {
  if (dim % 32 || dim < 32 || n_cls <= 0 || n_rows <= 0 || rows_per_img <= 0) return WD_ERR_UNSUPPORTED;
  if (!wd_aligned16(t_split) || !wd_aligned16(e_split) || !wd_aligned16(scale) || !wd_aligned16(bias)) return WD_ERR_UNSUPPORTED;
  WdConvGemm p{};
  p.a = static_cast<const float*>(t_split);
  p.c = out;
  p.batch = 1; p.hin = 1; p.win = n_cls; p.cin = dim; p.lda = dim;
  p.kh = p.kw = p.stride = 1; p.hout = 1; p.wout = n_cls;
  p.m = n_cls; p.n = n_rows; p.k = dim; p.ldc = ldo;
  p.out_scale = 1.0f;
  p.range_flag = range_flag;
  return launch_p8_padded(p, e_split, unscale, st, P8RetrMax{scale, bias, count, out, rows_per_img, ldo});
}

// wd_similarity_split on the 256 x 256 kernel (round 6; yolo_world_head.py:90-108, generate_proposal.py:1129-1131): region rows
// [rows][dim] as fp16 hi/lo groups (buffer padded to a multiple of eight rows) x text rows [n_cls][dim] split by
// wd_split_weights_padded; out[row][cls] = (sigmoid)(<e, t> * unscale * seg_scale[level(row)] + seg_bias[level(row)]), the
// epilogue of the fp32 similarity GEMM.  Ragged n_cls (1203) and ldo are fine (scalar stores when ldo % 4).
int wd_launch_p8_similarity(const WdConvGemm& p, const void* t_split, float unscale, hipStream_t st) {
  if (!p8_similarity_ok(p, t_split)) return WD_ERR_UNSUPPORTED;
  return launch_p8_padded(p, t_split, unscale, st, P8Store{});
}

// The fused forms: the launch above with a scoring epilogue in place of the stores; p.c is unused.  The callers
// (best.hip, sparse.hip, topn.hip, groups.hip) have checked the sizes, wd_similarity_bank_fits among them (launch_p8 refuses a
// larger bank too: 32-bit DMA offsets from the operand base).
int wd_launch_p8_best(const WdConvGemm& p, const void* t_split, float unscale, unsigned long long* key, int cls_offset, hipStream_t st) {
  if (!p8_similarity_ok(p, t_split) || !p.sigmoid || !key || (reinterpret_cast<uintptr_t>(key) & 7u)) return WD_ERR_UNSUPPORTED;
  return launch_p8_padded(p, t_split, unscale, st, P8Best{key, cls_offset});
}

int wd_launch_p8_sparse(const WdConvGemm& p, const void* t_split, float unscale, unsigned long long* list, int list_cap, int* state,
                        int rows_per_img, int n_cls_total, int cls_offset, float thr, hipStream_t st) {
  if (!p8_similarity_ok(p, t_split) || !p.sigmoid || !list || !state) return WD_ERR_UNSUPPORTED;
  return launch_p8_padded(p, t_split, unscale, st, P8Sparse{list, state, rows_per_img, cls_offset, n_cls_total, list_cap, thr});
}

int wd_launch_p8_topn(const WdConvGemm& p, const void* t_split, float unscale, unsigned long long* key, int n_top, int cls_offset,
                      const float* row_scale, const float* row_bias, hipStream_t st) {
  if (!p8_similarity_ok(p, t_split) || !p.sigmoid || !key || (reinterpret_cast<uintptr_t>(key) & 7u) || n_top < 1 || n_top > 8)
    return WD_ERR_UNSUPPORTED;
  return launch_p8_padded(p, t_split, unscale, st, P8Topn{key, row_scale, row_bias, cls_offset, n_top});
}

// p.n % 32 == 0: a bin is in or out of the launch as a whole
int wd_launch_p8_group(const WdConvGemm& p, const void* t_split, float unscale, const int* group_of, const int* bin_first, int cls_offset,
                       float* out, int ldo, int n_groups, hipStream_t st) {
  if (!p8_similarity_ok(p, t_split) || !p.sigmoid || !group_of || !bin_first || !out || (p.n & 31) || (cls_offset & 31))
    return WD_ERR_UNSUPPORTED;
  return launch_p8_padded(p, t_split, unscale, st, P8Group{group_of, bin_first, out, cls_offset, ldo, n_groups});
}
