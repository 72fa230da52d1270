// track_frame.h — what the frame walk of the tracker (include/wedetect_hip_track.h) is built from, shared by the two sources that
// launch it:
//   track.hip    wd_track_step           the greedy association
//   assign.hip   wd_track_step_optimal   the maximum-weight matching of include/addons/wedetect_hip_assign.h
// One workgroup per sequence walks its frames in order: predict, round 1 (IoU + appearance against all live slots), round 2 (IoU,
// low scores against the slots seen in the previous frame), update, births.  The slots' scalars live in LDS for the whole launch,
// the embeddings stay in the state; no global atomics, no scratch.  Here: the state layout, the reductions, the LDS object and
// the argument checks of the two entry points; the walk itself is track_walk.h, the text of both step kernels' bodies, which
// differ in the association of a round's candidate matrix and in nothing else.
#pragma once
#include "common.h"
#include "wedetect_hip_track.h"

namespace {

typedef unsigned long long u64;

constexpr int MT = WD_TRACK_MAX_TRACKS;      // slots per sequence, one lane each
constexpr int MR = WD_TRACK_MAX_OUT;         // rows per frame
constexpr int TILE = 6144;                   // candidate values kept in LDS; a larger matrix lives in the workspace

// the state of one sequence in 4-byte words (wd_track_state_bytes)
struct Layout {
  int mt, dim;
  __host__ __device__ int id() const { return 4; }
  __host__ __device__ int label() const { return 4 + mt; }
  __host__ __device__ int score() const { return 4 + 2 * mt; }
  __host__ __device__ int hits() const { return 4 + 3 * mt; }
  __host__ __device__ int miss() const { return 4 + 4 * mt; }
  __host__ __device__ int has() const { return 4 + 5 * mt; }
  __host__ __device__ int box() const { return 4 + 6 * mt; }
  __host__ __device__ int vel() const { return 4 + 10 * mt; }
  __host__ __device__ int scalars() const { return 4 + 14 * mt; }
  __host__ __device__ int embed() const { return (scalars() + 3) & ~3; }
  __host__ __device__ long long words() const { return (long long)embed() + (long long)mt * dim; }
};

// 64-lane maximum of a key: an xor butterfly on both halves of the word, every lane ends with the result (exemplar.hip)
__device__ __forceinline__ u64 wave_max_key(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, o, 64), hi = __shfl_xor((unsigned)(k >> 32), o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    k = other > k ? other : k;
  }
  return k;
}

// 256-lane maximum, one barrier inside.  ``part`` holds two sets of four keys which the caller alternates, so that a lane still
// reading one set never meets the next maximum's writes (greedy() leaves its loop straight after a maximum, without a barrier)
__device__ __forceinline__ u64 block_max_key(u64 k, u64* part, int lane, int wave) {
  k = wave_max_key(k);
  if (lane == 0) part[wave] = k;
  __syncthreads();
  const u64 a = part[0] > part[1] ? part[0] : part[1], b = part[2] > part[3] ? part[2] : part[3];
  return a > b ? a : b;
}

// inter / (area_p + area_d - inter), every operation individually rounded, in the order of iou_gt (postprocess.hip); a NaN is 0
__device__ __forceinline__ float track_iou(const f32x4 p, const f32x4 d) {
#pragma clang fp contract(off)
  const float area_p = (p[2] - p[0]) * (p[3] - p[1]);
  const float area_d = (d[2] - d[0]) * (d[3] - d[1]);
  const float xx1 = fmaxf(p[0], d[0]), yy1 = fmaxf(p[1], d[1]);
  const float xx2 = fminf(p[2], d[2]), yy2 = fminf(p[3], d[3]);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  const float iou = inter / (area_p + area_d - inter);
  return iou == iou ? iou : 0.f;
}

// the reduction tree of every sum over d: four accumulators per lane (one per d % 4), chunk after chunk, (a0 + a1) + (a2 + a3),
// then the 64-lane butterfly — it depends on nothing but dim.  Lanes past dim hold zeros.
template <int NC>
__device__ __forceinline__ float tree_dot(const f32x4 (&a)[NC], const f32x4 (&b)[NC]) {
#pragma clang fp contract(off)
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    a0 = a0 + a[c][0] * b[c][0];
    a1 = a1 + a[c][1] * b[c][1];
    a2 = a2 + a[c][2] * b[c][2];
    a3 = a3 + a[c][3] * b[c][3];
  }
  float s = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  return s;
}

template <int NC>
__device__ __forceinline__ void load_row(f32x4 (&v)[NC], const float* row, int dim, int lane) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = (c * 64 + lane) * 4;
    v[c] = d < dim ? *reinterpret_cast<const f32x4*>(row + d) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

template <int NC>
__device__ __forceinline__ void store_row(const f32x4 (&v)[NC], float* row, int dim, int lane) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = (c * 64 + lane) * 4;
    if (d < dim) *reinterpret_cast<f32x4*>(row + d) = v[c];
  }
}

__device__ __forceinline__ bool usable_norm(float ss) { return ss > 0.f && ss < __builtin_inff(); }   // a NaN fails both

struct StepParams {
  float high_thr, low_thr, new_thr, match_thr, iou2_thr, w_iou, w_app, ema_embed, w_embed, ema_vel, w_vel;
  int max_age, match_labels;
};

// everything a frame needs in LDS
struct Shared {
  int id[MT], label[MT], hits[MT], miss[MT], has[MT], match[MT];   // match: -1, or row | round << 16 (round 3: born in this frame)
  float score[MT];
  f32x4 box[MT], vel[MT], pred[MT];
  unsigned short live[MT];             // the live slots, ascending; after the update: the slots born in this frame
  unsigned short hi_rows[MR], lo_rows[MR], row_slot[MR];   // row lists, ascending; row_slot: slot + 1 of a row, 0 = none
  float inv_e[MR];                     // 1 / |e| of a high-score row, 0 = its embedding is not usable
  unsigned char starts[MR];            // the row's score is >= new_thr: it starts a track if nothing matches it
  float tile[TILE];
  u64 part[2][4];
  int wcnt[3][4];
  int n_live, n_hi, n_lo, n_born, next_id, status;
};

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool sizes_ok(int n_seq, int max_tracks, int dim) {
  return n_seq >= 1 && n_seq <= 65535 && max_tracks >= 1 && max_tracks <= MT && dim >= 4 && dim <= WD_TRACK_MAX_DIM && dim % 4 == 0;
}
inline bool finite(float v) { return v == v && v < __builtin_inff() && v > -__builtin_inff(); }
inline bool unit(float v) { return v >= 0.f && v <= 1.f; }

// every refusal of wd_track_step (wedetect_hip_track.h, "WD_ERR_BAD_ARG:"); wd_track_step_optimal makes the same ones
inline bool track_step_args_ok(const void* state, const void* workspace, const float* boxes, const float* scores, const int32_t* labels,
                               const int32_t* count, const float* embed, int32_t n_seq, int32_t n_frame, int32_t max_out,
                               int32_t max_tracks, int32_t dim, const WdTrackParams* params, const int32_t* track_ids,
                               const int32_t* track_hits) {
  if (!state || !workspace || !boxes || !scores || !labels || !count || !embed || !params || !track_ids || !track_hits) return false;
  if (!sizes_ok(n_seq, max_tracks, dim) || n_frame < 1 || max_out < 1 || max_out > MR) return false;
  if (n_frame > 0x7ffffff0LL / ((long long)n_seq * max_out * dim)) return false;   // n_seq * max_out * dim <= 2^36: no overflow
  if (!wd_aligned16(state) || !wd_aligned16(workspace) || !wd_aligned16(boxes) || !wd_aligned16(embed) || !aligned4(scores) ||
      !aligned4(labels) || !aligned4(count) || !aligned4(track_ids) || !aligned4(track_hits))
    return false;
  const WdTrackParams& p = *params;
  if (!finite(p.high_thr) || !finite(p.low_thr) || !finite(p.new_thr) || !finite(p.match_thr) || !finite(p.iou2_thr)) return false;
  if (p.low_thr > p.high_thr || p.new_thr < p.high_thr || !(p.match_thr > 0.f) || !(p.iou2_thr > 0.f)) return false;
  if (!unit(p.w_iou) || !unit(p.ema_embed) || !unit(p.ema_vel) || p.max_age < 0) return false;
  return true;
}

inline StepParams track_step_params(const WdTrackParams& p) {
  StepParams P;
  P.high_thr = p.high_thr; P.low_thr = p.low_thr; P.new_thr = p.new_thr; P.match_thr = p.match_thr; P.iou2_thr = p.iou2_thr;
  P.w_iou = p.w_iou; P.w_app = 1.0f - p.w_iou;                     // each rounded once, here
  P.ema_embed = p.ema_embed; P.w_embed = 1.0f - p.ema_embed;
  P.ema_vel = p.ema_vel; P.w_vel = 1.0f - p.ema_vel;
  P.max_age = p.max_age; P.match_labels = p.match_labels;
  return P;
}

}  // namespace
