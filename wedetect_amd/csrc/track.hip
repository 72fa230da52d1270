// track.hip — persistent object ids across frames, associated on the device (include/wedetect_hip_track.h).
//   wd_track_step     one workgroup per sequence walks its frames in order: predict, round 1 (IoU + appearance against all live
//                     slots), round 2 (IoU, low scores against the slots seen in the previous frame), update, births.  The slots'
//                     scalars live in LDS for the whole launch, the embeddings stay in the state; no global atomics, no scratch
//   wd_track_reset    selected sequences to "no tracks"
//   wd_track_export   the slots as plain arrays
//
// The frame walk itself (predict, candidates, update, births) is track_walk.h on the pieces of track_frame.h, shared with
// assign.hip (wd_track_step_optimal); this source gives it the greedy association.
#include "common.h"
#include "wedetect_hip_track.h"
#include "track_frame.h"

namespace {

// greedy assignment on cand[j * n_live + i] (row list index j, live index i; 0 = no candidate): lane i owns live slot i and keeps
// the best key of its free rows; one 256-lane maximum per pick, and only the lanes whose best row was taken look again
__device__ __forceinline__ void greedy(Shared& sh, const float* cand, const unsigned short* rows, int n_rows, int round, int tid,
                                       int lane, int wave, int& flip) {
  const int n_live = sh.n_live;
  const int t = tid < n_live ? sh.live[tid] : 0;
  bool free_i = tid < n_live && sh.match[t] < 0;
  u64 best = 0ull;
  bool scan = free_i;
  for (;;) {
    if (scan) {
      best = 0ull;
#pragma unroll 4
      for (int j = 0; j < n_rows; ++j) {
        const int r = rows[j];
        const unsigned v = __float_as_uint(cand[(long long)j * n_live + tid]);
        if (v != 0u && sh.row_slot[r] == 0) {
          const u64 key = ((u64)v << 32) | (u64)((0xFFFFu - (unsigned)t) << 16) | (u64)(0xFFFFu - (unsigned)r);
          best = key > best ? key : best;
        }
      }
      scan = false;
    }
    const u64 g = block_max_key(best, sh.part[flip], lane, wave);
    flip ^= 1;
    if (g == 0ull) break;                                          // block-uniform
    const int slot = 0xFFFF - (int)((g >> 16) & 0xFFFFu), row = 0xFFFF - (int)(g & 0xFFFFu);
    if (free_i && t == slot) {
      sh.match[t] = row | (round << 16);
      sh.row_slot[row] = (unsigned short)(slot + 1);
      free_i = false;
      best = 0ull;
    } else if (free_i && best != 0ull && 0xFFFF - (int)(best & 0xFFFFu) == row) {
      scan = true;
    }
    __syncthreads();
  }
}

// the association of wd_track_step; the round's threshold is not needed: a candidate's bits order like its value
#define WD_TRACK_SHARED Shared
#define WD_TRACK_ASSOCIATE(cand, rows, n_rows, round, thr) greedy(sh, cand, rows, n_rows, round, tid, lane, wave, flip)

template <int NC>
__global__ void __launch_bounds__(256) track_step_kernel(float* state, float* workspace, const float* __restrict__ boxes,
                                                         const float* __restrict__ scores, const int* __restrict__ labels,
                                                         const int* __restrict__ count, const float* __restrict__ embed, int n_frame,
                                                         int max_out, int max_tracks, int dim, StepParams P,
                                                         int* __restrict__ track_ids, int* __restrict__ track_hits) {
#include "track_walk.h"
}

#undef WD_TRACK_ASSOCIATE
#undef WD_TRACK_SHARED

__global__ void __launch_bounds__(256) track_reset_kernel(float* state, int max_tracks, int dim, const int* __restrict__ seq_mask) {
  const int s = blockIdx.x;
  if (seq_mask && seq_mask[s] == 0) return;                        // block-uniform
  const Layout L{max_tracks, dim};
  int* sti = reinterpret_cast<int*>(state + (long long)s * L.words());
  for (int w = threadIdx.x; w < L.scalars(); w += 256) sti[w] = w == 0 ? 1 : 0;
}

__global__ void __launch_bounds__(256) track_export_kernel(const float* __restrict__ state, int max_tracks, int dim,
                                                           int* __restrict__ ids, int* __restrict__ labels, float* __restrict__ scores,
                                                           float* __restrict__ boxes, int* __restrict__ hits, int* __restrict__ misses,
                                                           int* __restrict__ seq_info, float* __restrict__ vel, float* __restrict__ embed) {
  __shared__ int wcnt[4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Layout L{max_tracks, dim};
  const float* st = state + (long long)s * L.words();
  const int* sti = reinterpret_cast<const int*>(st);
  const bool in = tid < max_tracks;
  const int id = in ? sti[L.id() + tid] : 0;
  const bool lv = id > 0;
  if (in) {
    const long long o = (long long)s * max_tracks + tid;
    ids[o] = lv ? id : 0;
    labels[o] = lv ? sti[L.label() + tid] : 0;
    scores[o] = lv ? st[L.score() + tid] : 0.f;
    hits[o] = lv ? sti[L.hits() + tid] : 0;
    misses[o] = lv ? sti[L.miss() + tid] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) boxes[o * 4 + k] = lv ? st[L.box() + tid * 4 + k] : 0.f;
    if (vel) {
#pragma unroll
      for (int k = 0; k < 4; ++k) vel[o * 4 + k] = lv ? st[L.vel() + tid * 4 + k] : 0.f;
    }
  }
  const u64 m = __ballot(lv);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    int* q = seq_info + (long long)s * 4;
    q[0] = sti[0];
    q[1] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    q[2] = sti[1];
    q[3] = 0;
  }
  if (!embed) return;
  for (int t = wave; t < max_tracks; t += 4) {                     // a wave per slot, 16 bytes per lane
    const bool has = sti[L.id() + t] > 0 && sti[L.has() + t] != 0;
    const float* src = st + L.embed() + (long long)t * dim;
    float* dst = embed + ((long long)s * max_tracks + t) * dim;
    for (int d = lane * 4; d < dim; d += 256)
      *reinterpret_cast<f32x4*>(dst + d) = has ? *reinterpret_cast<const f32x4*>(src + d) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

}  // namespace

extern "C" int wd_track_abi_version(void) { return 1; }

extern "C" int64_t wd_track_state_bytes(int32_t n_seq, int32_t max_tracks, int32_t dim) {
  if (!sizes_ok(n_seq, max_tracks, dim)) return 0;
  return (int64_t)n_seq * Layout{max_tracks, dim}.words() * 4;
}

extern "C" int64_t wd_track_workspace_bytes(int32_t n_seq, int32_t max_tracks, int32_t max_out) {
  if (!sizes_ok(n_seq, max_tracks, 4) || max_out < 1 || max_out > MR) return 0;
  return (((int64_t)n_seq * max_tracks * max_out * 4) + 15) & ~(int64_t)15;
}

extern "C" int wd_track_reset(void* state, int32_t n_seq, int32_t max_tracks, int32_t dim, const int32_t* seq_mask, void* stream) {
  if (!state || !sizes_ok(n_seq, max_tracks, dim) || !wd_aligned16(state) || !aligned4(seq_mask)) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(track_reset_kernel, dim3((unsigned)n_seq), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<float*>(state), max_tracks, dim, seq_mask);
  return wd_launch_status();
}

extern "C" int wd_track_step(void* state, void* workspace, const float* boxes, const float* scores, const int32_t* labels,
                             const int32_t* count, const float* embed, int32_t n_seq, int32_t n_frame, int32_t max_out,
                             int32_t max_tracks, int32_t dim, const WdTrackParams* params, int32_t* track_ids, int32_t* track_hits,
                             void* stream) {
  if (!track_step_args_ok(state, workspace, boxes, scores, labels, count, embed, n_seq, n_frame, max_out, max_tracks, dim, params,
                          track_ids, track_hits))
    return WD_ERR_BAD_ARG;
  const StepParams P = track_step_params(*params);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define WD_TRACK_CASE(NC_) \
  hipLaunchKernelGGL(track_step_kernel<NC_>, dim3((unsigned)n_seq), dim3(256), 0, st, static_cast<float*>(state), \
                     static_cast<float*>(workspace), boxes, scores, labels, count, embed, n_frame, max_out, max_tracks, dim, P, \
                     track_ids, track_hits)
  if (dim <= 256) WD_TRACK_CASE(1);
  else if (dim <= 512) WD_TRACK_CASE(2);
  else if (dim <= 768) WD_TRACK_CASE(3);
  else WD_TRACK_CASE(4);
#undef WD_TRACK_CASE
  return wd_launch_status();
}

extern "C" int wd_track_export(const void* state, int32_t n_seq, int32_t max_tracks, int32_t dim, int32_t* ids, int32_t* labels,
                               float* scores, float* boxes, int32_t* hits, int32_t* misses, int32_t* seq_info, float* vel,
                               float* embed, void* stream) {
  if (!state || !ids || !labels || !scores || !boxes || !hits || !misses || !seq_info) return WD_ERR_BAD_ARG;
  if (!sizes_ok(n_seq, max_tracks, dim) || !wd_aligned16(state) || !wd_aligned16(embed)) return WD_ERR_BAD_ARG;
  if (!aligned4(ids) || !aligned4(labels) || !aligned4(scores) || !aligned4(boxes) || !aligned4(hits) || !aligned4(misses) ||
      !aligned4(seq_info) || !aligned4(vel))
    return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(track_export_kernel, dim3((unsigned)n_seq), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(state), max_tracks, dim, ids, labels, scores, boxes, hits, misses, seq_info, vel, embed);
  return wd_launch_status();
}
