// track.hip — persistent object ids across frames, associated on the device (include/wedetect_hip_track.h).
//   wd_track_step     one workgroup per sequence walks its frames in order: predict, round 1 (IoU + appearance against all live
//                     slots), round 2 (IoU, low scores against the slots seen in the previous frame), update, births.  The slots'
//                     scalars live in LDS for the whole launch, the embeddings stay in the state; no global atomics, no scratch
//   wd_track_reset    selected sequences to "no tracks"
//   wd_track_export   the slots as plain arrays
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

template <int NC>
__global__ void __launch_bounds__(256) track_step_kernel(float* state, float* workspace, const float* __restrict__ boxes,
                                                         const float* __restrict__ scores, const int* __restrict__ labels,
                                                         const int* __restrict__ count, const float* __restrict__ embed, int n_frame,
                                                         int max_out, int max_tracks, int dim, StepParams P,
                                                         int* __restrict__ track_ids, int* __restrict__ track_hits) {
#pragma clang fp contract(off)
  __shared__ Shared sh;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Layout L{max_tracks, dim};
  float* st = state + (long long)s * L.words();
  int* sti = reinterpret_cast<int*>(st);
  float* temb = st + L.embed();                                    // [max_tracks][dim], read and written between barriers
  float* ws = workspace + (long long)s * max_tracks * max_out;
  int flip = 0;

  // the slots' scalars into LDS; lanes past max_tracks hold free slots
  {
    const bool in = tid < max_tracks;
    sh.id[tid] = in ? sti[L.id() + tid] : 0;
    sh.label[tid] = in ? sti[L.label() + tid] : 0;
    sh.score[tid] = in ? st[L.score() + tid] : 0.f;
    sh.hits[tid] = in ? sti[L.hits() + tid] : 0;
    sh.miss[tid] = in ? sti[L.miss() + tid] : 0;
    sh.has[tid] = in ? sti[L.has() + tid] : 0;
    f32x4 bx = {0.f, 0.f, 0.f, 0.f}, vl = {0.f, 0.f, 0.f, 0.f};
    if (in) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { bx[k] = st[L.box() + tid * 4 + k]; vl[k] = st[L.vel() + tid * 4 + k]; }
    }
    sh.box[tid] = bx;
    sh.vel[tid] = vl;
    if (tid == 0) { sh.next_id = sti[0]; sh.status = sti[1]; }
  }
  __syncthreads();

  for (int f = 0; f < n_frame; ++f) {
    const long long b = (long long)s * n_frame + f;
    int cnt = count[b];                                            // uniform
    if (cnt < 0) {
      if (tid == 0) sh.status |= WD_TRACK_STATUS_BAD_COUNT;
      cnt = 0;
    }
    cnt = cnt > max_out ? max_out : cnt;
    const f32x4* fbox = reinterpret_cast<const f32x4*>(boxes) + b * max_out;
    const float* fscore = scores + b * max_out;
    const int* flabel = labels + b * max_out;
    const float* fembed = embed + b * max_out * dim;

    // ---- predict; the live slots and the two row lists, each ascending (ballot + prefix)
    {
      const bool lv = sh.id[tid] > 0;
      if (lv) sh.pred[tid] = sh.box[tid] + sh.vel[tid];
      sh.match[tid] = -1;
      const u64 m = __ballot(lv);
      if (lane == 0) sh.wcnt[0][wave] = __popcll(m);
      __syncthreads();
      int off = 0;
      for (int w = 0; w < wave; ++w) off += sh.wcnt[0][w];
      if (lv) sh.live[off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)tid;
      if (tid == 0) { sh.n_live = sh.wcnt[0][0] + sh.wcnt[0][1] + sh.wcnt[0][2] + sh.wcnt[0][3]; sh.n_born = 0; }
      int n_hi = 0, n_lo = 0;
      for (int r0 = 0; r0 < cnt; r0 += 256) {                      // uniform trip count
        const int r = r0 + tid;
        const float sc = r < cnt ? fscore[r] : -1.f;
        const bool hi = r < cnt && sc >= P.high_thr, lo = r < cnt && sc >= P.low_thr && sc < P.high_thr;
        if (r < cnt) { sh.row_slot[r] = 0; sh.starts[r] = sc >= P.new_thr; }
        const u64 mh = __ballot(hi), ml = __ballot(lo);
        if (lane == 0) { sh.wcnt[1][wave] = __popcll(mh); sh.wcnt[2][wave] = __popcll(ml); }
        __syncthreads();
        int oh = n_hi, ol = n_lo;
        for (int w = 0; w < wave; ++w) { oh += sh.wcnt[1][w]; ol += sh.wcnt[2][w]; }
        if (hi) sh.hi_rows[oh + __popcll(mh & ((1ull << lane) - 1ull))] = (unsigned short)r;
        if (lo) sh.lo_rows[ol + __popcll(ml & ((1ull << lane) - 1ull))] = (unsigned short)r;
        n_hi += sh.wcnt[1][0] + sh.wcnt[1][1] + sh.wcnt[1][2] + sh.wcnt[1][3];
        n_lo += sh.wcnt[2][0] + sh.wcnt[2][1] + sh.wcnt[2][2] + sh.wcnt[2][3];
        __syncthreads();
      }
      if (tid == 0) { sh.n_hi = n_hi; sh.n_lo = n_lo; }
      __syncthreads();
    }
    const int n_live = sh.n_live, n_hi = sh.n_hi, n_lo = sh.n_lo;

    // ---- round 1: the high-score rows against all live slots
    {
      float* cand = n_live * n_hi <= TILE ? sh.tile : ws;
      // appearance: cand[j * n_live + i] = max(cos, 0) of row j with live slot i.  A wave holds TWO rows in registers and
      // streams the slots past them eight at a time: 24 loads of 16 bytes in flight per lane, sixteen independent sums
      for (int j0 = wave * 2; j0 < n_hi; j0 += 8) {
        const bool two = j0 + 1 < n_hi;                            // wave-uniform
        const int r0 = sh.hi_rows[j0], r1 = sh.hi_rows[two ? j0 + 1 : j0];
        f32x4 e0[NC], e1[NC];
        load_row<NC>(e0, fembed + (long long)r0 * dim, dim, lane);
        load_row<NC>(e1, fembed + (long long)r1 * dim, dim, lane);
        const float ss0 = tree_dot<NC>(e0, e0), ss1 = tree_dot<NC>(e1, e1);
        const bool ok0 = usable_norm(ss0), ok1 = usable_norm(ss1);
        const float inv0 = ok0 ? 1.0f / sqrtf(ss0) : 0.f, inv1 = ok1 ? 1.0f / sqrtf(ss1) : 0.f;
        if (lane == 0) { sh.inv_e[r0] = inv0; sh.inv_e[r1] = inv1; }
        for (int i0 = 0; i0 < n_live; i0 += 8) {
          int t[8];
          f32x4 tv[8][NC];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            t[u] = sh.live[i0 + u < n_live ? i0 + u : n_live - 1];
            load_row<NC>(tv[u], temb + (long long)t[u] * dim, dim, lane);   // read whether the slot has one or not: inside the state
          }
          float mine = 0.f;                                        // lane u keeps row 0's value of slot i0 + u, lane 8 + u row 1's
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const bool has = sh.has[t[u]] != 0;
            const float c0 = tree_dot<NC>(tv[u], e0) * inv0, c1 = tree_dot<NC>(tv[u], e1) * inv1;
            const float v0 = (ok0 && has) ? fmaxf(c0, 0.f) : 0.f, v1 = (ok1 && has) ? fmaxf(c1, 0.f) : 0.f;
            mine = lane == u ? v0 : (lane == 8 + u ? v1 : mine);
          }
          const int u = lane & 7;
          if (lane < 16 && i0 + u < n_live && (lane < 8 || two)) cand[(long long)(j0 + (lane >> 3)) * n_live + i0 + u] = mine;
        }
      }
      __syncthreads();
      // sim = w_iou * iou + w_app * max(cos, 0), one pair per lane; 0 where the pair is no candidate
#pragma unroll 2
      for (int idx = tid; idx < n_live * n_hi; idx += 256) {
        const int i = idx % n_live, j = idx / n_live;
        const int t = sh.live[i], r = sh.hi_rows[j];
        const float iou = track_iou(sh.pred[t], fbox[r]);
        const float sim = P.w_iou * iou + P.w_app * cand[idx];
        const bool ok = sim >= P.match_thr && (!P.match_labels || sh.label[t] == flabel[r]);
        cand[idx] = ok ? sim : 0.f;
      }
      __syncthreads();
      if (n_live > 0 && n_hi > 0) greedy(sh, cand, sh.hi_rows, n_hi, 1, tid, lane, wave, flip);
    }

    // ---- round 2: IoU only, the low-score rows against the unmatched slots seen in the previous frame
    if (n_live > 0 && n_lo > 0) {                                  // block-uniform
      float* cand = n_live * n_lo <= TILE ? sh.tile : ws;
      __syncthreads();                                             // the last reads of round 1's values are done
      for (int idx = tid; idx < n_live * n_lo; idx += 256) {
        const int i = idx % n_live, j = idx / n_live;
        const int t = sh.live[i], r = sh.lo_rows[j];
        float v = 0.f;
        if (sh.match[t] < 0 && sh.miss[t] == 0 && (!P.match_labels || sh.label[t] == flabel[r])) {
          const float iou = track_iou(sh.pred[t], fbox[r]);
          v = iou >= P.iou2_thr ? iou : 0.f;
        }
        cand[idx] = v;
      }
      __syncthreads();
      greedy(sh, cand, sh.lo_rows, n_lo, 2, tid, lane, wave, flip);
    }
    __syncthreads();

    // ---- update: the slots' scalars, one lane per slot
    if (sh.id[tid] > 0) {
      const int m = sh.match[tid];
      if (m >= 0) {
        const int r = m & 0xFFFF;
        const f32x4 det = fbox[r], bx = sh.box[tid], vl = sh.vel[tid];
        f32x4 nv;
#pragma unroll
        for (int k = 0; k < 4; ++k) nv[k] = P.ema_vel * vl[k] + P.w_vel * (det[k] - bx[k]);
        sh.vel[tid] = nv;
        sh.box[tid] = det;
        sh.label[tid] = flabel[r];
        sh.score[tid] = fscore[r];
        sh.hits[tid] += 1;
        sh.miss[tid] = 0;
      } else {
        sh.box[tid] = sh.pred[tid];
        sh.miss[tid] += 1;
        if (sh.miss[tid] > P.max_age) sh.id[tid] = 0;
      }
    }
    // the embeddings of the round-1 matches, one wave per slot (has / match are not touched by the lanes above)
    for (int i = wave; i < n_live; i += 4) {
      const int t = sh.live[i], m = sh.match[t];
      if (m < 0 || (m >> 16) != 1) continue;                       // wave-uniform
      const int r = m & 0xFFFF;
      const float inv = sh.inv_e[r];
      if (!(inv > 0.f)) continue;
      f32x4 e[NC], v[NC];
      load_row<NC>(e, fembed + (long long)r * dim, dim, lane);
      float* trow = temb + (long long)t * dim;
      if (sh.has[t]) {
        load_row<NC>(v, trow, dim, lane);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = P.ema_embed * v[c][k] + P.w_embed * (e[c][k] * inv);
        const float ss = tree_dot<NC>(v, v);
        if (usable_norm(ss)) {
          const float vi = 1.0f / sqrtf(ss);
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = v[c][k] * vi;
          store_row<NC>(v, trow, dim, lane);
        }
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = e[c][k] * inv;
        store_row<NC>(v, trow, dim, lane);
        if (lane == 0) sh.has[t] = 1;
      }
    }
    __syncthreads();

    // ---- births: in row order, each into the lowest free slot — a serial rule, one lane
    if (tid == 0) {
      int fs = 0, nb = 0;
      for (int j = 0; j < n_hi; ++j) {
        const int r = sh.hi_rows[j];
        if (sh.row_slot[r] != 0 || !sh.starts[r]) continue;
        while (fs < max_tracks && sh.id[fs] > 0) ++fs;
        if (fs >= max_tracks) { sh.status |= WD_TRACK_STATUS_FULL; break; }   // every later row would find none either
        sh.id[fs] = sh.next_id++;
        sh.label[fs] = flabel[r];
        sh.score[fs] = fscore[r];
        sh.box[fs] = fbox[r];
        sh.vel[fs] = f32x4{0.f, 0.f, 0.f, 0.f};
        sh.hits[fs] = 1;
        sh.miss[fs] = 0;
        sh.has[fs] = 0;
        sh.match[fs] = r | (3 << 16);
        sh.row_slot[r] = (unsigned short)(fs + 1);
        sh.live[nb++] = (unsigned short)fs;
      }
      sh.n_born = nb;
    }
    __syncthreads();
    const int n_born = sh.n_born;
    for (int k = wave; k < n_born; k += 4) {
      const int t = sh.live[k], r = sh.match[t] & 0xFFFF;
      const float inv = sh.inv_e[r];
      if (!(inv > 0.f)) continue;                                  // wave-uniform
      f32x4 e[NC];
      load_row<NC>(e, fembed + (long long)r * dim, dim, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) e[c][q] = e[c][q] * inv;
      store_row<NC>(e, temb + (long long)t * dim, dim, lane);
      if (lane == 0) sh.has[t] = 1;
    }
    for (int r = tid; r < max_out; r += 256) {
      const int sl = r < cnt ? sh.row_slot[r] : 0;
      track_ids[b * max_out + r] = sl ? sh.id[sl - 1] : 0;
      track_hits[b * max_out + r] = sl ? sh.hits[sl - 1] : 0;
    }
    __syncthreads();                                               // the frame's LDS and embedding writes, before the next frame
  }

  if (tid < max_tracks) {
    sti[L.id() + tid] = sh.id[tid];
    sti[L.label() + tid] = sh.label[tid];
    st[L.score() + tid] = sh.score[tid];
    sti[L.hits() + tid] = sh.hits[tid];
    sti[L.miss() + tid] = sh.miss[tid];
    sti[L.has() + tid] = sh.has[tid];
    const f32x4 bx = sh.box[tid], vl = sh.vel[tid];
#pragma unroll
    for (int k = 0; k < 4; ++k) { st[L.box() + tid * 4 + k] = bx[k]; st[L.vel() + tid * 4 + k] = vl[k]; }
  }
  if (tid == 0) { sti[0] = sh.next_id; sti[1] = sh.status; }
}

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

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool sizes_ok(int n_seq, int max_tracks, int dim) {
  return n_seq >= 1 && n_seq <= 65535 && max_tracks >= 1 && max_tracks <= MT && dim >= 4 && dim <= WD_TRACK_MAX_DIM && dim % 4 == 0;
}
bool finite(float v) { return v == v && v < __builtin_inff() && v > -__builtin_inff(); }
bool unit(float v) { return v >= 0.f && v <= 1.f; }

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
  if (!state || !workspace || !boxes || !scores || !labels || !count || !embed || !params || !track_ids || !track_hits)
    return WD_ERR_BAD_ARG;
  if (!sizes_ok(n_seq, max_tracks, dim) || n_frame < 1 || max_out < 1 || max_out > MR) return WD_ERR_BAD_ARG;
  if (n_frame > 0x7ffffff0LL / ((long long)n_seq * max_out * dim)) return WD_ERR_BAD_ARG;   // n_seq * max_out * dim <= 2^36: no overflow
  if (!wd_aligned16(state) || !wd_aligned16(workspace) || !wd_aligned16(boxes) || !wd_aligned16(embed) || !aligned4(scores) ||
      !aligned4(labels) || !aligned4(count) || !aligned4(track_ids) || !aligned4(track_hits))
    return WD_ERR_BAD_ARG;
  const WdTrackParams& p = *params;
  if (!finite(p.high_thr) || !finite(p.low_thr) || !finite(p.new_thr) || !finite(p.match_thr) || !finite(p.iou2_thr))
    return WD_ERR_BAD_ARG;
  if (p.low_thr > p.high_thr || p.new_thr < p.high_thr || !(p.match_thr > 0.f) || !(p.iou2_thr > 0.f)) return WD_ERR_BAD_ARG;
  if (!unit(p.w_iou) || !unit(p.ema_embed) || !unit(p.ema_vel) || p.max_age < 0) return WD_ERR_BAD_ARG;
  StepParams P;
  P.high_thr = p.high_thr; P.low_thr = p.low_thr; P.new_thr = p.new_thr; P.match_thr = p.match_thr; P.iou2_thr = p.iou2_thr;
  P.w_iou = p.w_iou; P.w_app = 1.0f - p.w_iou;                     // each rounded once, here
  P.ema_embed = p.ema_embed; P.w_embed = 1.0f - p.ema_embed;
  P.ema_vel = p.ema_vel; P.w_vel = 1.0f - p.ema_vel;
  P.max_age = p.max_age; P.match_labels = p.match_labels;
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
