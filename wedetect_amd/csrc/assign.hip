// assign.hip — optimal (Hungarian) assignment on the device (include/addons/wedetect_hip_assign.h).
//   wd_assign_max           one workgroup per problem: shortest augmenting paths with potentials on integer weights; the columns'
//                           distances, potentials and visited flags live in registers (a lane owns columns tid, tid + 256, ... and
//                           dummy column tid), the rows' potentials, the matching and the path in about 6 KB of LDS;
//                           no global atomics, no scratch, every loop bounded by the sizes alone
//   wd_track_step_optimal   the frame walk of track.hip (track_walk.h, one text for both) with that solver as the association
#include "common.h"
#include "addons/wedetect_hip_assign.h"
#include "track_frame.h"

namespace {

constexpr int NA = WD_ASSIGN_MAX_A;          // rows of the problem (the slot side), augmented one at a time
constexpr int NB = WD_ASSIGN_MAX_B;          // real columns (the row side); dummy column NB + i is private to row i, cost 0
constexpr int KB = NB / 256;                 // real columns per lane
constexpr int KC = KB + 1;                   // ... and the lane's dummy column
constexpr int INF = 0x7fffffff;
constexpr int BIAS = 1 << 23;                // makes a tentative distance (within +-2^23, see the header) an unsigned key
constexpr u64 NO_KEY = ~0ull;

// what the solver keeps in LDS
struct Solver {
  int u[NA];                                 // potential of row i, in [-(2^21 + 1), 0]
  short col_of[NA];                          // the column of row i: j < NB, NB + i (its dummy: unmatched), -1 = not assigned yet
  short owner[NB];                           // the row of real column j, -1 = free
  short prev[NB + NA];                       // the row a column was reached from in the current search
};

// q(x) of the header for a finite x > 0: the product by 2^20 is exact (or overflows to +inf, which the minimum takes care of)
__device__ __forceinline__ int quant(float x) { return (int)fminf(floorf(x * 1048576.0f), 2097152.0f); }

// w of the header, 0 = no candidate; ``bad`` is set by a negative or non-finite value
__device__ __forceinline__ int weight(float x, int q_thr, bool& bad) {
  if (x == 0.f) return 0;
  if (!(x > 0.f && x < __builtin_inff())) { bad = true; return 0; }
  const int w = quant(x) - q_thr + 1;
  return w > 0 ? w : 0;
}

__device__ __forceinline__ u64 wave_min_key(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, o, 64), hi = __shfl_xor((unsigned)(k >> 32), o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    k = other < k ? other : k;
  }
  return k;
}

// 256-lane minimum, one barrier inside; the caller alternates the two sets of ``part`` as for block_max_key (track_frame.h)
__device__ __forceinline__ u64 block_min_key(u64 k, u64* part, int lane, int wave) {
  k = wave_min_key(k);
  if (lane == 0) part[wave] = k;
  __syncthreads();
  const u64 a = part[0] < part[1] ? part[0] : part[1], b = part[2] < part[3] ? part[2] : part[3];
  return a < b ? a : b;
}

// The maximum-weight matching of val[j * n_a + i] (i < n_a <= NA, j < n_b <= NB), called by all 256 lanes with block-uniform
// arguments.  On return (after a barrier) S.col_of[i] holds row i's column (>= NB: unmatched) and S.owner[j] column j's row or -1.
// Returns whether a search hit its bound without a free column (block-uniform; it cannot happen); ``bad`` is per lane.
//
// Minimum-cost assignment on the costs -w with one dummy column of cost 0 per row, rows inserted in order.  A search is Dijkstra
// from row i0 on the reduced costs: ``dist`` of a column is its tentative distance, D the distance of the column taken last; the
// potentials move once, at the end of the search (u[i] += D - dist[col of i], v[j] -= D - dist[j] for the visited columns,
// u[i0] += D).  Only row i has an edge to dummy NB + i, and a row is in the search tree only as i0 or as the owner of a REAL
// column, so a dummy column that is reached is always free and its potential is never touched: it is 0.  With u[i] + 0 <= 0 for
// every row this bounds all potentials to [-(2^21 + 1), 0].  i0's own dummy is reachable from the first step on, so a search
// always ends at a free column, after at most (matched real columns + 1) <= n_a + 1 steps.
__device__ __forceinline__ bool solve_max(Solver& S, u64 (*part)[4], const float* val, int n_a, int n_b, int q_thr, int tid, int lane,
                                          int wave, int& flip, bool& bad) {
  int v[KC];                                                       // the potentials of the lane's columns (v[KB] stays 0)
#pragma unroll
  for (int k = 0; k < KC; ++k) v[k] = 0;
  if (tid < n_a) { S.u[tid] = 0; S.col_of[tid] = -1; }
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (tid + 256 * k < n_b) S.owner[tid + 256 * k] = -1;
  __syncthreads();
  bool bound = false;

  for (int i0 = 0; i0 < n_a; ++i0) {                               // uniform trip count
    int dist[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) dist[k] = INF;
    unsigned used = 0u;                                            // bit k: the lane's column k is in the tree
    int i = i0, D = 0, sink = -1;
    for (int step = 0; step <= n_a; ++step) {                      // at most n_a + 1 steps, whatever the values are
      const int ui = S.u[i];
      u64 best = NO_KEY;
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const int j = tid + 256 * k;
        if (j < n_b && !((used >> k) & 1u)) {
          const int w = weight(val[(long long)j * n_a + i], q_thr, bad);
          if (w > 0) {
            const int cur = D - w - ui - v[k];
            if (cur < dist[k]) { dist[k] = cur; S.prev[j] = (short)i; }
          }
          if (dist[k] != INF) {
            const u64 key = ((u64)(unsigned)(dist[k] + BIAS) << 32) | (unsigned)j;
            best = key < best ? key : best;
          }
        }
      }
      if (tid < n_a && !((used >> KB) & 1u)) {                     // the dummy column of row tid: an edge from that row only
        if (tid == i) {
          const int cur = D - ui;
          if (cur < dist[KB]) { dist[KB] = cur; S.prev[NB + tid] = (short)i; }
        }
        if (dist[KB] != INF) {
          const u64 key = ((u64)(unsigned)(dist[KB] + BIAS) << 32) | (unsigned)(NB + tid);
          best = key < best ? key : best;
        }
      }
      const u64 g = block_min_key(best, part[flip], lane, wave);   // the nearest column outside the tree, lowest among equals
      flip ^= 1;
      if (g == NO_KEY) break;                                      // block-uniform, like everything derived from g
      D = (int)(unsigned)(g >> 32) - BIAS;
      const int c = (int)(unsigned)(g & 0xFFFFFFFFull);
      if (c < NB) {
        if ((c & 255) == tid) used |= 1u << (c >> 8);
      } else if (c - NB == tid) {
        used |= 1u << KB;
      }
      const int o = c < NB ? (int)S.owner[c] : -1;
      if (o < 0) { sink = c; break; }
      i = o;
    }
    if (sink < 0) {
      bound = true;                                                // row i0 stays unmatched
    } else {
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        if ((used >> k) & 1u) {
          const int d = D - dist[k], o = S.owner[tid + 256 * k];
          v[k] -= d;
          if (o >= 0) S.u[o] += d;                                 // a row owns one column: no two lanes write one u
        }
      }
      if (tid == 0) S.u[i0] += D;
      __syncthreads();                                             // prev and u are written, the owners are read
      if (tid == 0) {                                              // flip the path: a serial walk of at most n_a + 1 columns
        int c = sink;
        for (int t = 0; t <= n_a; ++t) {
          const int r = S.prev[c];
          if (c < NB) S.owner[c] = (short)r;
          const int next = S.col_of[r];
          S.col_of[r] = (short)c;
          if (r == i0) break;
          c = next;
        }
      }
    }
    __syncthreads();
  }
  if (bound && tid < n_a && S.col_of[tid] < 0) S.col_of[tid] = (short)(NB + tid);
  __syncthreads();
  return bound;
}

struct AssignShared {
  Solver sol;
  u64 part[2][4];
  long long sum[4];
};

__global__ void __launch_bounds__(256) assign_max_kernel(const float* __restrict__ val, int n_a, int n_b, long long ld_prob, float thr,
                                                         int* __restrict__ match_a, int* __restrict__ match_b,
                                                         long long* __restrict__ total, int* __restrict__ status) {
  __shared__ AssignShared sh;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* pv = val + (long long)p * ld_prob;
  const int q_thr = quant(thr);
  int flip = 0;
  bool bad = false;
  const bool bound = solve_max(sh.sol, sh.part, pv, n_a, n_b, q_thr, tid, lane, wave, flip, bad);
  long long w = 0;
  if (tid < n_a) {
    const int c = sh.sol.col_of[tid];
    const bool real = c >= 0 && c < NB;
    match_a[(long long)p * n_a + tid] = real ? c : -1;
    bool again = false;
    if (real) w = weight(pv[(long long)c * n_a + tid], q_thr, again);
  }
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int j = tid + 256 * k;
    if (j < n_b) match_b[(long long)p * n_b + j] = sh.sol.owner[j];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
  if (lane == 0) sh.sum[wave] = w;
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0) {
    total[p] = (sh.sum[0] + sh.sum[1]) + (sh.sum[2] + sh.sum[3]);
    status[p] = (bound ? WD_ASSIGN_STATUS_BOUND : 0) | (any_bad ? WD_ASSIGN_STATUS_BAD_VALUE : 0);
  }
}

// the LDS object of the optimal step: the walk's, then the solver's (62 KB in all)
struct SharedOpt : Shared {
  Solver sol;
};

// the association of wd_track_step_optimal (see WD_TRACK_ASSOCIATE in track_walk.h): the live slots are the rows of the problem,
// the round's row list its columns.  A value that passed the round's threshold is finite unless it is +inf, which is no candidate.
__device__ __forceinline__ void associate_optimal(SharedOpt& sh, const float* cand, const unsigned short* rows, int n_rows, int round,
                                                  float thr, int tid, int lane, int wave, int& flip) {
  const int n_live = sh.n_live;
  bool bad = false;
  const bool bound = solve_max(sh.sol, sh.part, cand, n_live, n_rows, quant(thr), tid, lane, wave, flip, bad);
  if (tid < n_live) {
    const int c = sh.sol.col_of[tid];
    if (c >= 0 && c < NB) {
      const int t = sh.live[tid], r = rows[c];
      sh.match[t] = r | (round << 16);
      sh.row_slot[r] = (unsigned short)(t + 1);
    }
  }
  if (bound && tid == 0) sh.status |= WD_TRACK_STATUS_ASSIGN_BOUND;
}

#define WD_TRACK_SHARED SharedOpt
#define WD_TRACK_ASSOCIATE(cand, rows, n_rows, round, thr) associate_optimal(sh, cand, rows, n_rows, round, thr, tid, lane, wave, flip)

template <int NC>
__global__ void __launch_bounds__(256) track_step_optimal_kernel(float* state, float* workspace, const float* __restrict__ boxes,
                                                                 const float* __restrict__ scores, const int* __restrict__ labels,
                                                                 const int* __restrict__ count, const float* __restrict__ embed,
                                                                 int n_frame, int max_out, int max_tracks, int dim, StepParams P,
                                                                 int* __restrict__ track_ids, int* __restrict__ track_hits) {
#include "track_walk.h"
}

#undef WD_TRACK_ASSOCIATE
#undef WD_TRACK_SHARED

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
bool assign_sizes_ok(int n_prob, int n_a, int n_b) {
  return n_prob >= 1 && n_prob <= 65535 && n_a >= 1 && n_a <= NA && n_b >= 1 && n_b <= NB;
}

}  // namespace

extern "C" int wd_assign_abi_version(void) { return 1; }

extern "C" int64_t wd_assign_workspace_bytes(int32_t n_prob, int32_t n_a, int32_t n_b) {
  if (!assign_sizes_ok(n_prob, n_a, n_b)) return 0;
  return (int64_t)n_prob * 16;
}

extern "C" int wd_assign_max(const float* val, int32_t n_prob, int32_t n_a, int32_t n_b, int64_t ld_prob, float thr, int32_t* match_a,
                             int32_t* match_b, int64_t* total, int32_t* status, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  if (!val || !match_a || !match_b || !total || !status || !workspace) return WD_ERR_BAD_ARG;
  if (!assign_sizes_ok(n_prob, n_a, n_b) || ld_prob < (int64_t)n_a * n_b) return WD_ERR_BAD_ARG;
  if (n_prob > 1 && ld_prob > ((1LL << 40) - (int64_t)n_a * n_b) / (n_prob - 1)) return WD_ERR_BAD_ARG;   // no overflow either
  if (!finite(thr) || !(thr > 0.f)) return WD_ERR_BAD_ARG;
  if (!aligned4(val) || !aligned4(match_a) || !aligned4(match_b) || !aligned4(status) || !aligned8(total) || !wd_aligned16(workspace))
    return WD_ERR_BAD_ARG;
  if (workspace_bytes < wd_assign_workspace_bytes(n_prob, n_a, n_b)) return WD_ERR_WORKSPACE;
  hipLaunchKernelGGL(assign_max_kernel, dim3((unsigned)n_prob), dim3(256), 0, static_cast<hipStream_t>(stream), val, n_a, n_b,
                     (long long)ld_prob, thr, match_a, match_b, reinterpret_cast<long long*>(total), status);
  return wd_launch_status();
}

extern "C" int64_t wd_track_optimal_workspace_bytes(int32_t n_seq, int32_t max_tracks, int32_t max_out) {
  return wd_track_workspace_bytes(n_seq, max_tracks, max_out);
}

extern "C" int wd_track_step_optimal(void* state, void* workspace, const float* boxes, const float* scores, const int32_t* labels,
                                     const int32_t* count, const float* embed, int32_t n_seq, int32_t n_frame, int32_t max_out,
                                     int32_t max_tracks, int32_t dim, const WdTrackParams* params, int32_t* track_ids,
                                     int32_t* track_hits, int64_t workspace_bytes, void* stream) {
  if (!track_step_args_ok(state, workspace, boxes, scores, labels, count, embed, n_seq, n_frame, max_out, max_tracks, dim, params,
                          track_ids, track_hits))
    return WD_ERR_BAD_ARG;
  if (workspace_bytes < wd_track_optimal_workspace_bytes(n_seq, max_tracks, max_out)) return WD_ERR_WORKSPACE;
  const StepParams P = track_step_params(*params);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define WD_TRACK_CASE(NC_) \
  hipLaunchKernelGGL(track_step_optimal_kernel<NC_>, dim3((unsigned)n_seq), dim3(256), 0, st, static_cast<float*>(state), \
                     static_cast<float*>(workspace), boxes, scores, labels, count, embed, n_frame, max_out, max_tracks, dim, P, \
                     track_ids, track_hits)
  if (dim <= 256) WD_TRACK_CASE(1);
  else if (dim <= 512) WD_TRACK_CASE(2);
  else if (dim <= 768) WD_TRACK_CASE(3);
  else WD_TRACK_CASE(4);
#undef WD_TRACK_CASE
  return wd_launch_status();
}
