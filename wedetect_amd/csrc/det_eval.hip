// det_eval.hip — COCO / LVIS box-mAP evaluation on the device (wedetect_amd/det_eval.py; the rules are restated in
// that module's docstring and, loop for loop, in tests/det_eval_ref.py).
//
// Three stages, all bit-identical to the float64 arithmetic of pycocotools' COCOeval / lvis-api's LVISEval:
//   match      one wave per (image, category) pair with a det or a gt: stable rank of the dets by score (kept
//              below max_det), the D x G float64 IoU matrix (maskApi.c bbIou), then the sequential greedy loop of
//              evaluateImg with one lane per (IoU threshold, area range) — 40 lanes, each with its own "gt already
//              matched" bitset.  Per (lane, kept det): bit 0 matched (dtm != 0), bit 1 ignored (final dtIg).
//   sort       every kept det keyed (category, score descending, slot): slots are laid out pair by pair with the
//              pairs ordered (category, image position) and the dets of a pair by rank, so the slot is the
//              (image position, rank) tie-break of accumulate's mergesort on the concatenation.  Bitonic network:
//              4096-key chunks in LDS plus global stages for the wider strides (bitonic.h, shared with top-k).
//   accumulate one workgroup per (category, area range, max_det, threshold): block-wide scans of the TP / FP counts
//              with a carry across chunks.  pr = tp / (fp + tp + 2^-52) is only needed at TP positions (the precision
//              envelope at the first index whose recall reaches r is the maximum of pr over the TPs from there on),
//              so every TP folds its pr into the bucket of the largest recall threshold it reaches, and a suffix
//              maximum over the 101 buckets gives precision[t, :, k, a, m].
// FP contraction is off in every kernel that computes an IoU, a recall or a precision: the reference has no FMA.
#include <float.h>
#include <limits.h>

#include "bitonic.h"
#include "common.h"

namespace {

constexpr int DE_T = 10;                 // IoU thresholds
constexpr int DE_A = 4;                  // area ranges
constexpr int DE_L = DE_T * DE_A;        // greedy lanes of the match kernel, lane = a * DE_T + t
constexpr int DE_R = 101;                // recall thresholds
constexpr int MATCH_LDS = 8192;          // per-pair workspace in LDS; larger pairs get a global scratch slice
constexpr int SORT_CHUNK = 4096;         // keys per LDS-resident bitonic chunk

// gt bits as the host packs them
constexpr unsigned GT_IGNORE = 1u, GT_CROWD = 2u, GT_ID_NONZERO = 4u;
// per-pair gt bits in the workspace: bit a = area-ignored (_ignore) in range a, then crowd, id != 0
constexpr unsigned W_CROWD = 16u, W_ID_NONZERO = 32u;

__host__ __device__ inline long long match_workspace_bytes(long long dk, long long g) {
  const long long words = (g + 31) / 32;
  const long long b = 8 * dk * g + 4 * dk + 4 * DE_L * words + g;
  return (b + 15) & ~15ll;
}

// order-preserving float -> uint map; -0.0 is taken as +0.0 first, because the ranking here and numpy's mergesort
// compare the two as equal (ties keep their slot order)
__device__ __forceinline__ unsigned ordered_bits(float v) {
  const unsigned b = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one sort element (struct WdDetSortKey of the header): (category << 32 | ~ordered(score), slot); unique
struct SortKV {
  unsigned long long key;
  unsigned val, pad;
};
static_assert(sizeof(SortKV) == sizeof(WdDetSortKey), "SortKV mirrors WdDetSortKey");
__device__ __forceinline__ bool wd_bitonic_greater(const SortKV& a, const SortKV& b) {
  return a.key > b.key || (a.key == b.key && a.val > b.val);
}

__global__ void __launch_bounds__(64) det_match_kernel(
    const int* __restrict__ pair_det_off, const int* __restrict__ pair_gt_off, const int* __restrict__ pair_slot_off,
    const int* __restrict__ pair_cat, const long long* __restrict__ pair_scratch, const float* __restrict__ det_box,
    const float* __restrict__ det_score, const unsigned char* __restrict__ det_flag, const double* __restrict__ gt_box,
    const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_flag, const double* __restrict__ thr,
    const double* __restrict__ area_rng, int max_det, unsigned char* __restrict__ scratch, float* __restrict__ slot_score,
    int* __restrict__ slot_rank, SortKV* __restrict__ kv, unsigned char* __restrict__ flags, int n_slot, int* __restrict__ npig, int* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) unsigned char lds[MATCH_LDS];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int d0 = pair_det_off[p], D = pair_det_off[p + 1] - d0;
  const int g0 = pair_gt_off[p], G = pair_gt_off[p + 1] - g0;
  const int s0 = pair_slot_off[p], Dk = pair_slot_off[p + 1] - s0;
  if (Dk != (D < max_det ? D : max_det)) {
    if (lane == 0) atomicOr(err, 1);
    return;
  }
  const long long need = match_workspace_bytes(Dk, G);
  unsigned char* ws = lds;
  if (pair_scratch[p] >= 0) {
    ws = scratch + pair_scratch[p];
  } else if (need > MATCH_LDS) {
    if (lane == 0) atomicOr(err, 2);
    return;
  }
  const int W = (G + 31) / 32;
  double* iou = reinterpret_cast<double*>(ws);                                // [Dk][G]
  int* perm = reinterpret_cast<int*>(ws + 8ll * Dk * G);                      // [Dk] det index of each rank
  unsigned* gtm = reinterpret_cast<unsigned*>(perm + Dk);                     // [DE_L][W]
  unsigned char* gig = reinterpret_cast<unsigned char*>(gtm + DE_L * W);      // [G]

  // stable rank by score, descending (numpy argsort(-score, kind='mergesort')), kept below max_det
  const unsigned long long cat_hi = (unsigned long long)(unsigned)pair_cat[p] << 32;
  for (int i = lane; i < D; i += 64) {
    const float si = det_score[d0 + i];
    int r = 0;
    for (int j = 0; j < D; ++j) {
      const float sj = det_score[d0 + j];
      r += (sj > si) || (sj == si && j < i);
    }
    if (r < Dk) {
      perm[r] = i;
      slot_score[s0 + r] = si;
      slot_rank[s0 + r] = r;
      kv[s0 + r].key = cat_hi | (unsigned long long)(~ordered_bits(si));
      kv[s0 + r].val = (unsigned)(s0 + r);
    }
  }
  for (int g = lane; g < G; g += 64) {
    const double ar = gt_area[g0 + g];
    const unsigned f = gt_flag[g0 + g];
    unsigned b = 0;
    for (int a = 0; a < DE_A; ++a)
      if ((f & GT_IGNORE) || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) b |= 1u << a;
    if (f & GT_CROWD) b |= W_CROWD;
    if (f & GT_ID_NONZERO) b |= W_ID_NONZERO;
    gig[g] = (unsigned char)b;
  }
  for (int e = lane; e < DE_L * W; e += 64) gtm[e] = 0u;
  __syncthreads();

  // maskApi.c bbIou: det box [x1, y1, x2 - x1, y2 - y1] in float64, gt box xywh from the annotation file
  for (int e = lane; e < Dk * G; e += 64) {
    const int d = e / G, g = e - d * G;
    const float* b = det_box + (size_t)(d0 + perm[d]) * 4;
    const double dx = b[0], dy = b[1], dw = (double)b[2] - (double)b[0], dh = (double)b[3] - (double)b[1];
    const double* gb = gt_box + (size_t)(g0 + g) * 4;
    const double da = dw * dh, ga = gb[2] * gb[3];
    double o = 0.0;
    const double w = fmin(dw + dx, gb[2] + gb[0]) - fmax(dx, gb[0]);
    if (!(w <= 0.0)) {
      const double h = fmin(dh + dy, gb[3] + gb[1]) - fmax(dy, gb[1]);
      if (!(h <= 0.0)) {
        const double in = w * h;
        const double un = (gig[g] & W_CROWD) ? da : da + ga - in;
        o = in / un;
      }
    }
    iou[e] = o;
  }
  if (lane < DE_A) {
    int c = 0;
    for (int g = 0; g < G; ++g) c += !(gig[g] & (1u << lane));
    npig[(size_t)p * DE_A + lane] = c;
  }
  __syncthreads();

  // evaluateImg's greedy loop.  The gts are visited sorted by _ignore (stable): first the ones kept in this lane's
  // area range, then the ignored ones; the reference's "matched a kept gt and reached an ignored one: stop" is the
  // second pass running only when the first found nothing.
  if (lane < DE_L) {
    const int t = lane % DE_T, a = lane / DE_T;
    const unsigned ab = 1u << a;
    const double th = thr[t], lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    unsigned* mine = gtm + lane * W;
    unsigned char* out = flags + (size_t)lane * n_slot + s0;
    for (int d = 0; d < Dk; ++d) {
      const double* row = iou + (size_t)d * G;
      double best = th;
      int m = -1;
      for (int pass = 0; pass < 2 && m < 0; ++pass) {
        for (int g = 0; g < G; ++g) {
          const unsigned gb = gig[g];
          if (((gb & ab) != 0) != (pass == 1)) continue;
          if (((mine[g >> 5] >> (g & 31)) & 1u) && !(gb & W_CROWD)) continue;
          const double v = row[g];
          if (v < best) continue;
          best = v;
          m = g;
        }
      }
      unsigned o = 0;
      if (m >= 0) {
        mine[m >> 5] |= 1u << (m & 31);
        const unsigned gb = gig[m];
        if (gb & W_ID_NONZERO) o |= 1u;        // dtm = id of the gt: 0 reads as unmatched
        if (gb & ab) o |= 2u;                  // dtIg = gtIg[m]
      }
      if (!(o & 1u)) {                         // unmatched: ignored outside the area range / in a not-exhaustive category
        const int di = d0 + perm[d];
        const float* b = det_box + (size_t)di * 4;
        const double da = ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]);
        if (da < lo || da > hi || (det_flag[di] & 1u)) o |= 2u;
      }
      out[d] = (unsigned char)o;
    }
  }
}

// size == 0: full local sort of each chunk; size > chunk: the strides < chunk of the merge of width size
__global__ void __launch_bounds__(256) det_sort_chunk_kernel(SortKV* __restrict__ kv, int chunk, long long size) {
  __shared__ SortKV sk[SORT_CHUNK];
  const long long base = (long long)blockIdx.x * chunk;
  for (int i = threadIdx.x; i < chunk; i += 256) sk[i] = kv[base + i];
  __syncthreads();
  if (size == 0) {
    for (long long sz = 2; sz <= chunk; sz <<= 1)
      for (int j = (int)(sz >> 1); j > 0; j >>= 1) wd_lds_bitonic_pass<256>(sk, chunk, base, j, sz);
  } else {
    for (int j = chunk >> 1; j > 0; j >>= 1) wd_lds_bitonic_pass<256>(sk, chunk, base, j, size);
  }
  for (int i = threadIdx.x; i < chunk; i += 256) kv[base + i] = sk[i];
}

// one global-memory stage (stride j >= chunk) of the merge of width size
__global__ void __launch_bounds__(256) det_sort_global_kernel(SortKV* __restrict__ kv, long long n2, long long j,
                                                              long long size) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n2) wd_global_bitonic_step(kv, i, j, size);
}

// sorted position -> the rank, score and 40 flag planes of its slot
__global__ void __launch_bounds__(256) det_permute_kernel(const SortKV* __restrict__ kv, int n_slot,
                                                          const int* __restrict__ slot_rank,
                                                          const float* __restrict__ slot_score,
                                                          const unsigned char* __restrict__ flags,
                                                          int* __restrict__ sorted_rank, float* __restrict__ sorted_score,
                                                          unsigned char* __restrict__ sorted_flags) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_slot) return;
  const unsigned s = kv[j].val;
  sorted_rank[j] = slot_rank[s];
  sorted_score[j] = slot_score[s];
  for (int l = 0; l < DE_L; ++l) sorted_flags[(size_t)l * n_slot + j] = flags[(size_t)l * n_slot + s];
}

// inclusive block scan (256 threads) of a 64-bit sum; *total = the block's sum
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v, unsigned long long* s_w,
                                                             unsigned long long* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned lo = __shfl_up((unsigned)v, o, 64), hi = __shfl_up((unsigned)(v >> 32), o, 64);
    if (lane >= o) v += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 63) s_w[w] = v;
  __syncthreads();
  unsigned long long pre = 0, tot = 0;
  for (int i = 0; i < 4; ++i) {
    const unsigned long long x = s_w[i];
    if (i < w) pre += x;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return v + pre;
}

__global__ void __launch_bounds__(256) det_accumulate_kernel(
    const int* __restrict__ cat_slot_off, const int* __restrict__ cat_pair_off, const int* __restrict__ npig,
    const int* __restrict__ sorted_rank, const float* __restrict__ sorted_score,
    const unsigned char* __restrict__ sorted_flags, int n_slot, const double* __restrict__ rec_thr,
    const int* __restrict__ max_dets, int n_m, int n_k, double* __restrict__ precision, double* __restrict__ recall,
    double* __restrict__ scores) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_w[4];
  __shared__ int s_red[4];
  __shared__ long long s_cr[DE_R];
  __shared__ unsigned long long s_bucket[DE_R];
  __shared__ float s_ss[DE_R];
  __shared__ int s_first;
  int b = blockIdx.x;
  const int t = b % DE_T;
  b /= DE_T;
  const int m = b % n_m;
  b /= n_m;
  const int a = b % DE_A;
  const int k = b / DE_A;
  const int tid = threadIdx.x;

  int c = 0;
  for (int p = cat_pair_off[k] + tid; p < cat_pair_off[k + 1]; p += 256) c += npig[(size_t)p * DE_A + a];
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((tid & 63) == 0) s_red[tid >> 6] = c;
  __syncthreads();
  const int n_pig = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  if (n_pig == 0) return;                                  // the slice keeps -1
  const double np_d = (double)n_pig;
  if (tid < DE_R) {
    // the smallest TP count c with c / npig >= r: searchsorted(rc, r, 'left') lands on the c-th TP
    const double r = rec_thr[tid];
    long long cc = (long long)ceil(r * np_d);
    if (cc < 0) cc = 0;
    while (cc > 0 && (double)(cc - 1) / np_d >= r) --cc;
    while ((double)cc / np_d < r) ++cc;
    s_cr[tid] = cc;
    s_bucket[tid] = 0ull;
    s_ss[tid] = 0.0f;
  }
  if (tid == 0) s_first = INT_MAX;
  __syncthreads();

  const int j0 = cat_slot_off[k], j1 = cat_slot_off[k + 1];
  const int md = max_dets[m];
  const unsigned char* fl = sorted_flags + (size_t)(a * DE_T + t) * n_slot;
  unsigned long long carry = 0;                            // (tp << 32) | fp before this chunk
  for (int base = j0; base < j1; base += 256) {
    const int j = base + tid;
    unsigned long long v = 0;
    bool tp = false;
    if (j < j1 && sorted_rank[j] < md) {
      const unsigned f = fl[j];
      if (!(f & 2u)) {
        tp = (f & 1u) != 0;
        v = tp ? (1ull << 32) : 1ull;
      }
      if (s_first == INT_MAX) atomicMin(&s_first, j);
    }
    unsigned long long tot;
    const unsigned long long inc = block_scan_u64(v, s_w, &tot) + carry;
    if (tp) {
      const long long ntp = (long long)(inc >> 32);
      const double tpd = (double)ntp, fpd = (double)(inc & 0xffffffffull);
      const double pr = tpd / (fpd + tpd + DBL_EPSILON);  // np.spacing(1)
      int lo = 0, hi = DE_R - 1;                           // the last r with cr[r] <= ntp (cr[0] = 0)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_cr[mid] <= ntp) lo = mid; else hi = mid - 1;
      }
      atomicMax(&s_bucket[lo], (unsigned long long)__double_as_longlong(pr));   // pr >= 0: bits order like values
      for (int r = lo; r > 0 && s_cr[r] == ntp; --r) s_ss[r] = sorted_score[j];
    }
    carry += tot;
  }
  __syncthreads();
  const long long ntp_total = (long long)(carry >> 32);
  const bool any = s_first != INT_MAX;
  if (tid < DE_R) {
    double q = 0.0, ss = 0.0;
    if (any && s_cr[tid] <= ntp_total) {
      unsigned long long mx = 0ull;
      for (int r = tid; r < DE_R; ++r) mx = s_bucket[r] > mx ? s_bucket[r] : mx;
      q = __longlong_as_double((long long)mx);
      ss = (double)(tid == 0 ? sorted_score[s_first] : s_ss[tid]);
    }
    const size_t o = ((((size_t)t * DE_R + tid) * n_k + k) * DE_A + a) * n_m + m;
    precision[o] = q;
    if (scores) scores[o] = ss;
  }
  if (tid == 0) recall[(((size_t)t * n_k + k) * DE_A + a) * n_m + m] = any ? (double)ntp_total / np_d : 0.0;
}

}  // namespace

extern "C" int64_t wd_det_match_workspace_bytes(int32_t dets_kept, int32_t gts) {
  return match_workspace_bytes(dets_kept, gts);
}

extern "C" int32_t wd_det_match_lds_bytes(void) { return MATCH_LDS; }

extern "C" int wd_det_match(const int32_t* pair_det_off, const int32_t* pair_gt_off, const int32_t* pair_slot_off,
                            const int32_t* pair_cat, const int64_t* pair_scratch, int32_t n_pair, const float* det_box,
                            const float* det_score, const uint8_t* det_flag, const double* gt_box, const double* gt_area,
                            const uint8_t* gt_flag, const double* iou_thr, const double* area_rng, int32_t max_det,
                            uint8_t* scratch, float* slot_score, int32_t* slot_rank, WdDetSortKey* sort_keys,
                            uint8_t* flags, int32_t n_slot, int32_t* npig, int32_t* err, void* stream) {
  if (!pair_det_off || !pair_gt_off || !pair_slot_off || !pair_cat || !pair_scratch || !det_box || !det_score ||
      !det_flag || !gt_box || !gt_area || !gt_flag || !iou_thr || !area_rng || !slot_score || !slot_rank ||
      !sort_keys || !flags || !npig || !err)
    return WD_ERR_BAD_ARG;
  if (n_pair < 0 || n_slot < 0 || max_det <= 0) return WD_ERR_BAD_ARG;
  if (n_pair == 0) return WD_OK;
  hipLaunchKernelGGL(det_match_kernel, dim3((unsigned)n_pair), dim3(64), 0, static_cast<hipStream_t>(stream),
                     pair_det_off, pair_gt_off, pair_slot_off, pair_cat, reinterpret_cast<const long long*>(pair_scratch),
                     det_box, det_score, det_flag, gt_box, gt_area, gt_flag, iou_thr, area_rng, (int)max_det, scratch,
                     slot_score, slot_rank, reinterpret_cast<SortKV*>(sort_keys), flags, (int)n_slot, npig,
                     err);
  return wd_launch_status();
}

extern "C" int wd_det_sort(WdDetSortKey* sort_keys, int64_t n2, void* stream) {
  if (!sort_keys || n2 < 2 || (n2 & (n2 - 1))) return WD_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SortKV* k = reinterpret_cast<SortKV*>(sort_keys);
  const int chunk = n2 < SORT_CHUNK ? (int)n2 : SORT_CHUNK;
  const unsigned nblk = (unsigned)(n2 / chunk);
  hipLaunchKernelGGL(det_sort_chunk_kernel, dim3(nblk), dim3(256), 0, st, k, chunk, 0ll);
  for (long long size = 2ll * chunk; size <= n2; size <<= 1) {
    for (long long j = size >> 1; j >= chunk; j >>= 1)
      hipLaunchKernelGGL(det_sort_global_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, k,
                         (long long)n2, j, size);
    hipLaunchKernelGGL(det_sort_chunk_kernel, dim3(nblk), dim3(256), 0, st, k, chunk, size);
  }
  return wd_launch_status();
}

extern "C" int wd_det_accumulate(const WdDetSortKey* sorted_keys, int32_t n_slot, const int32_t* slot_rank,
                                 const float* slot_score, const uint8_t* flags, int32_t* sorted_rank,
                                 float* sorted_score, uint8_t* sorted_flags, const int32_t* cat_slot_off,
                                 const int32_t* cat_pair_off, const int32_t* npig, int32_t n_cat,
                                 const double* rec_thr, const int32_t* max_dets, int32_t n_maxdet, double* precision,
                                 double* recall, double* scores, void* stream) {
  if (!cat_slot_off || !cat_pair_off || !npig || !rec_thr || !max_dets || !precision || !recall) return WD_ERR_BAD_ARG;
  if (n_slot < 0 || n_cat < 0 || n_maxdet <= 0) return WD_ERR_BAD_ARG;
  if (n_slot > 0 && (!sorted_keys || !slot_rank || !slot_score || !flags || !sorted_rank || !sorted_score || !sorted_flags))
    return WD_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_slot > 0)
    hipLaunchKernelGGL(det_permute_kernel, dim3((unsigned)((n_slot + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const SortKV*>(sorted_keys),
                       (int)n_slot, slot_rank, slot_score, flags, sorted_rank, sorted_score, sorted_flags);
  if (n_cat > 0)
    hipLaunchKernelGGL(det_accumulate_kernel, dim3((unsigned)(n_cat * DE_A * n_maxdet * DE_T)), dim3(256), 0, st,
                       cat_slot_off, cat_pair_off, npig, sorted_rank, sorted_score, sorted_flags, (int)n_slot, rec_thr,
                       max_dets, (int)n_maxdet, (int)n_cat, precision, recall, scores);
  return wd_launch_status();
}
