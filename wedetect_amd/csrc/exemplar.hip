// exemplar.hip — class-bank rows from example boxes (include/wedetect_hip_exemplar.h).
//   wd_exemplar_assign   one workgroup per (example, image): the m anchors whose decoded boxes overlap the example best, selected in
//                        registers, across lanes and through LDS — no atomics, no workspace
//   wd_exemplar_pool     one workgroup per class: IoU-weighted mean of the L2-normalised embeddings of its slots, L2-normalised
#include "common.h"
#include "wedetect_hip_exemplar.h"

namespace {

typedef unsigned long long u64;

// 64-lane maximum of a key: an xor butterfly on both halves of the word, every lane ends with the result
__device__ __forceinline__ u64 wave_max_key(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, o, 64), hi = __shfl_xor((unsigned)(k >> 32), o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    k = other > k ? other : k;
  }
  return k;
}

// inter / (area_e + area_n - inter), every operation individually rounded, in the order of iou_gt (postprocess.hip)
__device__ __forceinline__ float exemplar_iou(const f32x4 e, float area_e, const f32x4 n) {
#pragma clang fp contract(off)
  const float area_n = (n[2] - n[0]) * (n[3] - n[1]);
  const float xx1 = fmaxf(e[0], n[0]), yy1 = fmaxf(e[1], n[1]);
  const float xx2 = fminf(e[2], n[2]), yy2 = fminf(e[3], n[3]);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  return inter / (area_e + area_n - inter);
}

template <int M>
__global__ void __launch_bounds__(256) exemplar_assign_kernel(const f32x4* __restrict__ boxes, int n_anchor,
                                                              const float* __restrict__ ex_boxes, const int* __restrict__ ex_count,
                                                              const float* __restrict__ meta, int max_ex, float min_iou,
                                                              int* __restrict__ sel_anchors, float* __restrict__ sel_iou,
                                                              int* __restrict__ sel_count) {
  __shared__ u64 merged[4 * M];
  const int e = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int cnt = ex_count[b];                                           // uniform
  cnt = cnt < 0 ? 0 : (cnt > max_ex ? max_ex : cnt);
  const long long slot0 = ((long long)b * max_ex + e) * M;
  if (e == 0 && tid == 0) sel_count[b] = cnt * M;
  if (e >= cnt) {                                                  // block-uniform: an empty example slot
    if (tid < M) { sel_anchors[slot0 + tid] = -1; sel_iou[slot0 + tid] = 0.f; }
    return;
  }
  f32x4 ex;
  float area_e;
  {
#pragma clang fp contract(off)
    const float* mt = meta + (long long)b * 8;                     // pad_x, pad_y, -, scale_x, scale_y
    const float* eb = ex_boxes + ((long long)b * max_ex + e) * 4;
    ex[0] = eb[0] * mt[3] + mt[0];
    ex[1] = eb[1] * mt[4] + mt[1];
    ex[2] = eb[2] * mt[3] + mt[0];
    ex[3] = eb[3] * mt[4] + mt[1];
    area_e = (ex[2] - ex[0]) * (ex[3] - ex[1]);
  }
  const f32x4* bp = boxes + (long long)b * n_anchor;

  // the lane's M best keys, descending, in registers: every index below is a constant after unrolling
  u64 best[M];
#pragma unroll
  for (int j = 0; j < M; ++j) best[j] = 0ull;
  for (int n0 = tid; n0 < n_anchor; n0 += 1024) {
    f32x4 bx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + u * 256;
      bx[u] = n < n_anchor ? bp[n] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + u * 256;
      const float iou = exemplar_iou(ex, area_e, bx[u]);
      if (n < n_anchor && iou > min_iou) {                         // a NaN fails the comparison
        u64 c = ((u64)__float_as_uint(iou) << 32) | (u64)(0xFFFFFFFFu - (unsigned)n);
        if (c > best[M - 1]) {
#pragma unroll
          for (int j = 0; j < M; ++j) {                            // compare-exchange down the list: the loser of the last slot falls out
            const bool gt = c > best[j];
            const u64 hi = gt ? c : best[j];
            c = gt ? best[j] : c;
            best[j] = hi;
          }
        }
      }
    }
  }

  // the wave's M largest keys: M rounds of a 64-lane maximum; keys are distinct (the anchor is part of them), so exactly one lane
  // owns a non-empty maximum and drops its head
  u64 top[M];
#pragma unroll
  for (int t = 0; t < M; ++t) {
    const u64 mx = wave_max_key(best[0]);
    top[t] = mx;
    if (mx != 0ull && best[0] == mx) {
#pragma unroll
      for (int j = 0; j + 1 < M; ++j) best[j] = best[j + 1];
      best[M - 1] = 0ull;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < M; ++t) merged[wave * M + t] = top[t];
  }
  __syncthreads();
  if (wave != 0) return;
  u64 mine = lane < 4 * M ? merged[lane] : 0ull;                   // <= 32 keys, one per lane
#pragma unroll
  for (int t = 0; t < M; ++t) {
    const u64 mx = wave_max_key(mine);
    if (mx != 0ull && mine == mx) mine = 0ull;
    if (lane == 0) {
      sel_anchors[slot0 + t] = mx ? (int)(0xFFFFFFFFu - (unsigned)mx) : -1;
      sel_iou[slot0 + t] = mx ? __uint_as_float((unsigned)(mx >> 32)) : 0.f;
    }
  }
}

// sum over the workgroup of one float per lane: butterfly inside the wave, then the four wave sums in a fixed order — the tree
// depends on nothing but the lane count.  ``part`` holds two sets of four words: the caller alternates them, so one barrier per
// reduction is enough.
__device__ __forceinline__ float block_sum(float v, float* part, int lane, int wave) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) part[wave] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void __launch_bounds__(256) exemplar_pool_kernel(const float* __restrict__ level_embed, int dim, int off1, int off2,
                                                            const int* __restrict__ sel_anchors, const float* __restrict__ sel_iou,
                                                            int n_slot, const int* __restrict__ cls_off, const int* __restrict__ cls_slot,
                                                            float* __restrict__ bank, int* __restrict__ support) {
#pragma clang fp contract(off)
  __shared__ float part[2][4];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool active = tid * 4 < dim;
  int lo = cls_off[c];
  const int hi = cls_off[c + 1];
  lo = lo < 0 ? 0 : lo;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int n = 0, flip = 0;
  for (int i = lo; i < hi; ++i) {                                  // block-uniform control flow throughout
    const int s = cls_slot[i];
    if (s < 0 || s >= n_slot) continue;
    const int a = sel_anchors[s];
    if (a < 0) continue;
    const float w = sel_iou[s];
    const int l = (a >= off1) + (a >= off2);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (active) r = *reinterpret_cast<const f32x4*>(level_embed + ((long long)l * n_slot + s) * dim + tid * 4);
    const float sq = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3];
    const float inv = 1.0f / sqrtf(block_sum(sq, part[flip], lane, wave));
    flip ^= 1;
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[d] = acc[d] + w * (r[d] * inv);
    ++n;
  }
  const float sq = ((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]) + acc[3] * acc[3];
  const float nrm = sqrtf(block_sum(sq, part[flip], lane, wave));
  const bool ok = n > 0 && nrm > 0.f && nrm < __builtin_inff();    // a NaN fails both comparisons
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (ok) {
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = acc[d] / nrm;
  }
  if (active) *reinterpret_cast<f32x4*>(bank + (long long)c * dim + tid * 4) = o;
  if (tid == 0) support[c] = n;
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

template <int M>
void launch_assign(dim3 grid, hipStream_t st, const float* boxes, int n_anchor, const float* ex_boxes, const int* ex_count,
                   const float* meta, int max_ex, float min_iou, int* sel_anchors, float* sel_iou, int* sel_count) {
  hipLaunchKernelGGL(exemplar_assign_kernel<M>, grid, dim3(256), 0, st, reinterpret_cast<const f32x4*>(boxes), n_anchor, ex_boxes,
                     ex_count, meta, max_ex, min_iou, sel_anchors, sel_iou, sel_count);
}

}  // namespace

extern "C" int wd_exemplar_abi_version(void) { return 1; }

extern "C" int wd_exemplar_assign(const float* boxes, int32_t n_anchor, const float* ex_boxes, const int32_t* ex_count,
                                  const float* meta, int32_t max_ex, int32_t batch, int32_t m, float min_iou, int32_t* sel_anchors,
                                  float* sel_iou, int32_t* sel_count, void* stream) {
  if (!boxes || !ex_boxes || !ex_count || !meta || !sel_anchors || !sel_iou || !sel_count) return WD_ERR_BAD_ARG;
  if (n_anchor <= 0 || batch <= 0 || max_ex < 1 || max_ex > WD_EXEMPLAR_MAX_EX || m < 1 || m > WD_EXEMPLAR_MAX_M) return WD_ERR_BAD_ARG;
  if (!(min_iou >= 0.f) || !(min_iou < __builtin_inff())) return WD_ERR_BAD_ARG;
  if (!wd_aligned16(boxes) || !aligned4(ex_boxes) || !aligned4(ex_count) || !aligned4(meta) || !aligned4(sel_anchors) ||
      !aligned4(sel_iou) || !aligned4(sel_count))
    return WD_ERR_BAD_ARG;
  if ((long long)batch * n_anchor > 0x7ffffff0LL || batch > 65535) return WD_ERR_BAD_ARG;
  const dim3 grid((unsigned)max_ex, (unsigned)batch);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define WD_EX_CASE(M_) \
  case M_: launch_assign<M_>(grid, st, boxes, n_anchor, ex_boxes, ex_count, meta, max_ex, min_iou, sel_anchors, sel_iou, sel_count); break;
  switch (m) {
    WD_EX_CASE(1) WD_EX_CASE(2) WD_EX_CASE(3) WD_EX_CASE(4) WD_EX_CASE(5) WD_EX_CASE(6) WD_EX_CASE(7) WD_EX_CASE(8)
  }
#undef WD_EX_CASE
  return wd_launch_status();
}

extern "C" int wd_exemplar_pool(const float* level_embed, int32_t dim, int32_t off1, int32_t off2, const int32_t* sel_anchors,
                                const float* sel_iou, int32_t n_slot, const int32_t* cls_off, const int32_t* cls_slot, int32_t n_cls,
                                float* bank, int32_t* support, void* stream) {
  if (!level_embed || !sel_anchors || !sel_iou || !cls_off || !bank || !support) return WD_ERR_BAD_ARG;
  if (n_slot <= 0 || n_cls <= 0 || dim < 4 || dim > 1024 || dim % 4 || !(0 < off1 && off1 < off2)) return WD_ERR_BAD_ARG;
  if (!wd_aligned16(level_embed) || !wd_aligned16(bank) || !aligned4(sel_anchors) || !aligned4(sel_iou) || !aligned4(cls_off) ||
      !aligned4(cls_slot) || !aligned4(support))
    return WD_ERR_BAD_ARG;
  if (3LL * n_slot * dim > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(exemplar_pool_kernel, dim3((unsigned)n_cls), dim3(256), 0, static_cast<hipStream_t>(stream), level_embed, dim,
                     off1, off2, sel_anchors, sel_iou, n_slot, cls_off, cls_slot, bank, support);
  return wd_launch_status();
}
