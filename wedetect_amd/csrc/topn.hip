// topn.hip — the n_top best classes of every region row (include/wedetect_hip_topn.h) as 64-bit keys, n_top words per row.
//   wd_topn_similarity_split   the fp16x3 256 x 256 similarity launch with the top-n epilogue (split_gemm_p8.hip: p8_topn_epilogue)
//   wd_topn_rows               the same merge from a materialised block of scores or raw logits: one wave per row
//   wd_topn_unpack             one slot of every row -> (score, label)
//   wd_topn_kept               the lists of the rows NMS kept
#include "p8_score_launch.h"
#include "topn_key.h"
#include "wedetect_hip_topn.h"

namespace {

// One wave per row, one pass over the row's columns per slot: pass t finds the largest key below the one pass t - 1 found (keys of
// one row are distinct: the class is part of them), lane 0 offers it at slot t.  Keys come out in descending order, so the first
// one not above the bound ends the row.
template <bool AFFINE>
__global__ void __launch_bounds__(256) topn_rows_kernel(const float* __restrict__ block, long long rows, int rows_per_img, int n_cls,
                                                        int ld, int cls_offset, const int* __restrict__ count,
                                                        const float* __restrict__ row_scale, const float* __restrict__ row_bias,
                                                        int n_top, unsigned long long* key) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                        // wave-uniform
  int n = n_cls;
  if (count) {
    const int c = count[row / rows_per_img];
    n = c < n ? c : n;
  }
  if (n <= 0) return;
  const float* s = block + row * (long long)ld;
  float escale = 1.0f, bias = 0.0f;
  if (AFFINE) { escale = expf(row_scale[row]); bias = row_bias[row]; }
  const unsigned inv0 = 0xFFFFFFFFu - (unsigned)cls_offset;
  unsigned long long* slot = key + row * (long long)n_top;
  const unsigned long long bound = wd_topn_bound(slot, n_top);
  unsigned long long prev = ~0ull;
  for (int t = 0; t < n_top; ++t) {
    unsigned long long best = 0ull;
    for (int c = lane; c < n; c += 64) {
      const float x = AFFINE ? wd_topn_affine_score(s[c], escale, bias) : s[c];
      const unsigned long long k = ((unsigned long long)__float_as_uint(x) << 32) | (unsigned long long)(inv0 - (unsigned)c);
      best = (k < prev && k > best) ? k : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned lo = __shfl_xor((unsigned)best, o, 64), hi = __shfl_xor((unsigned)(best >> 32), o, 64);
      const unsigned long long k = ((unsigned long long)hi << 32) | lo;
      best = k > best ? k : best;
    }
    if (best <= bound) break;                                      // wave-uniform; 0 = the row has no further column
    if (lane == 0) wd_topn_offer(slot, n_top, t, best, bound);
    prev = best;
  }
}

__device__ __forceinline__ void topn_unpack_one(unsigned long long k, float& s, int& l) {
  s = k ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
  l = k ? (int)(0xFFFFFFFFu - (unsigned)k) : -1;
}

__global__ void __launch_bounds__(256) topn_unpack_kernel(const unsigned long long* __restrict__ key, long long rows, int n_top, int slot,
                                                          float* __restrict__ scores_out, int* __restrict__ labels_out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  topn_unpack_one(key[r * n_top + slot], scores_out[r], labels_out[r]);
}

__global__ void __launch_bounds__(256) topn_kept_kernel(const unsigned long long* __restrict__ key, int n_top, int n_anchor,
                                                        const int* __restrict__ out_anchors, const int* __restrict__ out_count,
                                                        int max_out, long long total, float* __restrict__ top_scores,
                                                        int* __restrict__ top_labels) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;   // element (b, i, j)
  if (e >= total) return;
  const int j = (int)(e % n_top);
  const long long bi = e / n_top;
  const int i = (int)(bi % max_out), b = (int)(bi / max_out);
  unsigned long long k = 0ull;
  if (i < out_count[b]) {
    const int a = out_anchors[bi];
    if ((unsigned)a < (unsigned)n_anchor) k = key[((long long)b * n_anchor + a) * n_top + j];
  }
  topn_unpack_one(k, top_scores[e], top_labels[e]);
}

bool topn_key_ok(const void* key, int n_top, long long rows, int cls_offset, int n_cls) {
  if (!key || (reinterpret_cast<uintptr_t>(key) & 7u) || n_top < 1 || n_top > WD_TOPN_MAX) return false;
  if (cls_offset < 0 || (long long)cls_offset + n_cls > 0x7fffffffLL) return false;
  return rows > 0 && rows * n_top <= 0x7ffffff0LL;
}

}  // namespace

extern "C" int wd_topn_abi_version(void) { return 1; }

extern "C" int wd_topn_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls,
                                        int32_t dim, int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale,
                                        const float* seg_bias, const float* row_scale, const float* row_bias, uint32_t* range_flag,
                                        int32_t cls_offset, int32_t n_top, uint64_t* key, void* stream) {
  WdConvGemm p;
  if (wd_similarity_problem(p, e_split, rows, t_split, unscale, n_cls, dim, seg_rows, seg_end0, seg_end1, seg_scale, seg_bias, 1, range_flag) != WD_OK)
    return WD_ERR_BAD_ARG;
  if (!topn_key_ok(key, n_top, rows, cls_offset, n_cls)) return WD_ERR_BAD_ARG;
  if ((row_scale == nullptr) != (row_bias == nullptr) || (row_scale && seg_rows > 0)) return WD_ERR_BAD_ARG;
  if (row_scale && ((reinterpret_cast<uintptr_t>(row_scale) | reinterpret_cast<uintptr_t>(row_bias)) & 3u)) return WD_ERR_BAD_ARG;
  if (!wd_similarity_bank_fits(n_cls, dim)) return WD_ERR_UNSUPPORTED;
  return wd_launch_p8_topn(p, t_split, unscale, reinterpret_cast<unsigned long long*>(key), n_top, cls_offset, row_scale, row_bias,
                           static_cast<hipStream_t>(stream));
}

extern "C" int wd_topn_rows(const float* block, int32_t n_img, int32_t rows_per_img, int32_t n_cls, int32_t ld, int32_t cls_offset,
                            const int32_t* count, const float* row_scale, const float* row_bias, int32_t n_top, uint64_t* key,
                            void* stream) {
  if (!block || n_img <= 0 || rows_per_img <= 0 || n_cls <= 0 || ld < n_cls) return WD_ERR_BAD_ARG;
  const long long rows = (long long)n_img * rows_per_img;
  if (!topn_key_ok(key, n_top, rows, cls_offset, n_cls) || (row_scale == nullptr) != (row_bias == nullptr)) return WD_ERR_BAD_ARG;
  const dim3 grid((unsigned)((rows + 3) / 4));
  unsigned long long* k = reinterpret_cast<unsigned long long*>(key);
  if (row_scale)
    hipLaunchKernelGGL(topn_rows_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), block, rows, rows_per_img, n_cls,
                       ld, cls_offset, count, row_scale, row_bias, n_top, k);
  else
    hipLaunchKernelGGL(topn_rows_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), block, rows, rows_per_img, n_cls,
                       ld, cls_offset, count, row_scale, row_bias, n_top, k);
  return wd_launch_status();
}

extern "C" int wd_topn_unpack(const uint64_t* key, int64_t rows, int32_t n_top, int32_t slot, float* scores_out, int32_t* labels_out,
                              void* stream) {
  if (!key || !scores_out || !labels_out || rows <= 0 || n_top < 1 || n_top > WD_TOPN_MAX || slot < 0 || slot >= n_top) return WD_ERR_BAD_ARG;
  if (rows * n_top > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(topn_unpack_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long*>(key), (long long)rows, n_top, slot, scores_out, labels_out);
  return wd_launch_status();
}

extern "C" int wd_topn_kept(const uint64_t* key, int32_t n_top, int32_t n_anchor, const int32_t* out_anchors, const int32_t* out_count,
                            int32_t max_out, int32_t batch, float* top_scores, int32_t* top_labels, void* stream) {
  if (!key || !out_anchors || !out_count || !top_scores || !top_labels) return WD_ERR_BAD_ARG;
  if (n_top < 1 || n_top > WD_TOPN_MAX || n_anchor <= 0 || max_out <= 0 || batch <= 0) return WD_ERR_BAD_ARG;
  const long long total = (long long)batch * max_out * n_top;
  if (total > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(topn_kept_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long*>(key), n_top, n_anchor, out_anchors, out_count, max_out, total,
                     top_scores, top_labels);
  return wd_launch_status();
}
