// groups.hip — prompt groups (include/wedetect_hip_groups.h): a class scored as the best of its prompts, [rows][n_groups] scores.
//   wd_group_similarity_split   the fp16x3 256 x 256 similarity launch with the class-max epilogue (split_gemm_p8.hip: p8_group_epilogue)
//   wd_group_rows               the same maxima from a materialised block of scores: a (row, class of the bin) pair per lane
#include "p8_score_launch.h"
#include "wedetect_hip_groups.h"

namespace {

// One workgroup per (8 rows, bin): thread = (row r8 = t >> 5, class k = t & 31 of the bin).  The bin is the same for the whole
// workgroup, so its 32 group_of words are uniform loads; a thread counts the columns in front of its class and those of it, reads
// them from the block row and stores the maximum at out[row][first class of the bin + k]: 32 consecutive lanes, one row segment.
// A NaN is kept (the fp32 tower's non-finite rows must reach wd_topk_candidates).
__global__ void __launch_bounds__(256) group_rows_kernel(const float* __restrict__ block, long long rows, int ld,
                                                         const int* __restrict__ group_of, const int* __restrict__ bin_first,
                                                         int cls_offset, float* __restrict__ out, int ldo, int n_groups) {
  const int bin = blockIdx.y;                                      // of this launch
  const int abin = (cls_offset >> 5) + bin;
  const int g0 = bin_first[abin];
  int ng = bin_first[abin + 1] - g0;
  ng = ng < 0 ? 0 : (ng > 32 ? 32 : ng);
  const int k = threadIdx.x & 31;
  const long long row = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int* __restrict__ go = group_of + cls_offset + 32 * bin;
  const int mine = g0 + k;
  int start = 0, end = 0;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const int gc = go[c];
    start += gc < mine ? 1 : 0;
    end += gc <= mine ? 1 : 0;
  }
  if (row >= rows || k >= ng || end <= start || g0 < 0 || mine >= n_groups) return;   // the last three: a table that is not a plan's
  const float* __restrict__ s = block + row * (long long)ld + 32 * bin;
  float v = s[start];
  for (int c = start + 1; c < end; ++c) {
    const float x = s[c];
    v = (x > v || x != x) ? x : v;                                 // max; a NaN sticks
  }
  out[row * (long long)ldo + mine] = v;
}

bool group_args_ok(const void* group_of, const void* bin_first, int cls_offset, int n_cls, const void* out, int ldo, int n_groups) {
  if (!group_of || !bin_first || !out || n_cls <= 0 || n_groups <= 0 || ldo < n_groups) return false;
  if (cls_offset < 0 || (cls_offset & 31) || (n_cls & 31) || (long long)cls_offset + n_cls > 0x7fffffffLL) return false;
  return ((reinterpret_cast<uintptr_t>(group_of) | reinterpret_cast<uintptr_t>(bin_first) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0;
}

}  // namespace

extern "C" int wd_groups_abi_version(void) { return 1; }

extern "C" int wd_group_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls, int32_t dim,
                                         int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale,
                                         const float* seg_bias, uint32_t* range_flag, const int32_t* group_of, const int32_t* bin_first,
                                         int32_t cls_offset, float* out, int32_t ldo, int32_t n_groups, void* stream) {
  WdConvGemm p;
  if (wd_similarity_problem(p, e_split, rows, t_split, unscale, n_cls, dim, seg_rows, seg_end0, seg_end1, seg_scale, seg_bias, 1, range_flag) != WD_OK)
    return WD_ERR_BAD_ARG;
  if (!group_args_ok(group_of, bin_first, cls_offset, n_cls, out, ldo, n_groups)) return WD_ERR_BAD_ARG;
  if (!wd_similarity_bank_fits(n_cls, dim)) return WD_ERR_UNSUPPORTED;
  return wd_launch_p8_group(p, t_split, unscale, group_of, bin_first, cls_offset, out, ldo, n_groups, static_cast<hipStream_t>(stream));
}

extern "C" int wd_group_rows(const float* block, int64_t rows, int32_t n_cls, int32_t ld, const int32_t* group_of, const int32_t* bin_first,
                             int32_t cls_offset, float* out, int32_t ldo, int32_t n_groups, void* stream) {
  if (!block || rows <= 0 || rows > 0x7ffffff0LL || ld < n_cls || (reinterpret_cast<uintptr_t>(block) & 3u)) return WD_ERR_BAD_ARG;
  if (!group_args_ok(group_of, bin_first, cls_offset, n_cls, out, ldo, n_groups) || n_cls / 32 > 65535) return WD_ERR_BAD_ARG;
  const dim3 grid((unsigned)((rows + 7) / 8), (unsigned)(n_cls / 32));
  hipLaunchKernelGGL(group_rows_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), block, (long long)rows, ld, group_of,
                     bin_first, cls_offset, out, ldo, n_groups);
  return wd_launch_status();
}
