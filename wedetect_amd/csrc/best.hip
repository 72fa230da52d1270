// best.hip — single-label detection (include/wedetect_hip_best.h): best class per region row as 64-bit keys.
//   wd_best_similarity_split   the fp16x3 256 x 256 similarity launch with the key epilogue (split_gemm_p8.hip: p8_best_epilogue)
//   wd_best_rows               the same merge from a materialised score block: one wave per row
//   wd_best_unpack             keys -> (score, label)
// (wd_nms_gather_labeled lives beside the kernel it is a form of: postprocess.hip.)
#include "p8_score_launch.h"
#include "wedetect_hip_best.h"

namespace {

// key = score bits << 32 | (0xFFFFFFFF - class): unsigned max = highest score, lowest class among equal scores
__global__ void __launch_bounds__(256) best_rows_kernel(const float* __restrict__ scores, long long rows, int rows_per_img,
                                                        int n_cls, int ld, int cls_offset, const int* __restrict__ count,
                                                        unsigned long long* __restrict__ key) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                        // wave-uniform
  int n = n_cls;
  if (count) {
    const int c = count[row / rows_per_img];
    n = c < n ? c : n;
  }
  const float* s = scores + row * (long long)ld;
  const unsigned inv0 = 0xFFFFFFFFu - (unsigned)cls_offset;
  unsigned long long best = 0ull;
  for (int c = lane; c < n; c += 64) {
    const unsigned long long k = ((unsigned long long)__float_as_uint(s[c]) << 32) | (unsigned long long)(inv0 - (unsigned)c);
    best = k > best ? k : best;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)best, o, 64), hi = __shfl_xor((unsigned)(best >> 32), o, 64);
    const unsigned long long k = ((unsigned long long)hi << 32) | lo;
    best = k > best ? k : best;
  }
  if (lane == 0 && best != 0ull) atomicMax(key + row, best);
}

__global__ void __launch_bounds__(256) best_unpack_kernel(const unsigned long long* __restrict__ key, long long rows,
                                                          float* __restrict__ scores_out, int* __restrict__ labels_out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const unsigned long long k = key[r];
  scores_out[r] = k ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
  labels_out[r] = k ? (int)(0xFFFFFFFFu - (unsigned)k) : -1;
}

}  // namespace

extern "C" int wd_best_abi_version(void) { return 1; }

extern "C" int wd_best_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls,
                                        int32_t dim, int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale,
                                        const float* seg_bias, uint32_t* range_flag, int32_t cls_offset, uint64_t* key,
                                        void* stream) {
  WdConvGemm p;
  if (wd_similarity_problem(p, e_split, rows, t_split, unscale, n_cls, dim, seg_rows, seg_end0, seg_end1, seg_scale, seg_bias, 1, range_flag) != WD_OK)
    return WD_ERR_BAD_ARG;
  if (!key || cls_offset < 0 || (long long)cls_offset + n_cls > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(key) & 7u)) return WD_ERR_BAD_ARG;
  if (!wd_similarity_bank_fits(n_cls, dim)) return WD_ERR_UNSUPPORTED;
  return wd_launch_p8_best(p, t_split, unscale, reinterpret_cast<unsigned long long*>(key), cls_offset,
                           static_cast<hipStream_t>(stream));
}

extern "C" int wd_best_rows(const float* scores, int32_t n_img, int32_t rows_per_img, int32_t n_cls, int32_t ld, int32_t cls_offset,
                            const int32_t* count, uint64_t* key, void* stream) {
  if (!scores || !key || n_img <= 0 || rows_per_img <= 0 || n_cls <= 0 || ld < n_cls) return WD_ERR_BAD_ARG;
  if (cls_offset < 0 || (long long)cls_offset + n_cls > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(key) & 7u)) return WD_ERR_BAD_ARG;
  const long long rows = (long long)n_img * rows_per_img;
  if (rows > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(best_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), scores, rows,
                     rows_per_img, n_cls, ld, cls_offset, count, reinterpret_cast<unsigned long long*>(key));
  return wd_launch_status();
}

extern "C" int wd_best_unpack(const uint64_t* key, int64_t rows, float* scores_out, int32_t* labels_out, void* stream) {
  if (!key || !scores_out || !labels_out || rows <= 0 || rows > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(best_unpack_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long*>(key), (long long)rows, scores_out, labels_out);
  return wd_launch_status();
}
