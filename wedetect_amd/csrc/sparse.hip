// sparse.hip — multi-label detection without the score tensor (include/wedetect_hip_sparse.h): the (anchor, class) pairs with
// score > thr as per-image lists of 64-bit keys (~score bits << 32 | flat index), the key wd_topk_candidates sorts by.
//   wd_sparse_similarity_split   the fp16x3 256 x 256 similarity launch with the candidate epilogue (split_gemm_p8.hip: p8_sparse_epilogue)
//   wd_sparse_rows               the same append from a materialised score block: one wave per row
//   wd_sparse_select             per-image sort of the list (bitonic.h: LDS chunks + global strides) and the unpack into the
//                                buffers wd_nms_gather reads
#include "bitonic.h"
#include "p8_score_launch.h"
#include "wedetect_hip_sparse.h"

namespace {

constexpr int SORT_CHUNK = 8192;          // keys sorted per LDS visit (64 KB), as in the top-k sort
constexpr int MAX_LIST_CAP = 1 << 20;

// one wave per row; per 64 columns the lanes that hold a candidate take consecutive slots behind ONE atomic of the first of them
__global__ void __launch_bounds__(256) sparse_rows_kernel(const float* __restrict__ scores, long long rows, int rows_per_img,
                                                          int n_cls, int ld, int cls_offset, const int* __restrict__ count,
                                                          int n_cls_total, float thr, unsigned long long* __restrict__ list,
                                                          unsigned cap, int* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                        // wave-uniform
  const int b = (int)(row / rows_per_img);
  int n = n_cls;
  if (count) {
    const int c = count[b];
    n = c < n ? c : n;
  }
  const float* s = scores + row * (long long)ld;
  const unsigned flat0 = (unsigned)(row - (long long)b * rows_per_img) * (unsigned)n_cls_total + (unsigned)cls_offset;
  unsigned long long* lb = list + (size_t)b * cap;
  bool bad = false;
  for (int c0 = 0; c0 < n; c0 += 64) {                            // wave-uniform trip count
    const int c = c0 + lane;
    float v = 0.f;
    if (c < n) v = s[c];
    const unsigned bits = __float_as_uint(v);
    bad |= (bits & 0x7F800000u) == 0x7F800000u;
    const bool pass = c < n && v > thr;
    const unsigned long long m = __ballot(pass);
    if (m == 0ull) continue;
    const unsigned before = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    const int leader = __ffsll((long long)m) - 1;
    unsigned base = 0u;
    if (lane == leader) base = (unsigned)atomicAdd(state + 2 * b, (int)__popcll(m));
    base = __shfl(base, leader, 64);
    const unsigned pos = base + before;
    if (pass && pos < cap) lb[pos] = ((unsigned long long)(~bits) << 32) | (unsigned long long)(flat0 + (unsigned)c);
  }
  if (bad) state[2 * b + 1] = 1;                                  // sticky, benign race
}

// n2 of image b: the power of two the sort works on; 0 = nothing to sort (no candidates, overflow or a non-finite image)
__device__ __forceinline__ int select_n2(const int* __restrict__ state, int b, int cap) {
  const int n = state[2 * b];
  if (state[2 * b + 1] != 0 || n <= 0 || n > cap) return 0;
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  return n2;
}

// list[b][n, n2) = ~0: pad keys sort last
__global__ void __launch_bounds__(256) sparse_pad_kernel(unsigned long long* __restrict__ list, int cap, const int* __restrict__ state) {
  const int b = blockIdx.y;
  const int n2 = select_n2(state, b, cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n2) return;
  if (i >= state[2 * b]) list[(size_t)b * cap + i] = ~0ull;
}

// size == 0: full local sort of the chunk; size > chunk: the strides below a chunk of the merge of width `size`
__global__ void __launch_bounds__(1024) sparse_sort_chunk_kernel(unsigned long long* __restrict__ list, int cap,
                                                                 const int* __restrict__ state, int size) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
  const int b = blockIdx.y, t = threadIdx.x;
  const int n2 = select_n2(state, b, cap);
  const int chunk = n2 < SORT_CHUNK ? n2 : SORT_CHUNK;
  const int base = blockIdx.x * SORT_CHUNK;
  if (base >= n2 || (size != 0 && size > n2)) return;             // workgroup-uniform
  unsigned long long* k = list + (size_t)b * cap + base;
  for (int i = t; i < chunk; i += 1024) sk[i] = k[i];
  __syncthreads();
  if (size == 0) {
    for (int sz = 2; sz <= chunk; sz <<= 1)
      for (int jj = sz >> 1; jj > 0; jj >>= 1) wd_lds_bitonic_pass<1024>(sk, chunk, base, jj, sz);
  } else {
    for (int jj = chunk >> 1; jj > 0; jj >>= 1) wd_lds_bitonic_pass<1024>(sk, chunk, base, jj, size);
  }
  for (int i = t; i < chunk; i += 1024) k[i] = sk[i];
}

// one global-memory stage (stride j >= SORT_CHUNK) of the merge of width `size`
__global__ void __launch_bounds__(256) sparse_sort_global_kernel(unsigned long long* __restrict__ list, int cap,
                                                                 const int* __restrict__ state, int size, int j) {
  const int b = blockIdx.y;
  const int n2 = select_n2(state, b, cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (size > n2 || i >= n2) return;
  wd_global_bitonic_step(list + (size_t)b * cap, i, j, size);
}

__global__ void __launch_bounds__(256) sparse_unpack_kernel(const unsigned long long* __restrict__ list, int cap,
                                                            const int* __restrict__ state, int nms_pre, int out_cap,
                                                            int* __restrict__ out_idx, float* __restrict__ out_score,
                                                            int* __restrict__ out_count, int* __restrict__ status) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = state[2 * b];
  const bool nonfinite = state[2 * b + 1] != 0, overflow = n > cap;
  const int want = (nonfinite || overflow || n <= 0) ? 0 : (n < nms_pre ? n : nms_pre);
  if (i < out_cap) {
    if (i < want) {
      const unsigned long long ck = list[(size_t)b * cap + i];
      out_idx[(size_t)b * out_cap + i] = (int)(unsigned)(ck & 0xFFFFFFFFull);
      out_score[(size_t)b * out_cap + i] = __uint_as_float(~(unsigned)(ck >> 32));
    } else {
      out_idx[(size_t)b * out_cap + i] = -1;
      out_score[(size_t)b * out_cap + i] = 0.f;
    }
  }
  if (i == 0) {
    out_count[b] = nonfinite ? -1 : want;
    status[b] = nonfinite ? WD_SPARSE_NONFINITE : overflow ? WD_SPARSE_OVERFLOW : WD_SPARSE_OK;
  }
}

bool bad_list(const void* list, int list_cap, const void* state) {
  return !list || !state || list_cap <= 0 || list_cap > MAX_LIST_CAP || (list_cap & (list_cap - 1)) ||
         (reinterpret_cast<uintptr_t>(list) & 7u) || (reinterpret_cast<uintptr_t>(state) & 3u);
}

}  // namespace

extern "C" int wd_sparse_abi_version(void) { return 1; }

extern "C" int wd_sparse_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls,
                                          int32_t dim, int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale,
                                          const float* seg_bias, uint32_t* range_flag, int32_t cls_offset, int32_t rows_per_img,
                                          int32_t n_cls_total, float thr, uint64_t* list, int32_t list_cap, int32_t* state,
                                          void* stream) {
  WdConvGemm p;
  if (wd_similarity_problem(p, e_split, rows, t_split, unscale, n_cls, dim, seg_rows, seg_end0, seg_end1, seg_scale, seg_bias, 1, range_flag) != WD_OK)
    return WD_ERR_BAD_ARG;
  if (bad_list(list, list_cap, state) || rows_per_img <= 0 || rows % rows_per_img || n_cls_total <= 0) return WD_ERR_BAD_ARG;
  if (cls_offset < 0 || (long long)cls_offset + n_cls > (long long)n_cls_total) return WD_ERR_BAD_ARG;
  if ((long long)rows_per_img * n_cls_total >= (1LL << 31)) return WD_ERR_UNSUPPORTED;
  if (!wd_similarity_bank_fits(n_cls, dim)) return WD_ERR_UNSUPPORTED;
  return wd_launch_p8_sparse(p, t_split, unscale, reinterpret_cast<unsigned long long*>(list), list_cap, state, rows_per_img,
                             n_cls_total, cls_offset, thr, static_cast<hipStream_t>(stream));
}

extern "C" int wd_sparse_rows(const float* scores, int32_t n_img, int32_t rows_per_img, int32_t n_cls, int32_t ld, int32_t cls_offset,
                              const int32_t* count, int32_t n_cls_total, float thr, uint64_t* list, int32_t list_cap,
                              int32_t* state, void* stream) {
  if (!scores || n_img <= 0 || rows_per_img <= 0 || n_cls <= 0 || ld < n_cls || n_cls_total <= 0) return WD_ERR_BAD_ARG;
  if (bad_list(list, list_cap, state)) return WD_ERR_BAD_ARG;
  if (cls_offset < 0 || (long long)cls_offset + n_cls > (long long)n_cls_total) return WD_ERR_BAD_ARG;
  if ((long long)rows_per_img * n_cls_total >= (1LL << 31)) return WD_ERR_UNSUPPORTED;
  const long long rows = (long long)n_img * rows_per_img;
  if (rows > 0x7ffffff0LL) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(sparse_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), scores, rows,
                     rows_per_img, n_cls, ld, cls_offset, count, n_cls_total, thr, reinterpret_cast<unsigned long long*>(list),
                     (unsigned)list_cap, state);
  return wd_launch_status();
}

extern "C" int wd_sparse_select(uint64_t* list, int32_t list_cap, const int32_t* state, int32_t batch, int32_t nms_pre,
                                int32_t* out_idx, float* out_score, int32_t* out_count, int32_t* status, void* stream) {
  if (!out_idx || !out_score || !out_count || !status) return WD_ERR_BAD_ARG;
  if (bad_list(list, list_cap, state) || batch <= 0 || batch > 65535 || nms_pre <= 0 || nms_pre > (1 << 20)) return WD_ERR_BAD_ARG;
  const int out_cap = wd_topk_capacity(nms_pre);
  if (list_cap < out_cap) return WD_ERR_BAD_ARG;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(list);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nchunk = (list_cap + SORT_CHUNK - 1) / SORT_CHUNK;
  const dim3 gch(nchunk, batch), gel((list_cap + 255) / 256, batch), gout((out_cap + 255) / 256, batch);
  hipLaunchKernelGGL(sparse_pad_kernel, gel, dim3(256), 0, st, keys, list_cap, state);
  hipLaunchKernelGGL(sparse_sort_chunk_kernel, gch, dim3(1024), SORT_CHUNK * 8, st, keys, list_cap, state, 0);
  for (int size = 2 * SORT_CHUNK; size <= list_cap; size <<= 1) {
    for (int j = size >> 1; j >= SORT_CHUNK; j >>= 1)
      hipLaunchKernelGGL(sparse_sort_global_kernel, gel, dim3(256), 0, st, keys, list_cap, state, size, j);
    hipLaunchKernelGGL(sparse_sort_chunk_kernel, gch, dim3(1024), SORT_CHUNK * 8, st, keys, list_cap, state, size);
  }
  hipLaunchKernelGGL(sparse_unpack_kernel, gout, dim3(256), 0, st, keys, list_cap, state, nms_pre, out_cap, out_idx, out_score,
                     out_count, status);
  return wd_launch_status();
}
