// fold.hip — the kept-row half of the folded text bank (include/wedetect_hip_fold.h): with the bank folded into the head's
// embedding conv the step never computes the [B, anchors, 768] embedding tensor; the 768-d embeddings of the <= max_out rows
// per image that wd_nms_gather keeps are computed afterwards by the SAME GEMM the embedding conv runs on, on the kept rows'
// c2 inputs.  The two kernels here move rows: gather the kept c2 rows grouped by head level (a level's GEMM has that level's
// weights), and pick every kept row's embedding from its level's GEMM output; a third gives the kept rows the scores and the
// order of the unfolded similarity GEMM, run on their embeddings.  (wd_fold_similarity lives in split_gemm.hip,
// next to the dispatcher whose argument checks it shares.)
#include "common.h"
#include "wedetect_hip_fold.h"

namespace {

// one wave per (kept slot, image, level): a c2 row is row_floats * 4 bytes (1 KB at 256 channels: one 16-byte load per lane)
__global__ void __launch_bounds__(64) kept_rows_gather_kernel(const float* __restrict__ c0, const float* __restrict__ c1,
                                                              const float* __restrict__ c2, int rows0, int rows1, int rows2,
                                                              int row_floats, const int* __restrict__ out_anchors,
                                                              const int* __restrict__ out_count, int max_out, int batch,
                                                              float* __restrict__ gathered) {
  const int s = blockIdx.x, b = blockIdx.y, l = blockIdx.z, lane = threadIdx.x;
  float* dst = gathered + (((size_t)l * batch + b) * max_out + s) * row_floats;
  const int a = out_anchors[(size_t)b * max_out + s];
  const int lvl = (a >= rows0) + (a >= rows0 + rows1);
  const bool take = s < out_count[b] && a >= 0 && a < rows0 + rows1 + rows2 && lvl == l;     // wave-uniform
  if (take) {
    const float* base = l == 0 ? c0 : l == 1 ? c1 : c2;
    const int rows = l == 0 ? rows0 : l == 1 ? rows1 : rows2;
    const int pos = a - (l == 0 ? 0 : l == 1 ? rows0 : rows0 + rows1);
    const float* src = base + ((size_t)b * rows + pos) * row_floats;
    for (int i = lane * 4; i < row_floats; i += 256) *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(src + i);
  } else {
    for (int i = lane * 4; i < row_floats; i += 256) *reinterpret_cast<f32x4*>(dst + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

__global__ void __launch_bounds__(64) kept_rows_select_kernel(const float* __restrict__ level_embed, int dim, int off1, int off2,
                                                              const int* __restrict__ out_anchors,
                                                              const int* __restrict__ out_count, const int* __restrict__ perm,
                                                              int max_out, int batch, float* __restrict__ out_embed) {
  const int s = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const size_t r = (size_t)b * max_out + s;
  float* dst = out_embed + r * dim;
  if (s < out_count[b]) {
    const int a = out_anchors[r];
    const int lvl = (a >= off1) + (a >= off2);
    int from = perm ? perm[r] : s;           // the slot the row had when the GEMMs ran (wd_kept_rows_reorder)
    from = min(max(from, 0), max_out - 1);
    const float* src = level_embed + (((size_t)lvl * batch + b) * max_out + from) * dim;
    for (int i = lane * 4; i < dim; i += 256) *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(src + i);
  } else {
    for (int i = lane * 4; i < dim; i += 256) *reinterpret_cast<f32x4*>(dst + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

constexpr int KEPT_MAX = 1024;      // wd_nms_gather's own limit on max_out

// one workgroup per image: the kept rows take the scores of the unfolded similarity GEMM (level_scores) and the order
// wd_topk_candidates gives rows of those scores: score descending, flat index anchor * k + label ascending
__global__ void __launch_bounds__(256) kept_rows_reorder_kernel(const float* __restrict__ level_scores, int k, int n_anchor,
                                                                int off1, int off2, float* __restrict__ out_boxes,
                                                                float* __restrict__ out_scores, int* __restrict__ out_labels,
                                                                int* __restrict__ out_anchors,
                                                                const int* __restrict__ out_count, int max_out, int batch,
                                                                int* __restrict__ perm) {
  __shared__ f32x4 s_box[KEPT_MAX];
  __shared__ float s_score[KEPT_MAX];
  __shared__ int s_label[KEPT_MAX], s_anchor[KEPT_MAX];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)b * max_out;
  const int n = min(max(out_count[b], 0), max_out);
  for (int s = tid; s < n; s += 256) {
    const int a = out_anchors[base + s], c = out_labels[base + s];
    float sc = out_scores[base + s];
    if (a >= 0 && a < n_anchor && c >= 0 && c < k) {
      const int lvl = (a >= off1) + (a >= off2);
      sc = level_scores[(((size_t)lvl * batch + b) * max_out + s) * k + c];
    }
    s_score[s] = sc; s_label[s] = c; s_anchor[s] = a;
    s_box[s] = *reinterpret_cast<const f32x4*>(out_boxes + (base + s) * 4);
  }
  __syncthreads();      // every slot < n is staged: the in-place writes below cannot overtake a read
  for (int s = tid; s < n; s += 256) {
    const float sc = s_score[s];
    const long long idx = (long long)s_anchor[s] * k + s_label[s];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = s_score[j];
      const long long ij = (long long)s_anchor[j] * k + s_label[j];
      rank += (sj > sc || (sj == sc && (ij < idx || (ij == idx && j < s)))) ? 1 : 0;
    }
    // ranks are a permutation of 0 .. n - 1 for ordered scores; a NaN (never kept: wd_topk_candidates flags the image) could
    // only repeat a rank, never leave the image's rows
    *reinterpret_cast<f32x4*>(out_boxes + (base + rank) * 4) = s_box[s];
    out_scores[base + rank] = sc;
    out_labels[base + rank] = s_label[s];
    out_anchors[base + rank] = s_anchor[s];
    perm[base + rank] = s;
  }
  for (int s = n + tid; s < max_out; s += 256) perm[base + s] = s;
}

}  // namespace

extern "C" int wd_fold_abi_version(void) { return 1; }

extern "C" int wd_kept_rows_gather(const float* c2_0, const float* c2_1, const float* c2_2, int32_t rows0, int32_t rows1,
                                   int32_t rows2, int32_t row_floats, const int32_t* out_anchors, const int32_t* out_count,
                                   int32_t max_out, int32_t batch, float* gathered, void* stream) {
  if (!c2_0 || !c2_1 || !c2_2 || !out_anchors || !out_count || !gathered) return WD_ERR_BAD_ARG;
  if (rows0 <= 0 || rows1 <= 0 || rows2 <= 0 || (long long)rows0 + rows1 + rows2 > 0x7fffffffLL) return WD_ERR_BAD_ARG;
  if (row_floats < 4 || row_floats > 1024 || (row_floats & 3) || max_out <= 0 || max_out > 65535 || batch <= 0 || batch > 65535)
    return WD_ERR_BAD_ARG;
  if (!wd_aligned16(c2_0) || !wd_aligned16(c2_1) || !wd_aligned16(c2_2) || !wd_aligned16(gathered)) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(kept_rows_gather_kernel, dim3(max_out, batch, 3), dim3(64), 0, static_cast<hipStream_t>(stream), c2_0, c2_1,
                     c2_2, rows0, rows1, rows2, row_floats, out_anchors, out_count, max_out, batch, gathered);
  return wd_launch_status();
}

extern "C" int wd_kept_rows_select(const float* level_embed, int32_t dim, int32_t off1, int32_t off2, const int32_t* out_anchors,
                                   const int32_t* out_count, const int32_t* perm, int32_t max_out, int32_t batch,
                                   float* out_embed, void* stream) {
  if (!level_embed || !out_anchors || !out_count || !out_embed) return WD_ERR_BAD_ARG;
  if (dim <= 0 || (dim & 3) || off1 < 0 || off2 < off1 || max_out <= 0 || max_out > 65535 || batch <= 0 || batch > 65535)
    return WD_ERR_BAD_ARG;
  if (!wd_aligned16(level_embed) || !wd_aligned16(out_embed)) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(kept_rows_select_kernel, dim3(max_out, batch), dim3(64), 0, static_cast<hipStream_t>(stream), level_embed,
                     dim, off1, off2, out_anchors, out_count, perm, max_out, batch, out_embed);
  return wd_launch_status();
}

extern "C" int wd_kept_rows_reorder(const float* level_scores, int32_t k, int32_t n_anchor, int32_t off1, int32_t off2,
                                    float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* out_anchors,
                                    const int32_t* out_count, int32_t max_out, int32_t batch, int32_t* perm, void* stream) {
  if (!level_scores || !out_boxes || !out_scores || !out_labels || !out_anchors || !out_count || !perm) return WD_ERR_BAD_ARG;
  if (k <= 0 || n_anchor <= 0 || off1 < 0 || off2 < off1 || off2 > n_anchor || max_out <= 0 || max_out > KEPT_MAX || batch <= 0 ||
      batch > 65535)
    return WD_ERR_BAD_ARG;
  if (!wd_aligned16(out_boxes)) return WD_ERR_BAD_ARG;
  hipLaunchKernelGGL(kept_rows_reorder_kernel, dim3(batch), dim3(256), 0, static_cast<hipStream_t>(stream), level_scores, k,
                     n_anchor, off1, off2, out_boxes, out_scores, out_labels, out_anchors, out_count, max_out, batch, perm);
  return wd_launch_status();
}
