// p8_score_launch.h — the similarity and retrieval launches of the 256 x 256 pre-split kernel, defined in split_gemm_p8.hip and called
// by the extern "C" entries of split_gemm_pre.hip, best.hip, sparse.hip, topn.hip and groups.hip.
#pragma once
#include "common.h"

// what every similarity launch needs: K in whole 32-column steps, row groups of eight, aligned bases, no epilogue but affine + sigmoid
static inline bool p8_similarity_ok(const WdConvGemm& p, const void* t_split) {
  if (p.k % 32 || p.k < 32 || p.lda % 8 || !wd_aligned16(p.a) || !wd_aligned16(t_split)) return false;
  return !(p.res || p.c2 || p.bias || p.act != WD_ACT_NONE || p.out_mode != WD_OUT_ROWS || p.c_batch_stride > 0 || p.ln_stats);
}

// p and t_split as wd_similarity_problem (common.h) leaves them; the fused forms need p.sigmoid and ignore p.c.  The callers have
// checked wd_similarity_bank_fits and their own arguments.
int wd_launch_p8_similarity(const WdConvGemm& p, const void* t_split, float unscale, hipStream_t st);
int wd_launch_p8_best(const WdConvGemm& p, const void* t_split, float unscale, unsigned long long* key, int cls_offset, hipStream_t st);
int wd_launch_p8_sparse(const WdConvGemm& p, const void* t_split, float unscale, unsigned long long* list, int list_cap, int* state,
                        int rows_per_img, int n_cls_total, int cls_offset, float thr, hipStream_t st);
int wd_launch_p8_topn(const WdConvGemm& p, const void* t_split, float unscale, unsigned long long* key, int n_top, int cls_offset,
                      const float* row_scale, const float* row_bias, hipStream_t st);
int wd_launch_p8_group(const WdConvGemm& p, const void* t_split, float unscale, const int* group_of, const int* bin_first, int cls_offset,
                       float* out, int ldo, int n_groups, hipStream_t st);
// operand roles swapped (P8RetrMax): bank rows [n_cls][dim] x region rows [n_rows][dim]; out [images][ldo] must be zero
int wd_launch_p8_retrieval(const void* t_split, int n_cls, const void* e_split, int n_rows, int dim, float unscale,
                           const float* scale, const float* bias, const int* count, int rows_per_img, float* out, int ldo,
                           unsigned* range_flag, hipStream_t st);
