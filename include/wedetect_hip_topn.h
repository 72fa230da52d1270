/*
 * wedetect_hip_topn.h — the few best names of a region ("top-n") of libwedetect_hip.so (MI355X / gfx950 only): the n_top best rows
 * of a text bank for every region row, 1 <= n_top <= 8, without the [rows, n_cls] score tensor.  The best-class step of
 * wedetect_hip_best.h keeps the winner only; in a bank of 13 k names the near-winners are its synonyms and hypernyms.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_topn_abi_version), like wedetect_hip_best.h and the other
 * add-on headers: the entry points below are compiled into the same library and follow the same conventions — plain C types,
 * device pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no mutable global state,
 * WD_OK or a negative WD_ERR_* code (wedetect_hip.h).
 *
 * Result definition (every path).  For region row r, a bank of K rows and n = n_top:
 *     top[r][0 .. min(n, K)) = the pairs (score[r][c], c) sorted by SCORE DESCENDING, CLASS ASCENDING
 * where score[r][c] is exactly the fp32 value the materialising similarity launch would have stored for the same operands (the
 * sigmoid per element, as in wedetect_hip_best.h).  Slots j >= min(n, K) are empty and unpack to (0.0f, -1).
 *
 * The key is the best-class key: (uint64) bits(score) << 32 | (0xFFFFFFFF - class).  Row r owns n consecutive words
 * key[r * n + j]; slot 0 is the best-class key of the row, bit for bit.  0 = empty.  The CALLER clears the keys (a memset on the
 * same stream) before the first producer of a step.
 *
 * The merge.  A producer offers a key k to a row with
 *     carry = k;  for j in 0 .. n-1:  old = atomic_max_u64(&slot[j], carry);  carry = min(old, carry)
 * A slot only ever grows and hands the loser down, so slot j ends as the (j+1)-th largest key ever offered, whatever the
 * interleaving: a bank may be cut into any launches in any order and the result has the same bits.  Any earlier value of
 * slot[n-1] is a lower bound of its final value, so keys not above one are dropped before any atomic.
 * Unlike a maximum the merge is NOT idempotent: a class offered twice in a step takes two slots.  The chunks of a step must be
 * DISJOINT class ranges.
 *
 * Non-finite: an inf / NaN accumulator raises *range_flag and gives the row non-finite score bits in slot 0 (so
 * wd_topk_candidates reports the image); the other slots of such a row are unspecified.
 *
 *   wd_topn_similarity_split   fp16x3 region x text GEMM whose epilogue merges into the keys (no score tensor)
 *   wd_topn_rows               the same merge from a materialised [rows][ld] block of scores or of raw logits
 *   wd_topn_unpack             one slot of every row -> (score fp32, label int32)
 *   wd_topn_kept               the lists of the rows NMS kept
 */
#ifndef WEDETECT_HIP_TOPN_H
#define WEDETECT_HIP_TOPN_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_TOPN_MAX 8

/* Bumped on any change of a signature below. */
int wd_topn_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * wd_topn_similarity_split — operands exactly as wd_best_similarity_split (wedetect_hip_best.h): e_split, rows, t_split,
 * unscale, n_cls, dim, the per-level affine seg_* (seg_rows = 0: none), optional range_flag, cls_offset.  In addition:
 *
 *   row_scale, row_bias   device fp32 [rows], 4-byte aligned, or both NULL: the per-region affine of the retrieval scripts,
 *                         score = sigmoid(logit * exp(row_scale[r]) + row_bias[r]).  Exclusive with the seg affine.
 *   n_top                 1 .. WD_TOPN_MAX
 *   key                   device uint64 [rows][n_top], 8-byte aligned: merged into, see above
 *
 * Runs the 256 x 256 fp16x3 kernel of wd_similarity_split with another epilogue: the same K loop, the same per-element
 * expression, so score bits equal that entry point's output.  A lane holds one region row and 32 classes: it reads the row's last
 * slot once (a device-scope load), selects its keys above that bound in descending order in registers and offers each to the row
 * with the cascade above.
 *
 * Masking: classes >= n_cls of the ragged last tile and rows >= rows contribute nothing.
 * Limit: n_cls * round_up(dim, 16) * 4 < 2^32 per launch (32-bit DMA offsets); larger banks are the caller's chunks.  A chunk is
 * t_split advanced by whole rows; a chunk that does not end the bank starts at a multiple of eight rows.
 *
 * Extents: reads e_split rows [0, round_up(rows, 8)), t_split rows [0, round_up(n_cls, 8)), row_scale / row_bias [0, rows);
 * reads and writes key[0, rows * n_top) only.
 * Both operands are addressed with 32-bit byte offsets (hence the limit above, and round_up(rows, 8) * dim * 4 < 2^32:
 * WD_ERR_UNSUPPORTED), key with 64-bit ones; a class index is a 31-bit int.
 * WD_ERR_BAD_ARG: null pointers, non-positive sizes, n_top outside 1 .. 8, cls_offset < 0, cls_offset + n_cls > 2^31 - 1,
 * rows * n_top > 2^31 - 16, a misaligned key, bad seg arguments, only one of row_scale / row_bias, the row affine together with
 * seg_rows > 0.  WD_ERR_UNSUPPORTED: dim % 32, operands not 16-byte aligned, the limit above.
 * ------------------------------------------------------------------------------------------- */
int wd_topn_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls, int32_t dim,
                             int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale,
                             const float* seg_bias, const float* row_scale, const float* row_bias, uint32_t* range_flag,
                             int32_t cls_offset, int32_t n_top, uint64_t* key, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_topn_rows — merges the n_top best columns of block[r][0 .. n) into row r's keys, r < n_img * rows_per_img, class =
 * cls_offset + column.
 *   block       device fp32 [n_img * rows_per_img][ld], ld >= n_cls.  Without the row affine: scores >= +0 (sigmoid output).
 *               With it: raw logits; the entry applies sigmoid(logit * exp(row_scale[r]) + row_bias[r]) through the device
 *               function of the fused epilogue, so the bits agree with wd_topn_similarity_split over the same logits.
 *   count       device int32 [n_img] or NULL: image b's rows read columns < min(count[b], n_cls) (<= 0: none); NULL: n_cls
 *   row_scale, row_bias   device fp32 [n_img * rows_per_img] or both NULL
 * One wave per row, one pass over the row per slot.
 * Extents: reads only the columns named above, count[0, n_img), row_scale / row_bias [0, n_img * rows_per_img); reads and
 * writes key[0, n_img * rows_per_img * n_top) only.
 * WD_ERR_BAD_ARG: null block / key, non-positive sizes, ld < n_cls, n_top outside 1 .. 8, cls_offset as above, a misaligned key,
 * only one of row_scale / row_bias.
 * ------------------------------------------------------------------------------------------- */
int wd_topn_rows(const float* block, int32_t n_img, int32_t rows_per_img, int32_t n_cls, int32_t ld, int32_t cls_offset,
                 const int32_t* count, const float* row_scale, const float* row_bias, int32_t n_top, uint64_t* key, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_topn_unpack — scores_out[r] / labels_out[r] = slot `slot` of row r; an empty key gives (0.f, -1).  With slot = 0 these are
 * the arrays wd_best_unpack gives.
 * Extents: reads key[r * n_top + slot] for r < rows; writes scores_out[0, rows) and labels_out[0, rows).
 * WD_ERR_BAD_ARG: null pointers, rows <= 0, n_top outside 1 .. 8, slot outside [0, n_top).
 * ------------------------------------------------------------------------------------------- */
int wd_topn_unpack(const uint64_t* key, int64_t rows, int32_t n_top, int32_t slot, float* scores_out, int32_t* labels_out,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_topn_kept — the lists of the rows NMS kept: for b < batch, i < max_out, j < n_top
 *     (top_scores, top_labels)[b][i][j] = slot j of row b * n_anchor + out_anchors[b][i]
 * and (0.f, -1) where i >= out_count[b] (a count <= 0: the whole image) or the anchor is outside [0, n_anchor).
 *   key          device uint64 [batch * n_anchor][n_top]
 *   out_anchors  device int32 [batch][max_out], out_count device int32 [batch] (wd_nms_gather / wd_nms_gather_labeled)
 *   top_scores   device fp32 [batch][max_out][n_top], top_labels device int32 likewise: EVERY element is written
 * Extents: reads out_count[0, batch), out_anchors[b][0, min(out_count[b], max_out)), the keys of the anchors named there;
 * writes top_scores / top_labels [0, batch * max_out * n_top).
 * WD_ERR_BAD_ARG: null pointers, non-positive sizes, n_top outside 1 .. 8.
 * ------------------------------------------------------------------------------------------- */
int wd_topn_kept(const uint64_t* key, int32_t n_top, int32_t n_anchor, const int32_t* out_anchors, const int32_t* out_count,
                 int32_t max_out, int32_t batch, float* top_scores, int32_t* top_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_TOPN_H */
