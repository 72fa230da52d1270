/*
 * wedetect_hip_best.h — single-label ("best class") detection of libwedetect_hip.so (MI355X / gfx950 only): which ONE row of
 * a text bank fits each region best, without the [rows, n_cls] score tensor.  The reference's multi_label=False branch of
 * YOLOWorldHead.predict_by_feat (yolo_world_head.py:712-719: scores.max(1, keepdim=True), then filter_scores_and_topk with
 * results=dict(labels=labels[:, 0])), and mmcv.ops.batched_nms(..., class_agnostic=True) that usually goes with it.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_best_abi_version), like wedetect_hip_feed.h,
 * wedetect_hip_tile.h, wedetect_hip_views.h and wedetect_hip_fold.h: the entry points below are compiled into the same library
 * and follow the same conventions — plain C types, device pointers, a hipStream_t passed as void*, asynchronous on the
 * caller's stream, no allocation, no mutable global state, WD_OK or a negative WD_ERR_* code (wedetect_hip.h).
 *
 * Result definition (every path).  For region row r
 *     best_score[r] = max over c < K of score[r][c]
 *     best_label[r] = the LOWEST c that attains it            (Tensor.max(1) / numpy.argmax: first occurrence)
 * where score[r][c] is exactly the fp32 value the materialising similarity launch would have stored for the same operands:
 * the sigmoid is applied per element, never to a maximum of logits (distinct logits can round to one score, and the lowest
 * class among EQUAL SCORES is asked for).
 *
 * The key.  Row r owns one 64-bit word
 *     key[r] = (uint64) bits(score) << 32 | (0xFFFFFFFF - class)
 * Scores are >= +0, so the unsigned order of the bit patterns is the order of the floats; the inverted class makes the
 * lowest class the largest key among equal scores.  Every producer below merges into key[r] with an unsigned 64-bit atomic
 * maximum, which is order-independent: a bank may be cut into any launches in any order (cls_offset names a launch's first
 * class) and the result has the same bits.  key[r] == 0 means "no class seen"; the CALLER clears the keys (a memset on the
 * same stream) before the first producer of a step.
 *
 *   wd_best_similarity_split   fp16x3 region x text GEMM whose epilogue reduces to keys (no score tensor)
 *   wd_best_rows               the same merge from a materialised [rows][ld] score block
 *   wd_best_unpack             keys -> (score fp32, label int32)
 *   wd_nms_gather_labeled      wd_nms_gather for candidates whose flat index IS the anchor, labels read from an array;
 *                              adds WD_NMS_MMCV_AGNOSTIC
 */
#ifndef WEDETECT_HIP_BEST_H
#define WEDETECT_HIP_BEST_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on any change of a signature below. */
int wd_best_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * wd_best_similarity_split — operands exactly as wd_similarity_split (wedetect_hip.h): e_split = region rows [rows][dim] as
 * fp16 hi/lo groups in a buffer padded to a multiple of eight rows, t_split = text rows from wd_split_weights_padded,
 * unscale, the per-level affine (seg_rows / seg_end0 / seg_end1 / seg_scale[3] / seg_bias[3]; seg_rows = 0: scale 1, bias 0),
 * optional range_flag.  The sigmoid is always on.  In place of out / ldo:
 *
 *   cls_offset   class index of t_split's first row (0 for a whole bank; the caller's chunk start otherwise)
 *   key          device uint64 [rows], 8-byte aligned: merged into, see above
 *
 * Runs the 256 x 256 fp16x3 kernel of wd_similarity_split with another epilogue: the same K loop, the same per-element
 * expression, so score bits equal that entry point's output.  A lane holds one region row and 32 classes of a 32 x 32 MFMA
 * tile pair: 31 maxima in registers, one exchange with the other half-wave, one 64-bit vector atomic per (row, wave).
 * Per row 8 bytes of keys are touched instead of 4 * n_cls bytes of scores.
 *
 * Masking: classes >= n_cls of the ragged last tile and rows >= rows contribute nothing.
 * Non-finite: a non-finite accumulator (an fp16 half that overflowed) raises *range_flag and gives the row NaN score bits,
 * which beat every score — the unpacked score is non-finite and wd_topk_candidates reports the image (out_count = -1).
 * Limit: n_cls * round_up(dim, 16) * 4 < 2^32 per launch (32-bit DMA offsets); larger banks are the caller's chunks.
 * A chunk is t_split advanced by whole rows (round_up(dim, 16) * 4 bytes each); a chunk that does not end the bank starts at a
 * multiple of eight rows, so that the eight-row groups the kernel fetches stay inside the padded bank.
 *
 * Extents: reads e_split rows [0, round_up(rows, 8)), t_split rows [0, round_up(n_cls, 8)); writes key[0, rows) only.
 * Both operands are addressed with 32-bit byte offsets (hence the limit above, and round_up(rows, 8) * dim * 4 < 2^32:
 * WD_ERR_UNSUPPORTED), key with 64-bit ones; a class index is a 31-bit int.
 * WD_ERR_BAD_ARG: null pointers, non-positive sizes, cls_offset < 0, cls_offset + n_cls > 2^31 - 1, a misaligned key, bad seg
 * arguments.  WD_ERR_UNSUPPORTED: dim % 32, operands not 16-byte aligned, the limit above.
 * ------------------------------------------------------------------------------------------- */
int wd_best_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls, int32_t dim,
                             int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale,
                             const float* seg_bias, uint32_t* range_flag, int32_t cls_offset, uint64_t* key, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_best_rows — key[r] = max(key[r], best of scores[r][0 .. n)) for r < n_img * rows_per_img, class = cls_offset + column.
 *   scores   device fp32 [n_img * rows_per_img][ld], ld >= n_cls, values >= +0 (sigmoid output)
 *   count    device int32 [n_img] or NULL: image b's rows read columns < min(count[b], n_cls) (<= 0: none); NULL: n_cls
 * One wave per row.  Extents: reads only the columns named above; writes key[0, n_img * rows_per_img) only.
 * ------------------------------------------------------------------------------------------- */
int wd_best_rows(const float* scores, int32_t n_img, int32_t rows_per_img, int32_t n_cls, int32_t ld, int32_t cls_offset,
                 const int32_t* count, uint64_t* key, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_best_unpack — scores_out[r] = the score bits of key[r], labels_out[r] = 0xFFFFFFFF - low word; key[r] == 0 gives
 * (0.f, -1).  Extents: reads key[0, rows), writes scores_out[0, rows) and labels_out[0, rows).
 * ------------------------------------------------------------------------------------------- */
int wd_best_unpack(const uint64_t* key, int64_t rows, float* scores_out, int32_t* labels_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_nms_gather_labeled — wd_nms_gather (wedetect_hip.h: same candidates, metadata, outputs, workspace and extents — all
 * max_out rows of every output are written, 0 / -1 from out_count on) for candidates that wd_topk_candidates drew from ONE
 * score per anchor (n_per_image = n_anchor): a candidate's flat index IS its anchor and its label is
 * anchor_labels[b, anchor].
 *   anchor_labels   device int32 [batch, n_anchor]
 *   n_label         labels are in [0, n_label): replaces k where the kernel bounds the labels an offset box can meet
 * nms_mode: WD_NMS_VANILLA / WD_NMS_TORCHVISION / WD_NMS_MMCV as in wd_nms_gather, and
 *   WD_NMS_MMCV_AGNOSTIC   mmcv.ops.batched_nms(..., class_agnostic=True): the boxes are NOT offset; with n < mode_param
 *                          (split_thr) candidates one NMS across all labels, otherwise NMS per label on the same boxes.
 * ------------------------------------------------------------------------------------------- */
#define WD_NMS_MMCV_AGNOSTIC 3
int wd_nms_gather_labeled(const int32_t* cand_idx, const float* cand_score, const int32_t* cand_count, int32_t cand_stride,
                          const float* boxes, int32_t n_anchor, const int32_t* anchor_labels, int32_t n_label,
                          const float* meta, float iou_thr, int32_t max_out, int32_t nms_mode, int32_t mode_param,
                          const float* embed, int32_t embed_dim, float* out_boxes, float* out_scores, int32_t* out_labels,
                          int32_t* out_anchors, int32_t* out_count, float* out_embed, int32_t batch, void* workspace,
                          int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_BEST_H */
