/*
 * wedetect_hip_sparse.h — "sparse scores": the multi-label detection step of libwedetect_hip.so (MI355X / gfx950 only) without
 * the [rows, n_cls] score tensor.  The reference's default branch of YOLOWorldHead.predict_by_feat (multi_label=True:
 * filter_scores_and_topk(scores, score_thr, nms_pre) over every (anchor, class) pair) only ever looks at the pairs with
 * score > score_thr and keeps at most nms_pre of them per image: the similarity launch appends exactly those pairs to a
 * per-image list, and a sort of that list gives what wd_topk_candidates gives.  Where an image's list does not overflow the result
 * is the dense step's result bit for bit.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_sparse_abi_version), like wedetect_hip_best.h: the entry
 * points below are compiled into the same library and follow the same conventions — plain C types, device pointers, a
 * hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no mutable global state, WD_OK or a negative
 * WD_ERR_* code (wedetect_hip.h).
 *
 * Data (owned by the caller).
 *   list    device uint64 [batch][list_cap], 8-byte aligned.  Needs no initialisation.
 *   state   device int32 [batch][2] = {candidates seen, non-finite seen}.  The CALLER zeroes it (one memset on the launch's
 *           stream) before the first producer of a step.
 *   key     (uint64)(~bits(score)) << 32 | flat,   flat = anchor * n_cls_total + cls_offset + class,
 *           anchor = row % rows_per_img of image row / rows_per_img.  It is the key wd_topk_candidates sorts by: ascending key =
 *           score descending, then flat index ascending.  Keys of one image are unique.
 *   list_cap   a power of two in [wd_topk_capacity(nms_pre), 2^20].
 * Every candidate (a valid element with score > thr, strict fp32 comparison as in filter_scores_and_topk) takes a slot
 * s = atomicAdd(&state[b][0], ...) and its key is stored at list[b][s] iff s < list_cap.  The counter keeps counting past the cap:
 * state[b][0] > list_cap means the list is incomplete (overflow).  The SET of keys of an image does not depend on how a bank is
 * cut into launches or on the order of tiles; the positions inside the list do.
 * rows_per_img * n_cls_total >= 2^31 is refused (WD_ERR_UNSUPPORTED): candidate indices are int32, as in the dense path.
 *
 *   wd_sparse_similarity_split   fp16x3 region x text GEMM whose epilogue appends candidates (no score tensor)
 *   wd_sparse_rows               the same append from a materialised [rows][ld] score block
 *   wd_sparse_select             per-image sort of the list -> the buffers wd_nms_gather reads, plus a status
 */
#ifndef WEDETECT_HIP_SPARSE_H
#define WEDETECT_HIP_SPARSE_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on any change of a signature below. */
int wd_sparse_abi_version(void);

#define WD_SPARSE_OK 0          /* status of wd_sparse_select: the image's candidates are complete */
#define WD_SPARSE_OVERFLOW 1    /* more candidates than list_cap: the list is incomplete and was not used */
#define WD_SPARSE_NONFINITE 2   /* a non-finite score / accumulator was seen (the dense path's out_count = -1) */

/* ---------------------------------------------------------------------------------------------
 * wd_sparse_similarity_split — operands exactly as wd_best_similarity_split (wedetect_hip_best.h): e_split, rows, t_split,
 * unscale, n_cls, dim, the seg_* arguments, range_flag, cls_offset (class index of t_split's first row).  rows =
 * n_img * rows_per_img region rows of whole images back to back.  In addition:
 *
 *   rows_per_img   region rows (anchors) of one image; rows % rows_per_img == 0
 *   n_cls_total    classes of the whole bank (the row pitch of the flat index); cls_offset + n_cls <= n_cls_total
 *   thr            score threshold; candidates have score > thr
 *   list, list_cap, state   see above; batch = rows / rows_per_img
 *
 * Runs the 256 x 256 fp16x3 kernel of wd_similarity_split with another epilogue: the same K loop and the same per-element
 * expression (fmaf(acc, unscale, 0), fmaf(x, oscale, obias), the fast sigmoid), so score bits equal that entry point's output.
 * A 32-row group of a wave that lies inside one image takes its slots with ONE vector atomic per (wave, group): the lanes'
 * candidate counts become offsets through a wave prefix sum.  A group that straddles two images issues one atomic per lane
 * that has candidates.  Keys are written with plain vector stores.
 *
 * Masking: classes >= n_cls of the ragged last tile and rows >= rows contribute nothing.
 * Non-finite: a non-finite accumulator (an fp16 half that overflowed) raises *range_flag and sets state[b][1] of the row's image.
 * Limit: n_cls * round_up(dim, 16) * 4 < 2^32 per launch; larger banks are the caller's chunks (t_split advanced by whole rows;
 * a chunk that does not end the bank starts at a multiple of eight rows).  Chunks may be issued in any order.
 *
 * Extents: reads e_split rows [0, round_up(rows, 8)), t_split rows [0, round_up(n_cls, 8)); reads and writes state[0, 2 * batch);
 * writes list[b][s] for s < min(state[b][0], list_cap) only.
 * Both operands are addressed with 32-bit byte offsets (hence the limit above, and round_up(rows, 8) * dim * 4 < 2^32:
 * WD_ERR_UNSUPPORTED); the flat index anchor * n_cls_total + class of a candidate is a 31-bit int (the limit below).
 * WD_ERR_BAD_ARG: null pointers, non-positive sizes, rows % rows_per_img, cls_offset < 0, cls_offset + n_cls > n_cls_total, a
 * misaligned list (8 bytes) or state (4 bytes), a list_cap that is not a power of two or lies outside [1, 2^20], bad seg
 * arguments.  WD_ERR_UNSUPPORTED: rows_per_img * n_cls_total >= 2^31, dim % 32, operands not 16-byte aligned, the limit above.
 * ------------------------------------------------------------------------------------------- */
int wd_sparse_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls, int32_t dim,
                               int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale,
                               const float* seg_bias, uint32_t* range_flag, int32_t cls_offset, int32_t rows_per_img,
                               int32_t n_cls_total, float thr, uint64_t* list, int32_t list_cap, int32_t* state, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_sparse_rows — the same append from a materialised block: arguments as wd_best_rows (wedetect_hip_best.h).
 *   scores   device fp32 [n_img * rows_per_img][ld], ld >= n_cls; column c is class cls_offset + c
 *   count    device int32 [n_img] or NULL: image b's rows read columns < min(count[b], n_cls) (<= 0: none); NULL: n_cls
 * One wave per row; one atomic per (wave, 64 columns) that holds a candidate.  A non-finite score (exponent bits all ones) sets
 * state[b][1].
 * Extents: reads only the columns named above; reads and writes state[0, 2 * n_img); writes list[b][s] for
 * s < min(state[b][0], list_cap) only.  Errors as above (ld < n_cls: WD_ERR_BAD_ARG).
 * ------------------------------------------------------------------------------------------- */
int wd_sparse_rows(const float* scores, int32_t n_img, int32_t rows_per_img, int32_t n_cls, int32_t ld, int32_t cls_offset,
                   const int32_t* count, int32_t n_cls_total, float thr, uint64_t* list, int32_t list_cap, int32_t* state,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_sparse_select — for each image b, with n = state[b][0], writes what wd_topk_candidates writes for the same scores, thr and
 * nms_pre: out_idx int32 [batch][cap], out_score fp32 [batch][cap], out_count int32 [batch], cap = wd_topk_capacity(nms_pre); all
 * cap entries of both rows are written, -1 / 0.f from max(out_count, 0) on.  Also status int32 [batch]:
 *
 *   state[b][1] != 0   out_count = -1 (as the dense kernel reports a non-finite row), no entries; status = WD_SPARSE_NONFINITE
 *   n > list_cap       out_count = 0, no entries; status = WD_SPARSE_OVERFLOW
 *   otherwise          the n keys sorted ascending (the network of csrc/bitonic.h: 8192-key chunks in LDS, wider strides in
 *                      global memory), the first min(n, nms_pre) unpacked to (flat index, score); status = WD_SPARSE_OK
 *
 * The list is sorted IN PLACE (no workspace): list[b][n .. n2), n2 = the next power of two >= n, is filled with ~0 first.  The
 * launches are sized for list_cap; workgroups past n2 leave at once, so the work follows n without a host read.  state is only
 * read.  list_cap >= wd_topk_capacity(nms_pre) is required.
 *
 * Extents: reads state[0, 2 * batch); reads and writes list[b][0, n2) of images with status 0; writes out_idx / out_score
 * [0, batch * cap), out_count / status [0, batch).
 * WD_ERR_BAD_ARG: null pointers, batch outside [1, 65535], nms_pre outside [1, 2^20], a bad list_cap (see above; also
 * list_cap < cap), a misaligned list.
 * ------------------------------------------------------------------------------------------- */
int wd_sparse_select(uint64_t* list, int32_t list_cap, const int32_t* state, int32_t batch, int32_t nms_pre, int32_t* out_idx,
                     float* out_score, int32_t* out_count, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_SPARSE_H */
