/*
 * wedetect_hip_groups.h — prompt groups of libwedetect_hip.so (MI355X / gfx950 only): a class with several names (synonyms) is
 * scored as the BEST of them.  The bank holds one row per prompt; the result is a score tensor [rows][n_groups] with one column
 * per class, so everything downstream of the score tensor (wd_topk_candidates, wd_nms_gather) runs unchanged.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_groups_abi_version), like wedetect_hip_best.h and the other
 * add-on headers: the entry points below are compiled into the same library and follow the same conventions — plain C types,
 * device pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no mutable global state,
 * WD_OK or a negative WD_ERR_* code (wedetect_hip.h).
 *
 * The packing (wedetect_amd/groups.py: PromptGroups).  The K_pad bank rows are cut into BINS of WD_GROUP_BIN = 32 consecutive
 * rows, K_pad % 32 == 0, and NO CLASS STRADDLES A BIN: the rows of class g are consecutive and lie inside one bin.  A bin that
 * its classes do not fill is padded by repeating the last row of its last class — a duplicate scores what its original scores, so
 * the maximum of the class is unchanged: no sentinel rows, no masks.  Two device tables describe the layout:
 *     group_of   int32 [K_pad]            the class of every bank row, non-decreasing
 *     bin_first  int32 [K_pad / 32 + 1]   the classes of bin s are [bin_first[s], bin_first[s + 1]), at most 32 of them
 * Every output element belongs to exactly one bin, so it is written exactly once by a plain vector store: no atomics, and
 * the output needs no clearing.
 *
 * Result definition (both entries).  For region row r and class g of a bin the launch covers:
 *     out[r][g] = max over bank rows c with group_of[c] == g of score[r][c]
 * where score[r][c] is exactly the fp32 value the materialising similarity launch (wd_similarity_split with sigmoid) would have
 * stored for the same operands: the sigmoid is applied per ELEMENT and the maximum taken over scores, so the bits are those of
 * a maximum over the materialised tensor.
 *
 *   wd_group_similarity_split   fp16x3 region x text GEMM whose epilogue stores the class maxima (no [rows][K_pad] tensor)
 *   wd_group_rows               the same maxima from a materialised [rows][ld] block of scores
 */
#ifndef WEDETECT_HIP_GROUPS_H
#define WEDETECT_HIP_GROUPS_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_GROUP_BIN 32

/* Bumped on any change of a signature below. */
int wd_groups_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * wd_group_similarity_split — operands as wd_best_similarity_split (wedetect_hip_best.h): e_split, rows, t_split, unscale, n_cls,
 * dim, the per-level affine seg_* (seg_rows = 0: none), optional range_flag; the sigmoid is always applied.  In addition:
 *
 *   group_of, bin_first   the WHOLE tables of the bank (above), device int32, 4-byte aligned; indexed by absolute bank row / bin
 *   cls_offset            the bank row t_split's first row stands for; a multiple of 32.  n_cls is a multiple of 32 too: a
 *                         launch covers whole bins
 *   out                   device fp32, row stride ldo >= n_groups, 4-byte aligned.  Written at columns
 *                         [bin_first[cls_offset / 32], bin_first[(cls_offset + n_cls) / 32)) of rows [0, rows)
 *   n_groups              classes of the whole bank (columns of out); an entry of a table that points past it is not stored
 *
 * Runs the 256 x 256 fp16x3 kernel of wd_similarity_split with another epilogue: the same K loop, the same per-element
 * expression.  A wave stages the scores of 32 rows x one bin in its LDS patch; lanes then take (row, class of the bin) pairs,
 * read the class's columns from the patch and store the maximum: consecutive lanes write consecutive classes of a row.
 *
 * Non-finite: an inf / NaN accumulator of (row, bin) raises *range_flag and stores NaN to that row's classes of the bin (so
 * wd_topk_candidates reports the image).
 * Masking: rows >= rows and the bins of the ragged last 256-column tile past n_cls contribute nothing and are not stored.
 * Limit: n_cls * round_up(dim, 16) * 4 < 2^32 per launch (32-bit DMA offsets); larger banks are the caller's chunks, any multiple
 * of 32 rows each.  Disjoint chunks write disjoint columns: a bank cut into launches gives the bits of one launch.
 *
 * Extents: reads e_split rows [0, round_up(rows, 8)), t_split rows [0, n_cls), group_of[cls_offset, cls_offset + n_cls),
 * bin_first[cls_offset / 32, (cls_offset + n_cls) / 32]; writes out[r][g] for r < rows and g in the column range above only
 * (every such element, exactly once; nothing between n_groups and ldo).
 * Both operands are addressed with 32-bit byte offsets (hence the limit above, and round_up(rows, 8) * dim * 4 < 2^32:
 * WD_ERR_UNSUPPORTED), out with 64-bit ones (rows * ldo may pass 2^32 bytes); a class index is a 31-bit int.
 * WD_ERR_BAD_ARG: null pointers (the tables included), non-positive sizes, cls_offset < 0 or cls_offset % 32, n_cls % 32,
 * cls_offset + n_cls > 2^31 - 1, n_groups <= 0, ldo < n_groups, out / group_of / bin_first not 4-byte aligned, bad seg arguments.
 * WD_ERR_UNSUPPORTED: dim % 32, operands not 16-byte aligned, the limit above.
 * ------------------------------------------------------------------------------------------- */
int wd_group_similarity_split(const void* e_split, int64_t rows, const void* t_split, float unscale, int32_t n_cls, int32_t dim,
                              int32_t seg_rows, int32_t seg_end0, int32_t seg_end1, const float* seg_scale, const float* seg_bias,
                              uint32_t* range_flag, const int32_t* group_of, const int32_t* bin_first, int32_t cls_offset,
                              float* out, int32_t ldo, int32_t n_groups, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_group_rows — the same maxima from a materialised block: block[r][0 .. n_cls) holds the scores of region row r against bank
 * rows [cls_offset, cls_offset + n_cls), both multiples of 32 (whole bins).  For banks below 256 rows, fp32 towers and the
 * caller's chunks of at most a few thousand columns.  The maximum is taken over the stored values, so the bits are those of
 * wd_group_similarity_split where the block is wd_similarity_split's output; a NaN in a class's columns gives NaN.
 *   block       device fp32 [rows][ld], ld >= n_cls
 *   group_of, bin_first, out, ldo, n_groups   as above
 * One workgroup per (8 rows, bin): a (row, class of the bin) pair per lane, consecutive lanes store consecutive classes.
 * Extents: reads block[r][0, n_cls) for r < rows, group_of[cls_offset, cls_offset + n_cls), bin_first[cls_offset / 32,
 * (cls_offset + n_cls) / 32]; writes out[r][g] for r < rows and g in [bin_first[cls_offset / 32], bin_first[(cls_offset + n_cls) /
 * 32)) only, every such element exactly once.
 * WD_ERR_BAD_ARG: null pointers, non-positive sizes, rows > 2^31 - 16, ld < n_cls, cls_offset < 0 or cls_offset % 32, n_cls % 32,
 * cls_offset + n_cls > 2^31 - 1, n_cls / 32 > 65535, n_groups <= 0, ldo < n_groups, a pointer not 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int wd_group_rows(const float* block, int64_t rows, int32_t n_cls, int32_t ld, const int32_t* group_of, const int32_t* bin_first,
                  int32_t cls_offset, float* out, int32_t ldo, int32_t n_groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_GROUPS_H */
