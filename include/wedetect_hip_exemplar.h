/*
 * wedetect_hip_exemplar.h — exemplar prompts of libwedetect_hip.so (MI355X / gfx950 only): class-bank rows made from example
 * boxes instead of text.  "Find more things like the one in this box": an example box is assigned the few anchors of the head
 * whose decoded boxes overlap it best, their post-BN region embeddings are pooled into one unit row per class, and that row is
 * used exactly like a row of a text bank (alone, concatenated with text rows, or in a per-image bank).
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_exemplar_abi_version), like wedetect_hip_topn.h and the
 * other add-on headers: the entry points below are compiled into the same library and follow the same conventions — plain C
 * types, device pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no workspace, no
 * atomics, no mutable global state, WD_OK or a negative WD_ERR_* code (wedetect_hip.h).  Every refusal below happens before any
 * launch.
 *
 * Result definition (every path; tests/exemplar_ref.py restates it in numpy).
 *
 * Inputs per image b of a batch: ex_count[b] example boxes ex_boxes[b][e] = (x1, y1, x2, y2) in ORIGINAL-IMAGE pixels, and the
 * image's 8-float metadata row of wd_nms_gather: pad_x, pad_y, -, scale_x, scale_y, ori_w, ori_h, -.  Parameters: m = anchors
 * per example (1 .. WD_EXEMPLAR_MAX_M), min_iou >= 0.
 *
 * To network pixels.  x' = x * scale_x + pad_x, y' = y * scale_y + pad_y: one fp32 multiply, then one fp32 add, per coordinate,
 * never fused — the inverse of the (box - pad) / scale of wd_nms_gather.
 *
 * Assignment.  For every anchor n of the image, iou[n] is the fp32 IoU of the example box E (network pixels) with boxes[b][n],
 * the decoded head boxes, every operation individually rounded, in this order (the order of the NMS kernels):
 *     area_e = (E.x2 - E.x1) * (E.y2 - E.y1);   area_n likewise
 *     w = max(0, min(E.x2, N.x2) - max(E.x1, N.x1));   h likewise
 *     inter = w * h
 *     iou = inter / (area_e + area_n - inter)            (the correctly rounded division)
 * Candidates are the anchors with iou[n] > min_iou; a NaN (a degenerate box) is not a candidate.  The example's list is the first
 * m candidates by (IoU DESCENDING, ANCHOR ASCENDING).  Slot e * m + j of sel_anchors[b] holds the anchor of rank j and the same
 * slot of sel_iou[b] its IoU; the slot is (-1, 0.0f) where fewer than m candidates exist and for e >= ex_count[b].
 * sel_count[b] = min(max(ex_count[b], 0), max_ex) * m.  Every element of the three outputs is written.
 *
 * Key form, as in the best-class and top-n headers: (uint64) bits(iou) << 32 | (0xFFFFFFFF - anchor); larger is better, 0 means
 * empty (a candidate's IoU is > 0, so its key is not 0).
 *
 * Embeddings.  The post-BN region embedding of a selected anchor is the row the level's embedding GEMM gives for the anchor's c2
 * row: present sel_anchors / sel_count to wd_kept_rows_gather (wedetect_hip_fold.h) with max_out = S = max_ex * m — it zero-fills
 * the rows whose anchor is out of range, so -1 is safe — and run each level's embedding GEMM on gathered[l].  That leaves
 * level_embed [3][batch * S][dim], the layout wd_kept_rows_select reads; [batch, anchors, dim] is never materialised.
 *
 * Prototype of class c.  The caller groups example slots into classes with a CSR pair: cls_off[n_cls + 1] and cls_slot[T], flat
 * slot indices b * S + e * m + j in the order the caller lists them.  For each listed slot with an anchor >= 0, in list order:
 *     r = its embedding row (level_embed[level of the anchor][slot]);   inv = 1 / sqrt(sum_d r[d]^2)
 *     acc[d] += iou * (r[d] * inv)                       (two multiplies and one add, never fused)
 * Each row is L2-normalised first because BN outputs have widely different norms.  Then bank[c] = acc / ||acc|| and support[c] =
 * the number of slots that contributed.  support[c] == 0, or a norm that is zero or not finite, gives an all-zero row: the caller
 * refuses such a class.  A listed slot outside [0, n_slot) contributes nothing.
 * The summation over slots is sequential in list order; the reduction tree of the two norms is fixed by the kernel and depends on
 * nothing but dim: the same inputs give the same bits on every run, at every class index and for every n_cls.
 *
 *   wd_exemplar_assign   example boxes -> the m best anchors of each (no atomics, no workspace)
 *   wd_exemplar_pool     selected anchors' embeddings -> one unit row per class
 */
#ifndef WEDETECT_HIP_EXEMPLAR_H
#define WEDETECT_HIP_EXEMPLAR_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_EXEMPLAR_MAX_M 8
#define WD_EXEMPLAR_MAX_EX 64

/* Bumped on any change of a signature below. */
int wd_exemplar_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * wd_exemplar_assign — the assignment above for batch images of max_ex example slots each.
 *
 *   boxes        device fp32 [batch][n_anchor][4], 16-byte aligned: the decoded head boxes in network pixels (wd_dfl_decode)
 *   ex_boxes     device fp32 [batch][max_ex][4], 4-byte aligned, original-image pixels; rows e >= ex_count[b] are not read
 *   ex_count     device int32 [batch]; a value below 0 counts as 0, one above max_ex as max_ex
 *   meta         device fp32 [batch][8], the rows of wd_nms_gather
 *   max_ex       1 .. WD_EXEMPLAR_MAX_EX;   m   1 .. WD_EXEMPLAR_MAX_M;   min_iou   finite, >= 0
 *   sel_anchors  device int32 [batch][max_ex * m];   sel_iou   device fp32 likewise;   sel_count   device int32 [batch]
 *
 * One workgroup of 256 lanes per (example, image).  A lane walks the anchors tid, tid + 256, ... with 16-byte box loads and keeps
 * its m best keys sorted in registers; each wave then pops its m largest keys with m rounds of a 64-lane maximum (the owner of a
 * round's maximum drops its head), the four wave leaders leave them in LDS, and wave 0 merges those <= 32 keys the same way and
 * stores the m slots.
 *
 * Extents: reads boxes[b][0, n_anchor) of the images with ex_count[b] > 0, ex_boxes[b][0, min(ex_count[b], max_ex)),
 * ex_count[0, batch), meta[b][0, 8); writes sel_anchors / sel_iou [0, batch * max_ex * m) and sel_count[0, batch) only, whole.
 * WD_ERR_BAD_ARG: null pointers, non-positive n_anchor / batch, max_ex outside 1 .. 64, m outside 1 .. 8, min_iou negative or
 * not finite, boxes not 16-byte aligned, another pointer not 4-byte aligned, batch > 65535, batch * n_anchor > 2^31 - 16.
 * ------------------------------------------------------------------------------------------- */
int wd_exemplar_assign(const float* boxes, int32_t n_anchor, const float* ex_boxes, const int32_t* ex_count, const float* meta,
                       int32_t max_ex, int32_t batch, int32_t m, float min_iou, int32_t* sel_anchors, float* sel_iou,
                       int32_t* sel_count, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_exemplar_pool — the prototypes above for n_cls classes.
 *
 *   level_embed  device fp32 [3][n_slot][dim], 16-byte aligned: the three embedding GEMMs' outputs (n_slot = batch * max_ex * m)
 *   dim          % 4 == 0, 4 .. 1024
 *   off1, off2   first anchor of head level 1 and of level 2 (0 < off1 < off2): an anchor a is of level (a >= off1) + (a >= off2)
 *   sel_anchors  device int32 [n_slot];   sel_iou   device fp32 [n_slot]   (wd_exemplar_assign)
 *   cls_off      device int32 [n_cls + 1], ascending from 0;   cls_slot   device int32 [cls_off[n_cls]] (may be NULL when every
 *                class is empty and nothing is listed)
 *   bank         device fp32 [n_cls][dim], 16-byte aligned;   support   device int32 [n_cls]
 *
 * One workgroup of 256 lanes per class; a lane owns 4 consecutive floats of the row (dim = 768: 192 active lanes).
 *
 * Extents: reads cls_off[0, n_cls + 1), cls_slot[cls_off[c], cls_off[c + 1]), sel_anchors / sel_iou at the listed slots, and
 * level_embed[l][s][0, dim) for the listed slots s with an anchor >= 0; writes bank[0, n_cls * dim) and support[0, n_cls) only,
 * whole.
 * WD_ERR_BAD_ARG: null pointers (cls_slot excepted), non-positive n_slot / n_cls, dim outside 4 .. 1024, dim % 4,
 * not 0 < off1 < off2, level_embed or bank not 16-byte aligned, another pointer not 4-byte aligned,
 * 3 * n_slot * dim > 2^31 - 16.
 * ------------------------------------------------------------------------------------------- */
int wd_exemplar_pool(const float* level_embed, int32_t dim, int32_t off1, int32_t off2, const int32_t* sel_anchors,
                     const float* sel_iou, int32_t n_slot, const int32_t* cls_off, const int32_t* cls_slot, int32_t n_cls,
                     float* bank, int32_t* support, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_EXEMPLAR_H */
