/*
 * wedetect_hip_views.h — test-time augmentation of libwedetect_hip.so (MI355X / gfx950 only): flipped views of a batch made
 * on the device, and the rows of all views of every image merged into one list per image on the device.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_views_abi_version), like wedetect_hip_feed.h and
 * wedetect_hip_tile.h: the entry points below are compiled into the same library and follow the same conventions — plain C
 * types, device pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no mutable
 * global state, WD_OK or a negative WD_ERR_* code (wedetect_hip.h).
 *
 *   wd_flip_u8       [n, h, w, 3] uint8 images -> the same images flipped (mmcv imflip), one launch for the batch
 *   wd_views_merge   the stacked per-view rows of wd_nms_gather -> one list per image: boxes of flipped views mirrored back,
 *                    one mmcv-form batched NMS per image over the rows of all its views (mmdet DetTTAModel.merge_aug_bboxes +
 *                    batched_nms), every image of the batch in one launch sequence
 */
#ifndef WEDETECT_HIP_VIEWS_H
#define WEDETECT_HIP_VIEWS_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on any change of a signature below. */
int wd_views_abi_version(void);

#define WD_FLIP_NONE 0
#define WD_FLIP_HORIZONTAL 1    /* np.flip(img, axis=1) */
#define WD_FLIP_VERTICAL 2      /* np.flip(img, axis=0) */
#define WD_FLIP_DIAGONAL 3      /* both */

/* ---------------------------------------------------------------------------------------------
 * wd_flip_u8 — dst[i, y, x, c] = src[i, y', x', c] with x' = w - 1 - x when direction & 1, y' = h - 1 - y when
 * direction & 2 (mmcv imflip 'horizontal' / 'vertical' / 'diagonal').  The channels of a pixel keep their order.
 *
 *   src, dst         device [n, h, w, 3] uint8, dense; any address; the two ranges must not overlap
 *   direction        1 .. 3 (WD_FLIP_NONE is a copy the caller does not need: refused)
 *
 * One launch: image = blockIdx.y, each lane produces four consecutive pixels of a destination row.  When w % 4 == 0 and
 * both pointers are 4-byte aligned the four source pixels are three aligned dwords, their bytes are permuted in registers
 * and leave as three dword stores; otherwise the same lanes load and store bytes.
 *
 * Extents
 *   read      [src, src + n * h * w * 3), every byte once
 *   written   [dst, dst + n * h * w * 3), every byte once, nothing else
 *
 * WD_ERR_BAD_ARG: a null pointer, direction outside 1 .. 3, a non-positive size, n > 65535, overlapping src / dst ranges.
 * ------------------------------------------------------------------------------------------- */
int wd_flip_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, int32_t direction, void* stream);

/* Bytes of wd_views_merge's workspace (0 for arguments the entry point refuses). */
int64_t wd_views_merge_workspace_bytes(int32_t n_view, int32_t batch, int32_t max_in);

/* ---------------------------------------------------------------------------------------------
 * wd_views_merge — the rows the per-view steps kept (wd_nms_gather's out_boxes / out_scores / out_labels / out_count with
 * pre_nms_rescale != 0: original-image pixels, clamped; stacked view by view) -> the rows of every image.
 *
 *   boxes [n_view, batch, max_in, 4] fp32 (16-byte aligned), scores [n_view, batch, max_in] fp32, labels
 *   [n_view, batch, max_in] int32, counts [n_view, batch] int32
 *   view_flip [n_view] int32, DEVICE array: the WD_FLIP_* code of each view (only bits 0 and 1 are read)
 *   img_wh [batch, 2] fp32: (width, height) of the original image (mmdet's ori_shape, reversed)
 *   A row's slot within its image is  view * max_in + row.
 *
 *   which rows     only rows < counts[v, b] are read; what lies beyond may hold anything.  Rows whose label is outside
 *                  [0, n_cls) are skipped.  Scores are positive and finite (what wd_nms_gather writes).
 *   un-flip        mmdet bbox_flip with img_shape = ori_shape, one fp32 subtraction per coordinate, W = img_wh[b, 0],
 *                  H = img_wh[b, 1]:   bit 0: x1' = W - x2, x2' = W - x1     bit 1: y1' = H - y2, y2' = H - y1
 *   order          survivors by (score descending, slot ascending)
 *   NMS            mmcv.ops.batched_nms on them (WD_NMS_MMCV of wd_nms_gather: fp32 coordinate offsets
 *                  label * (max coordinate + 1), the max taken per image over its surviving rows; one class-agnostic pass
 *                  below split_thr survivors, per class from split_thr), `ovr > iou_thr`, stopped at max_out rows
 *   out_boxes [batch, max_out, 4] (16-byte aligned; the un-flipped boxes, clamped to [0, W] x [0, H] — a no-op for rows of
 *   wd_nms_gather), out_scores [batch, max_out], out_labels [batch, max_out], out_src [batch, max_out] (the slot a row came
 *   from), out_count [batch].  All max_out rows of every output are written: 0 / -1 from the count on.
 *   guard          out_count[b] = -1 (and no rows: all 0 / -1) for an image where any view has counts[v, b] < 0, the
 *                  per-view step's report of non-finite scores.  The other images of the batch are not affected.
 *
 * Launches, the same whatever the batch: one kernel with one workgroup per image (filter + un-flip + 64-bit keys, their
 * bitonic sort in LDS with the passes of csrc/bitonic.h, the candidate list), wd_nms_gather on `batch` "images" of
 * n_view * max_in anchors with identity metadata, one kernel for the guard.
 *
 * workspace: wd_views_merge_workspace_bytes(n_view, batch, max_in) bytes, 256-byte aligned, no initialisation needed.
 *
 * WD_ERR_UNSUPPORTED (before any launch): n_view outside 1 .. 8, n_view * max_in > 4096, max_out > 1024,
 * n_view * max_in * n_cls >= 2^31.
 * WD_ERR_BAD_ARG: null pointers, non-positive sizes, batch > 65535, misaligned boxes / out_boxes / workspace, iou_thr not
 * finite.  WD_ERR_WORKSPACE: workspace_bytes too small.
 * ------------------------------------------------------------------------------------------- */
int wd_views_merge(const float* boxes, const float* scores, const int32_t* labels, const int32_t* counts,
                   const int32_t* view_flip, const float* img_wh, int32_t n_view, int32_t batch, int32_t max_in,
                   int32_t n_cls, float iou_thr, int32_t split_thr, int32_t max_out, float* out_boxes, float* out_scores,
                   int32_t* out_labels, int32_t* out_src, int32_t* out_count, void* workspace, int64_t workspace_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_VIEWS_H */
