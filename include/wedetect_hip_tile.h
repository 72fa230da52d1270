/*
 * wedetect_hip_tile.h — tiled inference of libwedetect_hip.so (MI355X / gfx950 only): one large image as a batch of
 * overlapping network-sized tiles, merged on the device.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_tile_abi_version), like wedetect_hip_feed.h: the
 * entry points below are compiled into the same library and follow the same conventions — plain C types, device
 * pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no mutable global state,
 * WD_OK or a negative WD_ERR_* code (wedetect_hip.h).
 *
 *   wd_tile_cut_u8   the image (uploaded once) -> [n_tile, th, tw, 3] uint8 tiles, the layout the image tower reads
 *   wd_tile_merge    the stacked per-tile rows of wd_nms_gather -> one list for the image: rows cut by an interior tile
 *                    side dropped, boxes translated to image pixels, one mmcv-form batched NMS over all tiles
 */
#ifndef WEDETECT_HIP_TILE_H
#define WEDETECT_HIP_TILE_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on any change of WdTile or of a signature below. */
int wd_tile_abi_version(void);

#define WD_TILE_CROP 0          /* a window of the image, pixels copied as they are */
#define WD_TILE_OVERVIEW 1      /* the whole image resampled by the caller; its rows arrive in image pixels */
#define WD_TILE_BLANK 2         /* batch padding: all fill, its rows are never read */

/* ---------------------------------------------------------------------------------------------
 * WdTile — one tile of a plan (32 bytes).
 *
 *   x0, y0           image pixel of the tile's pixel (0, 0) (crops; 0 otherwise)
 *   w, h             valid size: the tile shows image pixels [x0, x0 + w) x [y0, y0 + h), w <= tw, h <= th; the rest
 *                    of the tile is fill (an image smaller than a tile along that axis)
 *   interior_mask    bit 0 = left, 1 = top, 2 = right, 3 = bottom: set when that side of the valid window is not a
 *                    side of the image (x0 > 0, y0 > 0, x0 + w < img_w, y0 + h < img_h)
 *   kind             WD_TILE_CROP / WD_TILE_OVERVIEW / WD_TILE_BLANK
 *   img_w, img_h     size of the image the plan was made for (the same in every tile of a plan)
 * ------------------------------------------------------------------------------------------- */
typedef struct WdTile {
  int32_t x0, y0, w, h;
  int32_t interior_mask, kind;
  int32_t img_w, img_h;
} WdTile;

/* sizeof(WdTile) as the library was compiled (binding self-check). */
int32_t wd_tile_sizeof_tile(void);

/* ---------------------------------------------------------------------------------------------
 * wd_tile_cut_u8 — dst[t, y, x, c] = img[y0 + y, x0 + x, c'] inside the valid w x h of a CROP tile, `fill` elsewhere in
 * it; BLANK tiles are all `fill`; the bytes of OVERVIEW tiles are NOT touched (the caller fills that slot through
 * wd_cv_resize_paste_u8 / wd_feed_batch_u8).  c' = 2 - c when swap_rb != 0, else c.
 *
 *   img                  device uint8 HWC image, 3 channels, h rows of w pixels, rows row_pitch_bytes apart
 *                        (row_pitch_bytes >= w * 3); any address, any pitch
 *   tiles                DEVICE array of n_tile descriptors
 *   tiles_host           the same descriptors in host memory: read during the call (argument checks; nothing is read
 *                        back from the device), not needed afterwards
 *   th, tw               tile size;  fill: 0 .. 255, written to all three channels
 *   dst                  device [n_tile, th, tw, 3] uint8, dense; any address
 *
 * One launch: tile = blockIdx.y (its descriptor is read through uniform loads), each lane produces four pixels of a
 * tile row and stores them as three dwords when tw % 4 == 0 and dst is 4-byte aligned; otherwise the same lanes store
 * bytes.
 *
 * Extents
 *   read      of img only [y * row_pitch_bytes, y * row_pitch_bytes + w * 3) of the rows a crop shows — dword loads are
 *             used only where all four lie inside [img, img + h * row_pitch_bytes), so no load leaves that range and no
 *             result depends on the bytes between two rows; the n_tile device descriptors
 *   written   all th * tw * 3 bytes of every CROP and BLANK tile, nothing else
 *
 * WD_ERR_BAD_ARG: a null pointer, n_tile outside 1 .. 65535, a crop whose window leaves the image or the tile or is
 * empty, an unknown kind, fill outside 0 .. 255, row_pitch_bytes < w * 3.
 * ------------------------------------------------------------------------------------------- */
int wd_tile_cut_u8(const uint8_t* img, int32_t h, int32_t w, int64_t row_pitch_bytes, const WdTile* tiles,
                   const WdTile* tiles_host, int32_t n_tile, int32_t th, int32_t tw, int32_t fill, int32_t swap_rb,
                   uint8_t* dst, void* stream);

/* Bytes of wd_tile_merge's workspace (0 for arguments the entry point refuses). */
int64_t wd_tile_merge_workspace_bytes(int32_t n_tile, int32_t max_in);

/* ---------------------------------------------------------------------------------------------
 * wd_tile_merge — the rows the per-tile steps kept (wd_nms_gather's out_boxes / out_scores / out_labels / out_count,
 * stacked tile by tile) -> the rows of the image.
 *
 *   boxes [n_tile, max_in, 4] fp32 (16-byte aligned), scores [n_tile, max_in] fp32, labels [n_tile, max_in] int32,
 *   counts [n_tile] int32, tiles: the n_tile DEVICE descriptors.  A row's slot is  tile * max_in + row.
 *
 *   which rows     only rows < counts[t] of non-BLANK tiles are read; what lies beyond may hold anything.  Rows whose
 *                  label is outside [0, n_cls) are skipped.  Scores are positive and finite, coordinates >= 0 (what
 *                  wd_nms_gather writes).
 *   border drop    CROP tiles, edge_margin m > 0: with the tile-local box (x1, y1, x2, y2) and the valid size as
 *                  floats (w, h) a row is dropped iff
 *                    (mask & 1 && x1 < m) || (mask & 2 && y1 < m) || (mask & 4 && x2 > w - m) || (mask & 8 && y2 > h - m)
 *                  (fp32): an object cut by an interior tile side lies whole in a neighbouring tile or in the overview
 *   translate      CROP rows: + (x0, y0) as fp32 adds; OVERVIEW rows are in image pixels already
 *   order          survivors by (score descending, slot ascending)
 *   NMS            mmcv.ops.batched_nms on them (WD_NMS_MMCV of wd_nms_gather: fp32 coordinate offsets
 *                  label * (max coordinate + 1), one class-agnostic pass below split_thr survivors, per class from
 *                  split_thr), `ovr > iou_thr`, stopped at max_out rows
 *   out_boxes [max_out, 4] (16-byte aligned; the un-offset boxes, clamped to [0, img_w] x [0, img_h] of descriptor 0 —
 *   a no-op for rows of wd_nms_gather), out_scores [max_out], out_labels [max_out], out_src [max_out] (the slot a row
 *   came from), out_count [1].  All max_out rows of every output are written: 0 / -1 from the count on.
 *   guard          out_count = -1 (and no rows) if any non-BLANK tile has counts[t] < 0, the per-tile step's report
 *                  of non-finite scores
 *
 * Launches: one filter + translate + key kernel, the bitonic sort of the 64-bit keys (csrc/bitonic.h), one unpack
 * kernel, wd_nms_gather on one "image" of n_tile * max_in anchors with identity metadata, one kernel for the guard.
 *
 * workspace: wd_tile_merge_workspace_bytes(n_tile, max_in) bytes, 256-byte aligned, no initialisation needed.
 *
 * WD_ERR_UNSUPPORTED (before any launch): n_tile * max_in > 32768, max_out > 1024, n_tile * max_in * n_cls >= 2^31.
 * WD_ERR_BAD_ARG: null pointers, non-positive sizes, misaligned boxes / out_boxes / workspace, edge_margin < 0 or not
 * finite.  WD_ERR_WORKSPACE: workspace_bytes too small.
 * ------------------------------------------------------------------------------------------- */
int wd_tile_merge(const float* boxes, const float* scores, const int32_t* labels, const int32_t* counts,
                  const WdTile* tiles, int32_t n_tile, int32_t max_in, int32_t n_cls, float edge_margin, float iou_thr,
                  int32_t split_thr, int32_t max_out, float* out_boxes, float* out_scores, int32_t* out_labels,
                  int32_t* out_src, int32_t* out_count, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_TILE_H */
