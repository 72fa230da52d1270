/*
 * wedetect_hip_feed.h — batched ragged pre-processing ("the feed") of libwedetect_hip.so (MI355X / gfx950 only).
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_feed_abi_version): the entry points below are
 * compiled into the same library and follow the same conventions — plain C types, device pointers, a hipStream_t
 * passed as void*, asynchronous on the caller's stream, no allocation, no mutable global state, capture-safe,
 * WD_OK or a negative WD_ERR_* code (codes and the WD_CVRESIZE_* modes: wedetect_hip.h).
 *
 * What it replaces: the per-image launches of wd_cv_resize_paste_u8 / wd_letterbox_u8 (one or two kernels and up to
 * six table uploads per image) followed by the permute -> stack -> wd_chw_to_hwc_u8 round trip of a dataset loop
 * (test.py, eval_recall/eval_recall.py, YOLOWorldDetector.predict).  One call resamples and pads a whole batch of
 * decoded images of different sizes into the tower's [batch, dst_h, dst_w, 3] uint8 canvas in at most two kernel
 * launches, whatever the batch size and the mix of sizes and modes.  Every output byte equals what the per-image
 * entry point writes for that image (same integer arithmetic; the float accumulation of WD_CVRESIZE_AREA keeps its
 * operation order, contraction off).
 */
#ifndef WEDETECT_HIP_FEED_H
#define WEDETECT_HIP_FEED_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on any change of WdFeedImage or of a signature below. */
int wd_feed_abi_version(void);

/* mode of an image: one of the four WD_CVRESIZE_* values (OpenCV family, wd_cv_resize_paste_u8) or */
#define WD_FEED_PILLOW 4        /* Pillow's two-pass 22-bit antialiased BILINEAR (wd_letterbox_u8) */

/* ---------------------------------------------------------------------------------------------
 * WdFeedImage — one image of a batch.  Images of one batch may use different modes.
 *
 *   src_off          byte offset of the image (uint8 HWC, 3 channels, dense rows) in the source arena; the host
 *                    feed places images at multiples of 256, the kernels need no alignment
 *   sh, sw           source size;  new_h, new_w: resampled size, pasted at (top, left) of the canvas
 *   fill             colour of every canvas pixel outside the pasted rectangle, one byte per canvas channel:
 *                    c0 | c1 << 8 | c2 << 16 (written as is: swap_rb does not reorder it)
 *   swap_rb          != 0: resampled pixels are written with channels 0 and 2 exchanged (BGR <-> RGB)
 *   mode             WD_CVRESIZE_COPY / AREA_FAST / AREA / LINEAR or WD_FEED_PILLOW
 *   xa .. yw         ELEMENT offsets (4-byte elements) of the image's tables in the table arena, -1 = none.
 *                    Contents and lengths are those of the per-image entry points:
 *                      AREA    xa [new_w, 2], xidx / xw [taps]; ya [new_h, 2], yidx / yw [taps]
 *                      LINEAR  xa [new_w, 2], xidx [new_w]; ya [new_h, 2], yidx [new_h]
 *                      PILLOW  xa = bounds_h [new_w, 2], xidx = kk_h [new_w, ksize_h];
 *                              ya = bounds_v [new_h, 2], yidx = kk_v [new_h, ksize_v]
 *                    Images may share tables (the host deduplicates them within a batch).
 *   ksize_h, ksize_v PILLOW: row length of kk_h / kk_v
 *   p0, p1, p2       as wd_cv_resize_paste_u8 (AREA_FAST: iscale_x, iscale_y, 1.f / (p0 * p1); LINEAR: p0 = xmax)
 *   tmp_off          PILLOW: byte offset of the image's intermediate in the tmp arena; it takes
 *                    wd_feed_tmp_bytes(sh, new_w) bytes (rows padded to a 16-byte pitch)
 * ------------------------------------------------------------------------------------------- */
typedef struct WdFeedImage {
  int64_t src_off;
  int64_t tmp_off;
  int32_t sh, sw, new_h, new_w, top, left;
  int32_t fill, swap_rb, mode;
  int32_t xa, xidx, xw, ya, yidx, yw;
  int32_t ksize_h, ksize_v;
  int32_t p0, p1;
  float p2;
} WdFeedImage;

/* sizeof(WdFeedImage) as the library was compiled (binding self-check). */
int32_t wd_feed_sizeof_image(void);

/* Bytes of one PILLOW image's intermediate: sh rows of new_w pixels at a 16-byte row pitch, rounded up to 256. */
int64_t wd_feed_tmp_bytes(int32_t sh, int32_t new_w);

/* ---------------------------------------------------------------------------------------------
 * wd_feed_batch_u8 — resample + pad `batch` images into dst [batch, dst_h, dst_w, 3] uint8.
 *
 *   src, src_bytes       device source arena
 *   images               DEVICE array of `batch` descriptors
 *   images_host          the same descriptors in host memory: read during the call (argument checks and grid
 *                        sizes; nothing is read back from the device), not needed afterwards
 *   tables, table_elems  device table arena of 4-byte elements (int32 / float32); may be NULL / 0 when no image
 *                        names a table
 *   tmp, tmp_bytes       device tmp arena; may be NULL / 0 without PILLOW images
 *
 * Alignment: `tables` is 4-byte aligned; with PILLOW images `tmp` and every PILLOW image's `tmp_off` are 16-byte
 * aligned (the intermediate's rows keep their 16-byte pitch in memory; wd_feed_tmp_bytes is a multiple of 256, so
 * ranges laid out back to back from an aligned base qualify).  src and dst need none.  Anything else: WD_ERR_BAD_ARG.
 *
 * Launches: one ragged horizontal pass over the PILLOW images (skipped when there is none), then one pass over the
 * whole canvas (vertical pass / resize / paste / fill; image = blockIdx.y, so the mode is uniform per workgroup).
 * Each lane produces four canvas pixels and stores them as three dwords when dst_w % 4 == 0 and dst is 4-byte
 * aligned (rows of every shipped canvas size are 16-byte multiples); otherwise the same lanes store bytes.
 *
 * Extents
 *   read      [src_off, src_off + sh * sw * 3) of every image; of the table arena only the ranges a descriptor
 *             names (lengths above); the `batch` device descriptors
 *   written   all batch * dst_h * dst_w * 3 bytes of dst, nothing else of the caller's besides tmp
 *   tmp       [tmp_off, tmp_off + wd_feed_tmp_bytes(sh, new_w)) of every PILLOW image is written before it is
 *             read: no initialisation needed; ranges of different images must not overlap
 *
 * WD_ERR_BAD_ARG: a descriptor that does not fit its arenas or the canvas, an unknown mode, a table offset an image's
 * mode needs that is negative or whose documented length passes table_elems, the mode conditions of
 * wd_cv_resize_paste_u8.
 * ------------------------------------------------------------------------------------------- */
int wd_feed_batch_u8(const uint8_t* src, int64_t src_bytes, const WdFeedImage* images, const WdFeedImage* images_host,
                     int32_t batch, const void* tables, int64_t table_elems, uint8_t* tmp, int64_t tmp_bytes,
                     uint8_t* dst, int32_t dst_h, int32_t dst_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_FEED_H */
