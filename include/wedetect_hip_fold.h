/*
 * wedetect_hip_fold.h — the text bank FOLDED into the head's embedding conv (libwedetect_hip.so, MI355X / gfx950 only).
 *
 * The BN-contrastive head's logit is linear in the embedding conv's input c2 (the 256-channel output of head{l}.cls1):
 *     logit[b, n, k] = < W_e c2[b, n] + b_e , t_k > e^scale_l + bias_l
 *                    = < c2[b, n] , (t W_e)_k > e^scale_l + < b_e , t_k > e^scale_l + bias_l
 * so a step scores every anchor from c2 with the [K, 256] folded weights of its level and computes the 768-d embeddings of
 * the rows the post-process keeps only (wedetect_amd.engine.ImageTower._fold_text / _similarity_folded / _kept_embeddings).
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_fold_abi_version), like wedetect_hip_feed.h,
 * wedetect_hip_tile.h and wedetect_hip_views.h: same library, same conventions — plain C types, device pointers, a
 * hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no mutable global state, WD_OK or a
 * negative WD_ERR_* code (wedetect_hip.h).
 */
#ifndef WEDETECT_HIP_FOLD_H
#define WEDETECT_HIP_FOLD_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on any change of a signature below. */
int wd_fold_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * wd_fold_similarity — one head level of the folded similarity: wd_conv_gemm_split(p, w_split, w_unscale, WD_SPLIT_A) on the
 * implicit-GEMM LDS-DMA kernel (the kernel the level's embedding conv runs on), with ONE addition: the weights' unscale is
 * w_unscale * *w_unscale_dev, the second factor a DEVICE float (a power of two).  The fold chooses the pre-split scale of the
 * folded weights on the device, so a new bank costs no host read and a captured graph follows an in-place refold.  (That holds
 * for the banks the unfolded step scores with the fp32 similarity GEMM, fewer than 256 rows by default.  For larger banks the
 * engine also keeps wd_split_weights of the bank for the re-scoring of the kept rows, wd_kept_rows_reorder: one host read per new
 * bank, as in the unfolded step, and a captured step of such a bank is not folded.)
 *
 *   p                a 1x1 / stride 1 layer over pre-split rows (p->a: fp16 hi/lo groups, cin % 16 == 0, lda % 8 == 0) with
 *                    c_batch_stride > 0 (rows of image b go to b * c_batch_stride + pos of the [B, anchors, K] scores), fp32
 *                    output, no residual / c2 / LayerNorm fold / seg; out_scale, out_bias, sigmoid, range_flag as in wd_conv_gemm.
 *                    ANY n (the bank size) and ldc >= n, p->c 4-byte aligned: where n % 8, ldc % 4 or the address keep the
 *                    kernel from its 16-byte stores, a row's 8-column pieces are stored element by element, columns < n
 *                    only (wd_conv_gemm_split accepts such fp32 row outputs of this kernel too);
 *                    p->bias: round_up(n, 8) floats, 16-byte aligned, or NULL
 *   w_split          wd_split_weights_padded(n, cin) of the folded weights
 *   w_unscale_dev    device float, read by the kernel
 * Extents: reads the batch * hin * win rows of lda floats of p->a, the round_up(n, 8) rows of w_split and of p->bias, one float
 * at w_unscale_dev; writes columns < n of the m mapped output rows only.
 * Address widths, here and for wd_conv_gemm / wd_conv_gemm_split (whose own header, wedetect_hip.h, is frozen at ABI 15 and
 * says "lda >= cin" only): rows of a, c, res and c2 are addressed with 64-bit offsets, so m * lda, m * ldc, m * ldres, m * ldc2
 * and batch * c_batch_stride * ldc may pass 2^31 and 2^32 bytes.  Two limits, both WD_ERR_UNSUPPORTED: the forced tiles cfg 64 /
 * 65 / 66 of wd_conv_gemm_split need m * lda * 4 < 2^32 and n * round_up(k, 16) * 4 < 2^32 (32-bit operand offsets; cfg < 0
 * never picks them beyond that), and a kh x kw layer on pre-split activations (WD_SPLIT_A), the row-sharing 3 x 3 kernels
 * included, needs ((kh - 1) * win + kw - 1) * lda * 4 + cin * 4 <= 2^31 (a filter tap's byte offset from its pixel is a 32-bit
 * int; a 1 x 1 layer such as this entry's is never refused by it).
 */
int wd_fold_similarity(const WdConvGemm* p, const void* w_split, float w_unscale, const float* w_unscale_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_kept_rows_gather — the c2 rows of the anchors wd_nms_gather kept, grouped by head level, for the three embedding GEMMs
 * that follow.  Row r = b * max_out + i of gathered[l] ([3][batch * max_out][row_floats]) receives the row of anchor
 * a = out_anchors[b, i] from level l's buffer (c2[l] + ((size_t)b * rows[l] + a - off[l]) * row_floats, off = {0, off1, off2})
 * when i < out_count[b] and a lies in level l, and ZEROS otherwise (every row of gathered is written: the GEMMs read all).
 * The rows are copied as bytes: fp32 rows or fp16 hi/lo groups alike.
 *
 *   c2_0..c2_2       device, 16-byte aligned, [batch * rows_l][row_floats]
 *   rows0..rows2     anchors per image of the level (> 0); off1 = rows0, off2 = rows0 + rows1 by the caller's layout
 *   row_floats       % 4 == 0, 4 .. 1024
 *   out_anchors      device int32 [batch][max_out]; out_count device int32 [batch] (values outside 0 .. max_out are clamped;
 *                    an anchor outside 0 .. rows0 + rows1 + rows2 - 1 gives zero rows)
 *   gathered         device, 16-byte aligned, 3 * batch * max_out * row_floats floats
 */
int wd_kept_rows_gather(const float* c2_0, const float* c2_1, const float* c2_2, int32_t rows0, int32_t rows1, int32_t rows2,
                        int32_t row_floats, const int32_t* out_anchors, const int32_t* out_count, int32_t max_out,
                        int32_t batch, float* gathered, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_kept_rows_select — out_embed[b, i, :] = level_embed[l][b * max_out + perm[b, i]][:] with l the level of out_anchors[b, i]
 * for i < out_count[b], ZEROS for i >= out_count[b] (what wd_nms_gather's own gather leaves there).
 *
 *   level_embed      device, 16-byte aligned, [3][batch * max_out][dim] fp32: the three embedding GEMMs' outputs
 *   dim              % 4 == 0, > 0
 *   perm             device int32 [batch][max_out] from wd_kept_rows_reorder (values clamped to 0 .. max_out - 1), or NULL:
 *                    the rows are where the GEMMs left them (perm[b, i] = i)
 *   out_embed        device, 16-byte aligned, [batch][max_out][dim]
 */
int wd_kept_rows_select(const float* level_embed, int32_t dim, int32_t off1, int32_t off2, const int32_t* out_anchors,
                        const int32_t* out_count, const int32_t* perm, int32_t max_out, int32_t batch, float* out_embed,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_kept_rows_reorder — the kept rows of a folded step take the scores and the order of the unfolded step.  The folded
 * scores differ from the unfolded ones in their last bits, which is enough to swap neighbours in wd_nms_gather's output.
 * level_scores[l][b * max_out + i][:] holds the unfolded similarity GEMM's scores of kept row (b, i) computed with level l's
 * scale and bias (the caller runs that GEMM on the kept rows' embeddings); row (b, i), i < out_count[b], gets
 * level_scores[level of its anchor][b * max_out + i][out_labels[b, i]], and the rows of image b are then sorted as
 * wd_topk_candidates sorts: score descending, anchor * k + label ascending.  out_boxes / out_scores / out_labels / out_anchors
 * are permuted IN PLACE (rows >= out_count[b] untouched); perm[b, j] = the slot the row now at j came from (j itself for
 * j >= out_count[b]).  A row whose anchor or label is out of range keeps its score.
 *
 *   level_scores     device fp32 [3][batch * max_out][k]
 *   n_anchor         anchors per image; 0 <= off1 <= off2 <= n_anchor
 *   out_boxes        device, 16-byte aligned, [batch][max_out][4]; out_scores / out_labels / out_anchors [batch][max_out]
 *   max_out          1 .. 1024 (wd_nms_gather's limit); out_count values outside 0 .. max_out are clamped
 *   perm             device int32 [batch][max_out], written completely
 */
int wd_kept_rows_reorder(const float* level_scores, int32_t k, int32_t n_anchor, int32_t off1, int32_t off2, float* out_boxes,
                         float* out_scores, int32_t* out_labels, int32_t* out_anchors, const int32_t* out_count,
                         int32_t max_out, int32_t batch, int32_t* perm, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WEDETECT_HIP_FOLD_H */
