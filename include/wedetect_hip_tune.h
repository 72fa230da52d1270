/*
 * wedetect_hip_tune.h — bank tuning of libwedetect_hip.so (MI355X / gfx950 only): the rows of a class bank learned from
 * labelled boxes with both towers frozen.  The class bank is then the only thing that learns, and its gradient is the region x
 * text similarity GEMM run forwards and then backwards: S = E·Tᵀ, p = sigmoid(a·S + b), dT = ((p − y)·a)ᵀ·E.  The [rows, K]
 * matrix in the middle is never written.  The region embeddings of the labelled images are computed once by the image tower and
 * cached; an optimisation step is then one fused two-GEMM launch per cached chunk and one update launch, no tower in the loop.
 * The result is an ordinary [K, 768] bank of unit rows, used exactly like a text bank.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_tune_abi_version), like wedetect_hip_exemplar.h and the
 * other add-on headers: the entry points below are compiled into the same library and follow the same conventions — plain C
 * types, device pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no atomics, no
 * mutable global state, WD_OK or a negative WD_ERR_* code (wedetect_hip.h).  Every refusal below happens before any launch.
 *
 * Result definition (tests/tune_ref.py restates it in float64 numpy).
 *
 * The cache is a list of chunks; a chunk is one batch's region embeddings and targets:
 *     E        fp32 [rows][768], rows = batch * n_anchor: the post-BN embeddings (ImageTower.embed after an unfolded features())
 *     pos_cls  int32 [rows]: the class the row is a positive of, or -1 (the row is a negative for every class)
 *     pos_y    fp32 [rows]: the target of that class (the IoU of the row's anchor with the labelled box)
 * Row r belongs to anchor r % n_anchor, whose head level is l = (anchor >= off1) + (anchor >= off2); its logit scale is
 * a_r = scale[l] (= exp(logit_scale_l), as ImageTower.lvl_scale holds it) and its bias b_r = bias[l].  The six floats are passed
 * by value.
 *
 * Targets are static.  For every labelled box, wd_exemplar_assign (wedetect_hip_exemplar.h, unchanged) gives the m anchors whose
 * decoded boxes overlap it best.  wd_tune_targets resolves the slots of one image into per-anchor targets: an anchor claimed by
 * several slots keeps the claim with the larger IoU, ties going to the lower slot index (the lower example index); pos_cls is that
 * box's class and pos_y its IoU; every other anchor gets (-1, 0.0f).  Every element of both arrays is written.
 * Why static: the reference's task-aligned assigner ranks anchors by a metric that contains the score of the class being learned,
 * which is noise for a fresh row, so the assignment would follow the initialisation and not the boxes.  Targets that do not depend
 * on the bank are also what lets the embeddings be computed once: nothing in a step depends on the image tower.
 *
 * Parameters and loss.  The parameters are raw rows W fp32 [K][768]; t_k = W_k / ||W_k||.
 *     z[r,k]  = a_r * <E_r, t_k> + b_r
 *     y[r,k]  = pos_y[r] if pos_cls[r] == k, else 0
 *     norm    = max(sum_r pos_y[r], 1) over all chunks (the caller computes it once and passes 1 / norm)
 *     loss    = sum_{r,k} bce(z, y) / norm,   bce = max(z, 0) - z*y + log1p(exp(-|z|))
 *               (the reference's loss_cls: sigmoid cross-entropy, summed, divided by assigned_scores_sum.clamp(min=1))
 *     g[r,k]  = (sigmoid(z) - y) / norm,   sigmoid(z) = 1 / (1 + e) for z >= 0 and e / (1 + e) otherwise, e = exp(-|z|)
 *     dt_k    = sum_r a_r * g[r,k] * E_r
 *     dW_k    = (dt_k - <dt_k, t_k> t_k) / ||W_k||
 *
 * Update: Adam without weight decay, on the rows whose trainable[k] byte is non-zero.
 *     m <- beta1 m + (1 - beta1) dW;   v <- beta2 v + (1 - beta2) dW^2
 *     W <- W - lr * (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps);   then T_k = W_k / ||W_k||
 * A row with a zero byte keeps W, m, v and T bit for bit (new classes learned beside frozen text rows that serve as negatives).
 * A trainable row whose norm — before or after the step — is zero or not finite sets *status = 1 and is left unchanged.
 *
 * Determinism.  No float atomics anywhere: partial sums go to slabs that are summed in a fixed order, so the same inputs give
 * the same bits on every run.  Given the split count, a class's gradient depends neither on which other classes the bank holds
 * nor on the class's position in it: every element of S is eight k-ordered fmaf chains over 96 dimensions each, joined by one
 * fixed tree, and every element of dt one k-ordered chain over the rows of the workgroup's range, whichever lane holds the class.
 *
 *   wd_tune_plan      (rows, K) -> the split count of wd_tune_grad: a pure host function
 *   wd_tune_targets   the selected slots of wd_exemplar_assign -> per-anchor targets
 *   wd_tune_grad      one chunk, forwards and backwards: partial-gradient slabs and partial losses
 *   wd_tune_update    slabs of all chunks -> projection, Adam step, renormalisation, loss_out[step]
 */
#ifndef WEDETECT_HIP_TUNE_H
#define WEDETECT_HIP_TUNE_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_TUNE_DIM 768         /* the embedding width every entry point below is built for */
#define WD_TUNE_CLASS_BLOCK 32  /* classes per workgroup of wd_tune_grad: K_pad = ceil(K / 32) * 32 */
#define WD_TUNE_ROW_TILE 128    /* rows per sweep step: a split owns whole tiles */
#define WD_TUNE_MAX_SPLIT 256

/* Bumped on any change of a signature below. */
int wd_tune_abi_version(void);

/* The split count wd_tune_grad is meant to run with for a chunk of `rows` rows and a bank of n_cls classes, so that small banks
 * still fill the chip: min(ceil(rows / 128), max(1, 256 / ceil(n_cls / 32))), one workgroup per (class block, split) and at most
 * one workgroup per CU (K = 80: three class blocks x 85 splits).  0 for rows <= 0 or n_cls <= 0.  Touches no device. */
int32_t wd_tune_plan(int64_t rows, int32_t n_cls);

/* ---------------------------------------------------------------------------------------------
 * wd_tune_targets — the target resolution above for batch images.
 *
 *   sel_anchors  device int32 [batch][max_ex * m];   sel_iou   device fp32 likewise   (wd_exemplar_assign; -1 = an empty slot)
 *   ex_cls       device int32 [batch][max_ex]: the class of example e of image b; read only for slots that hold an anchor
 *   max_ex       1 .. WD_EXEMPLAR_MAX_EX (64);   m   1 .. WD_EXEMPLAR_MAX_M (8)
 *   pos_cls      device int32 [batch][n_anchor];   pos_y   device fp32 likewise
 *
 * One workgroup of 256 lanes per image: the <= 512 slots go to LDS, every anchor is written (-1, 0), and behind a barrier every
 * slot that no other slot of the same anchor beats (larger IoU, or equal IoU and lower slot) writes its anchor.  A slot whose
 * anchor is outside [0, n_anchor) claims nothing.
 *
 * Extents: reads sel_anchors / sel_iou [0, batch * max_ex * m), ex_cls[b][e] of the slots with an anchor in range; writes
 * pos_cls / pos_y [0, batch * n_anchor) only, whole.
 * WD_ERR_BAD_ARG: null pointers, non-positive batch / n_anchor, max_ex outside 1 .. 64, m outside 1 .. 8, a pointer not
 * 4-byte aligned, batch > 65535, batch * n_anchor > 2^31 - 16.
 * ------------------------------------------------------------------------------------------- */
int wd_tune_targets(const int32_t* sel_anchors, const float* sel_iou, const int32_t* ex_cls, int32_t max_ex, int32_t m,
                    int32_t batch, int32_t n_anchor, int32_t* pos_cls, float* pos_y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_tune_grad — one chunk forwards and backwards: dt and the loss of the result definition, in n_split partial sums.
 *
 *   embed        device fp32 [rows][dim], 16-byte aligned;   dim   must be 768
 *   n_anchor, off1, off2   row r is anchor r % n_anchor; 0 < off1 < off2 <= n_anchor
 *   scale0..2, bias0..2    a and b of the three head levels, finite
 *   pos_cls      device int32 [rows];   pos_y   device fp32 [rows]
 *   bank         device fp32 [n_cls][dim], 16-byte aligned: the unit rows t_k
 *   inv_norm     1 / norm, finite and > 0
 *   n_split      1 .. WD_TUNE_MAX_SPLIT
 *   slabs        device fp32 [n_split][K_pad][dim], 16-byte aligned, K_pad = ceil(n_cls / 32) * 32: slab s holds the sum of
 *                a_r * g[r,k] * E_r over the rows of split s; rows k >= n_cls of a slab are zero
 *   loss_parts   device fp32 [n_split][K_pad / 32]: the sum of bce / norm over the split's rows and the block's classes
 *
 * Split s owns the row tiles [s * nt / n_split, (s + 1) * nt / n_split) of 128 rows, nt = ceil(rows / 128) (an empty range
 * writes zeros).  One workgroup of 256 lanes per (class block of 32, split), its 32 x 768 block of t in LDS (96 KiB) and its
 * 32 x 768 block of dt in 96 accumulator registers per lane for the whole sweep (class-on-the-workgroup, as attention backward
 * keeps dK).  Per tile each of the four waves computes S for 32 rows x 32 classes with mfma_f32_32x32x2f32 (eight accumulators of
 * 96 dimensions each, joined by one fixed tree: short chains, and eight independent ones in flight), applies scale, bias,
 * sigmoid and the sparse target in registers, leaves a * g in LDS (16 KiB), and accumulates its 192 columns of dt over the tile's
 * 128 rows with the same instruction.  No atomics.
 *
 * Loss accumulation chain: a lane adds the bce of its 16 elements of a tile sequentially, tile after tile, so the longest
 * sequential chain of a partial is 16 * ceil(ceil(rows / 128) / n_split) terms, followed by a 6-level butterfly over the wave
 * and 3 adds over the waves; wd_tune_update then adds the partials sequentially per lane and in a fixed tree.
 *
 * embed must be finite: a row past the end of the last, ragged tile re-reads row rows - 1 with g == 0, so an inf or NaN in that
 * row would reach every class's dt as 0 * inf (wedetect_amd/tune.py checks its cache before the first step).
 *
 * Extents: reads embed[0, rows * dim), pos_cls / pos_y [0, rows), bank[0, n_cls * dim); writes slabs[0, n_split * K_pad * dim)
 * and loss_parts[0, n_split * K_pad / 32) only, whole.
 * WD_ERR_BAD_ARG: null pointers, dim != 768, non-positive rows / n_anchor / n_cls, not 0 < off1 < off2 <= n_anchor, a scale or
 * bias that is not finite, inv_norm not finite or <= 0, n_split outside 1 .. 256, embed / bank / slabs not 16-byte aligned,
 * another pointer not 4-byte aligned, rows * dim > 2^31 - 16, n_cls > 65535 * 32, n_split * K_pad * dim >= 2^40.
 * ------------------------------------------------------------------------------------------- */
int wd_tune_grad(const float* embed, int32_t rows, int32_t dim, int32_t n_anchor, int32_t off1, int32_t off2, float scale0,
                 float scale1, float scale2, float bias0, float bias1, float bias2, const int32_t* pos_cls, const float* pos_y,
                 const float* bank, int32_t n_cls, float inv_norm, int32_t n_split, float* slabs, float* loss_parts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_tune_update — the slabs of ALL chunks -> dW, the Adam step and the renormalised rows; the step's loss.
 *
 *   slabs        device fp32 [n_slab][K_pad][dim], 16-byte aligned: the slabs of every chunk's wd_tune_grad, one behind the other
 *   loss_parts   device fp32 [n_slab * K_pad / 32]: their partial losses, likewise
 *   n_cls, dim   K; dim must be 768
 *   w, m, v      device fp32 [n_cls][dim]: raw rows and the two Adam moments, updated in place
 *   bank         device fp32 [n_cls][dim]: t, rewritten for the rows that stepped
 *   trainable    device uint8 [n_cls]: a zero byte freezes the row
 *   lr, beta1, beta2, eps   finite; lr >= 0, 0 <= beta < 1, eps > 0
 *   bc1, bc2     1 - beta1^t and 1 - beta2^t of this step (t >= 1), in (0, 1]
 *   loss_out     device fp32 [>= step + 1]: loss_out[step] is written
 *   status       device uint32 [1]: set to 1 by a trainable row whose norm is zero or not finite; never cleared here
 *
 * One workgroup of 256 lanes per class row; a lane owns 3 floats of it.  dt_k is the sum over the slabs in slab order; the
 * dot product and the two norms use one fixed tree.  Workgroup 0 also sums the partial losses (lane i adds entries i, i + 256,
 * ... in order, then the tree).
 *
 * Extents: reads slabs[i][k][0, dim) for k < n_cls (the padded rows are not read), loss_parts[0, n_slab * K_pad / 32),
 * trainable[0, n_cls), and w / m / v / bank rows of the trainable classes; writes those rows of w / m / v / bank,
 * loss_out[step] and (only on a bad norm) status[0].
 * WD_ERR_BAD_ARG: null pointers, dim != 768, non-positive n_slab / n_cls, negative step, a hyper-parameter outside the ranges
 * above, slabs not 16-byte aligned, another float or word pointer not 4-byte aligned, n_cls > 65535 * 32,
 * n_slab * K_pad * dim >= 2^40.
 * ------------------------------------------------------------------------------------------- */
int wd_tune_update(const float* slabs, int32_t n_slab, const float* loss_parts, int32_t n_cls, int32_t dim, float* w, float* m,
                   float* v, float* bank, const uint8_t* trainable, float lr, float beta1, float beta2, float eps, float bc1,
                   float bc2, float* loss_out, int32_t step, uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_TUNE_H */
