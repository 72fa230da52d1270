/*
 * wedetect_hip_track.h — tracking of libwedetect_hip.so (MI355X / gfx950 only): persistent object ids across the frames of a
 * video, associated on the device.  The rows a detection step keeps (wd_nms_gather and its labelled / sparse siblings) carry
 * their region embeddings; the association below uses them as the appearance feature, so no second network runs and nothing is
 * downloaded between frames.  The rule is the two rounds of ByteTrack (high-score detections first, low-score ones against the
 * tracks that were seen in the previous frame) with an appearance term in the first round as in BoT-SORT, greedy instead of
 * Hungarian, a constant-velocity prediction instead of a Kalman filter.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_track_abi_version), like wedetect_hip_exemplar.h and the
 * other add-on headers: the entry points below are compiled into the same library and follow the same conventions — plain C
 * types, device pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no allocation, no global atomics,
 * no mutable global state (the tracks live in a buffer of the caller's), WD_OK or a negative WD_ERR_* code (wedetect_hip.h).
 * Every refusal below happens before any launch.
 *
 * Result definition (every path; tests/track_ref.py restates it in numpy).
 *
 * A launch serves n_seq independent sequences of n_frame consecutive frames each: image b = s * n_frame + f is frame f of
 * sequence s (one video: n_frame = batch; one frame of each of B cameras: n_frame = 1).  Per image: boxes [max_out][4] in
 * original-image pixels, scores, labels, count, embed [max_out][dim].  Only rows r < min(count[b], max_out) are read; count[b] < 0
 * makes the frame empty and sets status bit 1 (WD_TRACK_STATUS_BAD_COUNT).
 *
 * Per sequence: max_tracks slots (1 .. WD_TRACK_MAX_TRACKS).  A live slot (id >= 1) holds id, label, score, box and velocity
 * (4 fp32 each, x1 y1 x2 y2), a unit embedding t with a has_embed flag, hits and misses.  The sequence also holds next_id
 * (1 after a reset) and the sticky status word.
 *
 * WdTrackParams holds PARAMETERS of the rule, not tuned values: the library has no defaults and no opinion about them.
 *
 * Frames run in order.  Every fp32 operation is individually rounded, never fused.
 *  1. Predict.  pred = box + vel per coordinate, for every live slot.
 *  2. Round 1: the rows with score >= high_thr against ALL live slots.
 *       iou  = the fp32 IoU of pred with the row's box in the operation order of the NMS kernels,
 *                  area_p = (p.x2 - p.x1) * (p.y2 - p.y1);  area_d likewise;
 *                  w = max(0, min(p.x2, d.x2) - max(p.x1, d.x1));  h likewise;  inter = w * h;
 *                  iou = inter / (area_p + area_d - inter)           (the correctly rounded division), a NaN counts as 0;
 *       cos  = (sum_d t[d] * e[d]) * inv_e with inv_e = 1 / sqrt(sum_d e[d]^2); 0 when the slot has no embedding or the row's
 *              sum of squares is zero or not finite (the row's embedding is then "not usable");
 *       sim  = w_iou * iou + w_app * max(cos, 0), w_app = 1 - w_iou rounded once on the host.
 *     A pair is a candidate iff sim >= match_thr (and, with match_labels != 0, the slot's label equals the row's).  Greedy:
 *     repeatedly take the largest key  (uint64) bits(sim) << 32 | (0xFFFF - slot) << 16 | (0xFFFF - row)  among the candidates
 *     whose slot and row are both still free.  Thresholds are > 0, so a candidate's value is > 0 and its bits order like it.
 *  3. Round 2: the rows with low_thr <= score < high_thr that round 1 left (all of them) against the slots round 1 left
 *     unmatched whose misses == 0.  IoU only: candidate iff iou >= iou2_thr, the same label rule, the same greedy on bits(iou).
 *  4. Update.  A matched slot: vel = ema_vel * vel + (1 - ema_vel) * (det - box) (1 - ema_vel rounded once on the host; two
 *     multiplies, one add), box = det, the row's label and score, hits += 1, misses = 0.  A round-1 match whose row embedding is
 *     usable: with ê = e * inv_e, v = ema_embed * t + (1 - ema_embed) * ê, t = v * (1 / sqrt(sum_d v[d]^2)) — t keeps its value if
 *     that sum is zero or not finite; a slot without an embedding takes ê and sets has_embed.  A round-2 match leaves t alone.
 *     An unmatched live slot: box = pred, misses += 1; it is freed (id = 0) when misses > max_age.
 *     Then the unmatched rows with score >= new_thr start tracks, in row order, each in the lowest free slot (a slot freed in
 *     this frame included): id = next_id++, vel = 0, hits = 1, misses = 0, t = ê / has_embed = 1 if the embedding is usable,
 *     has_embed = 0 otherwise.  If no slot is free the row gets no id and status bit 0 (WD_TRACK_STATUS_FULL) is set.
 *  5. Outputs per frame, aligned with the detection rows: track_ids [n_img][max_out] int32 (0 = none, and 0 from count on) and
 *     track_hits likewise (the slot's hits after the update).  Every element is written.
 *
 * Sums over d use one reduction tree, fixed by the kernel, that depends on nothing but dim: lane l of a wave adds the products of
 * the elements d with (d / 4) % 64 == l into four accumulators (one per d % 4), chunk after chunk, then (a0 + a1) + (a2 + a3), then
 * a 64-lane xor butterfly.  A pair's cos depends on the bits of its two vectors only: equal inputs tie exactly and the key
 * resolves the tie (lowest slot, then lowest row).
 *
 * Identities, bit for bit: n_frame frames in one launch == n_frame launches of one frame; a sequence's results do not depend on
 * what the other sequences hold; two runs give the same bits.
 *
 *   wd_track_state_bytes / wd_track_workspace_bytes   sizes of the caller's two buffers
 *   wd_track_reset    all sequences, or the selected ones, to "no tracks, next_id 1, status 0"
 *   wd_track_step     the rule above, one launch for n_seq x n_frame images
 *   wd_track_export   the slots of every sequence as plain arrays
 */
#ifndef WEDETECT_HIP_TRACK_H
#define WEDETECT_HIP_TRACK_H

#include <stdint.h>

#include "wedetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_TRACK_MAX_TRACKS 256
#define WD_TRACK_MAX_OUT 1024
#define WD_TRACK_MAX_DIM 1024
#define WD_TRACK_STATUS_FULL 1       /* bit 0: a row with score >= new_thr found no free slot */
#define WD_TRACK_STATUS_BAD_COUNT 2  /* bit 1: a frame arrived with count < 0 */

/* Parameters of the association rule — parameters, NOT tuned values: no trained weights or video data stand behind any setting,
 * the caller chooses them.  Host memory, read before the launch. */
typedef struct WdTrackParams {
  float high_thr;       /* round 1 takes rows with score >= high_thr */
  float low_thr;        /* round 2 takes rows with low_thr <= score < high_thr;   low_thr <= high_thr */
  float new_thr;        /* an unmatched row with score >= new_thr starts a track;  new_thr >= high_thr */
  float match_thr;      /* round 1: candidate iff sim >= match_thr;   > 0 */
  float iou2_thr;       /* round 2: candidate iff iou >= iou2_thr;    > 0 */
  float w_iou;          /* weight of the IoU in sim, in [0, 1]; the appearance term has 1 - w_iou */
  float ema_embed;      /* in [0, 1]: share of the old embedding in the update */
  float ema_vel;        /* in [0, 1]: share of the old velocity in the update */
  int32_t max_age;      /* >= 0: a slot is freed when misses > max_age */
  int32_t match_labels; /* != 0: a pair needs equal labels */
} WdTrackParams;

/* Bumped on any change of a signature or of WdTrackParams. */
int wd_track_abi_version(void);

/* Bytes of the state of n_seq sequences (a multiple of 16), 0 for arguments wd_track_step refuses.  Per sequence, in 4-byte
 * words: next_id, status, 2 unused; then [max_tracks] each of id, label, score, hits, misses, has_embed; box [max_tracks][4];
 * vel [max_tracks][4]; padded to a multiple of 4 words; then embed [max_tracks][dim].  The layout is the library's: callers read
 * the state through wd_track_export. */
int64_t wd_track_state_bytes(int32_t n_seq, int32_t max_tracks, int32_t dim);

/* Bytes of the workspace of wd_track_step (a multiple of 16, never 0 for valid arguments), 0 for arguments it refuses: the
 * candidate matrix of a sequence, max_tracks x max_out fp32, used where it exceeds the kernel's LDS tile. */
int64_t wd_track_workspace_bytes(int32_t n_seq, int32_t max_tracks, int32_t max_out);

/* ---------------------------------------------------------------------------------------------
 * wd_track_reset — sequences to "no tracks, next_id 1, status 0".
 *
 *   state     device, 16-byte aligned, wd_track_state_bytes(n_seq, max_tracks, dim) bytes; any contents
 *   seq_mask  device int32 [n_seq] or NULL: NULL resets every sequence, otherwise those with seq_mask[s] != 0
 *
 * One workgroup of 256 lanes per sequence.  The embeddings are not touched: a free slot's embedding is never read.
 *
 * Extents: reads seq_mask[0, n_seq) if given; writes, for each reset sequence, its 4 header words and its per-slot words up to
 * the embeddings (4 + 14 * max_tracks words), nothing else.
 * WD_ERR_BAD_ARG: null state, n_seq outside 1 .. 65535, max_tracks outside 1 .. 256, dim outside 4 .. 1024 or dim % 4, state not
 * 16-byte aligned, seq_mask not 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int wd_track_reset(void* state, int32_t n_seq, int32_t max_tracks, int32_t dim, const int32_t* seq_mask, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_track_step — the rule above for n_seq sequences of n_frame frames.
 *
 *   state       device, 16-byte aligned (wd_track_state_bytes), reset once; read and written
 *   workspace   device, 16-byte aligned (wd_track_workspace_bytes); any contents, nothing in it outlives the launch
 *   boxes       device fp32 [n_seq * n_frame][max_out][4], 16-byte aligned
 *   scores      device fp32 [n_seq * n_frame][max_out];   labels   device int32 likewise;   count   device int32 [n_seq * n_frame]
 *   embed       device fp32 [n_seq * n_frame][max_out][dim], 16-byte aligned
 *   max_out     1 .. WD_TRACK_MAX_OUT;   dim   % 4 == 0, 4 .. WD_TRACK_MAX_DIM
 *   params      host, see WdTrackParams
 *   track_ids   device int32 [n_seq * n_frame][max_out];   track_hits   likewise
 *
 * One workgroup of 256 lanes per sequence walks its frames in order with the slots' scalars in LDS (the embeddings stay in the
 * state).  A frame's work is bounded by its live slots and its count, both read on the device.  Round 1: a wave holds two rows'
 * embeddings in registers and streams the live slots' embeddings past them, 16 bytes per lane, eight slots in flight; the values
 * land in an LDS tile (6144 pairs) or, beyond that, in the workspace, and a second pass, one pair per lane, adds the IoU term.
 * Greedy: one best key per slot, a 256-lane maximum per pick, and only the slots that lost their row look again.
 *
 * Extents: reads count[0, n_img), and for each image boxes / scores / labels / embed rows [0, min(count, max_out)) — embed only
 * of rows with score >= high_thr; reads and writes the state of every sequence (embeddings of live slots only) and at most
 * max_tracks * max_out words per sequence of the workspace; writes track_ids / track_hits [0, n_img * max_out), whole.
 * WD_ERR_BAD_ARG: null pointers, n_seq outside 1 .. 65535, n_frame < 1, n_seq * n_frame * max_out * dim > 2^31 - 16, max_tracks /
 * max_out / dim outside the ranges above, state / workspace / boxes / embed not 16-byte aligned, another device pointer not
 * 4-byte aligned, a parameter that is not finite or outside its range (see WdTrackParams), low_thr > high_thr, new_thr < high_thr.
 * ------------------------------------------------------------------------------------------- */
int wd_track_step(void* state, void* workspace, const float* boxes, const float* scores, const int32_t* labels,
                  const int32_t* count, const float* embed, int32_t n_seq, int32_t n_frame, int32_t max_out, int32_t max_tracks,
                  int32_t dim, const WdTrackParams* params, int32_t* track_ids, int32_t* track_hits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * wd_track_export — the slots of every sequence as plain arrays.
 *
 *   ids, labels, hits, misses   device int32 [n_seq][max_tracks] (id 0 = free; a free slot's other fields are 0)
 *   scores                      device fp32 [n_seq][max_tracks];   boxes   device fp32 [n_seq][max_tracks][4] (the slot's box: the
 *                               last matched detection, moved by its velocity once per missed frame)
 *   seq_info                    device int32 [n_seq][4]: next_id, n_live, status, 0
 *   vel                         device fp32 [n_seq][max_tracks][4] or NULL: the slots' velocities
 *   embed                       device fp32 [n_seq][max_tracks][dim], 16-byte aligned, or NULL: the unit embeddings, zero rows
 *                               for free slots and slots without one
 *
 * One workgroup of 256 lanes per sequence.
 *
 * Extents: reads the state (embeddings of live slots with has_embed only); writes every element of the outputs given, nothing else.
 * WD_ERR_BAD_ARG: null pointers (vel and embed excepted), sizes as for wd_track_reset, state or embed not 16-byte aligned, another pointer
 * not 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int wd_track_export(const void* state, int32_t n_seq, int32_t max_tracks, int32_t dim, int32_t* ids, int32_t* labels, float* scores,
                    float* boxes, int32_t* hits, int32_t* misses, int32_t* seq_info, float* vel, float* embed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_TRACK_H */
