/*
 * wedetect_hip_assign.h — optimal (Hungarian) assignment of libwedetect_hip.so (MI355X / gfx950 only): a maximum-weight matching
 * solved on the device, as an entry point of its own (wd_assign_max) and as the association of the tracker
 * (wd_track_step_optimal) beside the greedy rule of wedetect_hip_track.h.  ByteTrack and BoT-SORT associate by a linear assignment
 * problem; the greedy rule differs from it exactly where two rows compete for the same two slots.  No claim about tracking quality
 * is made here: the result below is defined and tested as an optimisation problem, nothing more.
 *
 * An addition to include/wedetect_hip.h with a version of its own (wd_assign_abi_version), like wedetect_hip_track.h, and with
 * the same conventions: plain C types, device pointers, a hipStream_t passed as void*, asynchronous on the caller's stream, no
 * allocation, no global atomics, no mutable global state, WD_OK or a negative WD_ERR_* code (wedetect_hip.h).  Every refusal
 * below happens before any launch.  The header lives in include/addons/ (-I include reaches it as "addons/wedetect_hip_assign.h").
 *
 * Result definition (every path; tests/assign_ref.py restates it in numpy and holds it to scipy.optimize.linear_sum_assignment).
 *
 * A problem is a candidate matrix in the tracker's layout: val[j * n_a + i], fp32, i < n_a the slot-side index, j < n_b the
 * row-side index; 0 means "no candidate", a candidate's value is >= thr > 0.  Weights are integers, so the optimum is exact and
 * does not depend on the order of any reduction:
 *
 *     q(x)    = (int32) min(floorf(x * 2^20), 2^21)       (exact in fp32: a power-of-two product, a floor, a minimum)
 *     w[i][j] = q(val) - q(thr) + 1   where val is a finite value > 0 and that is >= 1,      0 ("no candidate") otherwise
 *
 * so 0 <= w <= 2^21 + 1.  A value that is negative or not finite (a NaN, an infinity) is no candidate and sets status bit 1; a
 * positive value below thr whose weight would be < 1 is no candidate either (no status bit: it is merely below the threshold).
 *
 * The result is a maximum-weight matching: a set of candidate pairs, no i and no j twice, with the largest sum of w.  Indices may
 * stay unmatched — a pair is taken iff it pays against leaving both ends unmatched, the objective of lapjv(cost_limit = ...).  In
 * scipy's terms: linear_sum_assignment(W, maximize=True) on the [n_a, n_b] matrix W, keeping the pairs with W > 0.
 *
 * Where the optimum is not unique any optimum is correct, and the kernel's choice is deterministic: the same bits on every run,
 * independent of the other problems of the launch, and, in the tracker, n frames in one launch == n launches of one frame.  (The
 * arithmetic is integer and every minimum takes the lowest column among equals.)
 *
 * The solver.  One workgroup of 256 lanes per problem: shortest augmenting paths with potentials (Hungarian / Jonker-Volgenant) on
 * the costs -w.  "May stay unmatched" is one private column of cost 0 per i (n_a dummy columns), so every i is assigned and the
 * problem is always feasible.  The a-side is augmented one index at a time; each Dijkstra step is one scan of the columns — a lane
 * owns columns tid, tid + 256, ... and dummy column tid, with their distances, potentials and visited flags in registers — plus one
 * 256-lane arg-min in which the lowest column wins ties.  int32 throughout: a dummy column's potential never moves from 0, hence
 * every potential stays in [-(2^21 + 1), 0], a path length in [-(2^21 + 1), 0] and a tentative distance within +-2^23.
 * Every loop has a trip count fixed by the sizes alone: the outer loop runs n_a times, the search at most n_a + 1 steps (the
 * matched columns plus one free one), the walk back along the path likewise — whatever the bits of val are.  Should a search end
 * at its bound without a free column — it cannot — that i stays unmatched and status bit 0 is set: the bit proves it did not happen.
 *
 *   wd_assign_workspace_bytes / wd_assign_max                     the solver on n_prob matrices
 *   wd_track_optimal_workspace_bytes / wd_track_step_optimal      wd_track_step with this association
 */
#ifndef WEDETECT_HIP_ASSIGN_H
#define WEDETECT_HIP_ASSIGN_H

#include <stdint.h>

#include "wedetect_hip.h"
#include "wedetect_hip_track.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_ASSIGN_MAX_A WD_TRACK_MAX_TRACKS  /* 256: the slot side, one lane each */
#define WD_ASSIGN_MAX_B WD_TRACK_MAX_OUT     /* 1024: the row side */
#define WD_ASSIGN_STATUS_BOUND 1             /* bit 0: a search ended at its step bound without a free column (cannot happen) */
#define WD_ASSIGN_STATUS_BAD_VALUE 2         /* bit 1: a negative or non-finite value was seen and treated as no candidate */
#define WD_TRACK_STATUS_ASSIGN_BOUND 4       /* bit 2 of a sequence's status word, wd_track_step_optimal only: as bit 0 above */

/* Bumped on any change of a signature. */
int wd_assign_abi_version(void);

/* Bytes of the workspace of wd_assign_max (a multiple of 16, never 0 for valid arguments), 0 for arguments it refuses.  The
 * solver keeps its arrays in LDS and registers; the workspace is reserved (16 bytes per problem) and not touched today. */
int64_t wd_assign_workspace_bytes(int32_t n_prob, int32_t n_a, int32_t n_b);

/* ---------------------------------------------------------------------------------------------
 * wd_assign_max — the maximum-weight matching of the result definition for n_prob problems of one size.
 *
 *   val        device fp32, 4-byte aligned: problem p is val[p * ld_prob + j * n_a + i];  ld_prob >= n_a * n_b
 *   n_prob     1 .. 65535;   n_a   1 .. WD_ASSIGN_MAX_A;   n_b   1 .. WD_ASSIGN_MAX_B
 *   thr        finite, > 0
 *   match_a    device int32 [n_prob][n_a]: the j matched to i, or -1
 *   match_b    device int32 [n_prob][n_b]: the i matched to j, or -1
 *   total      device int64 [n_prob], 8-byte aligned: the sum of w over the matched pairs
 *   status     device int32 [n_prob]: 0, or WD_ASSIGN_STATUS_* bits
 *   workspace  device, 16-byte aligned, workspace_bytes >= wd_assign_workspace_bytes(n_prob, n_a, n_b)
 *
 * One workgroup of 256 lanes per problem; about 6 KB of LDS.
 *
 * Extents: reads val[p * ld_prob, p * ld_prob + n_a * n_b) of every problem, nothing between the problems; writes every element of
 * match_a, match_b, total and status, nothing else; the workspace is neither read nor written.
 * WD_ERR_BAD_ARG: null pointers, n_prob / n_a / n_b outside the ranges above, ld_prob < n_a * n_b, (n_prob - 1) * ld_prob + n_a * n_b
 * > 2^40, a thr that is not finite or <= 0, val / match_a / match_b / status not 4-byte aligned, total not 8-byte aligned, workspace
 * not 16-byte aligned.  WD_ERR_WORKSPACE (-3): workspace_bytes below the size query.
 * ------------------------------------------------------------------------------------------- */
int wd_assign_max(const float* val, int32_t n_prob, int32_t n_a, int32_t n_b, int64_t ld_prob, float thr, int32_t* match_a,
                  int32_t* match_b, int64_t* total, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* Bytes of the workspace of wd_track_step_optimal (a multiple of 16, never 0 for valid arguments), 0 for arguments it refuses:
 * the candidate matrix of a sequence as for wd_track_step (wd_track_workspace_bytes).  The solver's arrays add about 6 KB to
 * the step kernel's LDS object (62 KB in all, below 64 KB), so neither the kernel's LDS tile nor this workspace changes size. */
int64_t wd_track_optimal_workspace_bytes(int32_t n_seq, int32_t max_tracks, int32_t max_out);

/* ---------------------------------------------------------------------------------------------
 * wd_track_step_optimal — wd_track_step (wedetect_hip_track.h) with the optimal association: its arguments in its order, plus
 * workspace_bytes; the same state layout, WdTrackParams and outputs.  wd_track_reset and wd_track_export serve both steps, and
 * a state may be stepped by either from frame to frame.
 *
 * Everything in the result definition of wedetect_hip_track.h holds with one change: in rounds 1 and 2, "Greedy: repeatedly take
 * the largest key ..." is replaced by "the maximum-weight matching of this header's result definition over the same candidates,
 * with thr = match_thr (round 1) / iou2_thr (round 2), i the live slots in ascending order and j the round's rows in ascending
 * order".  The identities of that header hold bit for bit.  Status bit 2 (WD_TRACK_STATUS_ASSIGN_BOUND) is this step's alone.
 *
 * The same kernel as wd_track_step's — one source text for the frame walk — with the solver above in place of the greedy picks.
 *
 * Extents: as wd_track_step: reads count[0, n_img), and for each image boxes / scores / labels / embed rows [0, min(count, max_out))
 * — embed only of rows with score >= high_thr; reads and writes the state of every sequence (embeddings of live slots only) and at
 * most max_tracks * max_out words per sequence of the workspace; writes track_ids / track_hits [0, n_img * max_out), whole.
 * WD_ERR_BAD_ARG: every refusal of wd_track_step.  WD_ERR_WORKSPACE (-3): workspace_bytes below the size query.
 * ------------------------------------------------------------------------------------------- */
int wd_track_step_optimal(void* state, void* workspace, const float* boxes, const float* scores, const int32_t* labels,
                          const int32_t* count, const float* embed, int32_t n_seq, int32_t n_frame, int32_t max_out,
                          int32_t max_tracks, int32_t dim, const WdTrackParams* params, int32_t* track_ids, int32_t* track_hits,
                          int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEDETECT_HIP_ASSIGN_H */
