"""The top-n wrappers of wedetect_amd/topn.py declared to the happens-before checker (tests/hazards.py): what each launch reads
and writes, from its scalar arguments (include/wedetect_hip_topn.h, "Extents:").  Extended at import time, as
tests/best_hazards.py does: every test module of the top-n mode imports this one, and pytest imports every test module before it
runs the first test."""
import os

from tests import hazards as H

R, W, A = H.R, H.W, H.A


def _topn_similarity_split(a, ret):
    # the keys are merged by a cascade of atomic maxima: a read-modify-write, ordered like a write against everything else
    return [H._run(R, a.e_split, H._up8(a.rows) * a.dim * 4), H._run(R, a.t_split, H._up8(a.n_cls) * a.dim * 4, off=a.t_row * a.dim * 4),
            H._run(R, a.row_scale, a.rows * 4), H._run(R, a.row_bias, a.rows * 4),
            H._run(W, a.key, a.rows * a.n_top * 8), H._run(A, a.range_flag, 4)]


def _topn_rows(a, ret):
    rows = a.n_img * a.rows_per_img
    return [H._rect(R, a.block, rows, a.ld * 4, a.n_cls * 4), H._run(R, a.count, a.n_img * 4), H._run(R, a.row_scale, rows * 4),
            H._run(R, a.row_bias, rows * 4), H._run(W, a.key, rows * a.n_top * 8)]


def _topn_unpack(a, ret):
    # one slot of every row: 8 bytes every n_top * 8
    return [H._rect(R, a.key, a.rows, a.n_top * 8, 8) if a.slot == 0 else H._run(R, a.key, a.rows * a.n_top * 8),
            H._run(W, a.scores_out, a.rows * 4), H._run(W, a.labels_out, a.rows * 4)]


def _topn_kept(a, ret):
    n = a.batch * a.max_out
    return [H._run(R, a.key, a.batch * a.n_anchor * a.n_top * 8), H._run(R, a.out_anchors, n * 4), H._run(R, a.out_count, a.batch * 4),
            H._run(W, a.top_scores, n * a.n_top * 4), H._run(W, a.top_labels, n * a.n_top * 4)]


def _flag_line() -> int:
    """The line of csrc/split_gemm_p8.hip on which the top-n epilogue stores the flag."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wedetect_amd", "csrc", "split_gemm_p8.hip")
    lines = open(src).read().splitlines()
    body = max(i for i, l in enumerate(lines) if "p8_topn_epilogue(" in l and l.startswith("__device__"))      # the definition follows the declaration
    return next(i for i in range(body, len(lines)) if "*p.range_flag = 1u;" in lines[i]) + 1


def declare() -> None:
    if "topn.topn_rows" in H.ACCESS:
        return
    H.ACCESS.update({
        "topn.topn_similarity_split": _topn_similarity_split,
        "topn.topn_rows": _topn_rows,
        "topn.topn_unpack": _topn_unpack,
        "topn.topn_kept": _topn_kept,
    })
    H.BENIGN.append(("topn.topn_similarity_split", "range_flag",
                     f"csrc/split_gemm_p8.hip:{_flag_line()} — `if (p.range_flag) *p.range_flag = 1u;` in p8_topn_epilogue"))


declare()
