"""The single-label wrappers of wedetect_amd/best.py declared to the happens-before checker (tests/hazards.py): what each
launch reads and writes, from its scalar arguments (include/wedetect_hip_best.h, "Extents:").  tests/hazards.py keeps its
tables in module-level dicts, so they are extended here at import time: every test module of the single-label mode imports
this one, and pytest imports every test module before it runs the first test."""
import os

from tests import hazards as H

R, W, A = H.R, H.W, H.A


def _best_similarity_split(a, ret):
    # the keys are merged with an atomic maximum: a read-modify-write, ordered like a write against everything else
    return [H._run(R, a.e_split, H._up8(a.rows) * a.dim * 4), H._run(R, a.t_split, H._up8(a.n_cls) * a.dim * 4, off=a.t_row * a.dim * 4),
            H._run(W, a.key, a.rows * 8), H._run(A, a.range_flag, 4)]


def _best_rows(a, ret):
    rows = a.n_img * a.rows_per_img
    return [H._rect(R, a.scores, rows, a.ld * 4, a.n_cls * 4), H._run(R, a.count, a.n_img * 4), H._run(W, a.key, rows * 8)]


def _nms_gather_labeled(a, ret):
    return H._nms_gather(a, ret) + [H._run(R, a.anchor_labels, a.batch * a.n_anchor * 4)]


def _flag_line() -> int:
    """The line of csrc/split_gemm_p8.hip on which the key epilogue (the last function of the file that does) stores the flag."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wedetect_amd", "csrc", "split_gemm_p8.hip")
    lines = open(src).read().splitlines()
    body = max(i for i, l in enumerate(lines) if "p8_best_epilogue(" in l and l.startswith("__device__"))      # the definition follows the declaration
    return next(i for i in range(body, len(lines)) if "*p.range_flag = 1u;" in lines[i]) + 1


def declare() -> None:
    if "best.best_rows" in H.ACCESS:
        return
    H.ACCESS.update({
        "best.best_similarity_split": _best_similarity_split,
        "best.best_rows": _best_rows,
        "best.best_unpack": lambda a, r: [H._run(R, a.key, a.rows * 8), H._run(W, a.scores_out, a.rows * 4), H._run(W, a.labels_out, a.rows * 4)],
        "best.nms_gather_labeled": _nms_gather_labeled,
    })
    H.BENIGN.append(("best.best_similarity_split", "range_flag",
                     f"csrc/split_gemm_p8.hip:{_flag_line()} — `if (p.range_flag) *p.range_flag = 1u;` in p8_best_epilogue"))


declare()
