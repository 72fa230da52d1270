"""The "sparse scores" wrappers of wedetect_amd/sparse.py declared to the happens-before checker (tests/hazards.py): what each
launch reads and writes, from its scalar arguments (include/wedetect_hip_sparse.h, "Extents:").  tests/hazards.py keeps its
tables in module-level dicts, so they are extended here at import time, as tests/best_hazards.py does: every test module of
the mode imports this one, and pytest imports every test module before it runs the first test.

The counters ``state`` are drawn from with atomic adds and the list slots follow from what was drawn: both are classed W (a
read-modify-write, ordered like a write against everything else) — the memset of ``state`` at the head of a step must be ordered
behind the previous step's wd_sparse_select, which reads it, and the checker sees that pair as W against R."""
import os

from tests import hazards as H

R, W, A = H.R, H.W, H.A


def _sparse_similarity_split(a, ret):
    batch = a.rows // a.rows_per_img
    return [H._run(R, a.e_split, H._up8(a.rows) * a.dim * 4), H._run(R, a.t_split, H._up8(a.n_cls) * a.dim * 4, off=a.t_row * a.dim * 4),
            H._run(W, a.list_, batch * a.list_cap * 8), H._run(W, a.state, batch * 8), H._run(A, a.range_flag, 4)]


def _sparse_rows(a, ret):
    rows = a.n_img * a.rows_per_img
    return [H._rect(R, a.scores, rows, a.ld * 4, a.n_cls * 4), H._run(R, a.count, a.n_img * 4), H._run(W, a.list_, a.n_img * a.list_cap * 8),
            H._run(W, a.state, a.n_img * 8)]


def _sparse_select(a, ret):
    from wedetect_amd import lib as L
    cap = L.topk_capacity(a.nms_pre)
    return [H._run(W, a.list_, a.batch * a.list_cap * 8), H._run(R, a.state, a.batch * 8), H._run(W, a.out_idx, a.batch * cap * 4),
            H._run(W, a.out_score, a.batch * cap * 4), H._run(W, a.out_count, a.batch * 4), H._run(W, a.status, a.batch * 4)]


def _flag_line() -> int:
    """The line of csrc/split_gemm_p8.hip on which the candidate epilogue stores the flag."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wedetect_amd", "csrc", "split_gemm_p8.hip")
    lines = open(src).read().splitlines()
    body = max(i for i, l in enumerate(lines) if "p8_sparse_epilogue(" in l and l.startswith("__device__"))     # the definition follows the declaration
    return next(i for i in range(body, len(lines)) if "*p.range_flag = 1u;" in lines[i]) + 1


def declare() -> None:
    if "sparse.sparse_rows" in H.ACCESS:
        return
    H.ACCESS.update({
        "sparse.sparse_similarity_split": _sparse_similarity_split,
        "sparse.sparse_rows": _sparse_rows,
        "sparse.sparse_select": _sparse_select,
    })
    H.BENIGN.append(("sparse.sparse_similarity_split", "range_flag",
                     f"csrc/split_gemm_p8.hip:{_flag_line()} — `if (p.range_flag) *p.range_flag = 1u;` in p8_sparse_epilogue"))


declare()
