"""The prompt-group wrappers of wedetect_amd/groups.py declared to the happens-before checker (tests/hazards.py): what each launch
reads and writes, from its scalar arguments (include/wedetect_hip_groups.h, "Extents:").  Extended at import time, as
tests/topn_hazards.py does: every test module of the mode imports this one, and pytest imports every test module before it runs
the first test.  Which columns of ``out`` a launch writes is in the device tables; the declaration names all ``n_groups`` columns
of every row, which can only over-report."""
import os

from tests import hazards as H

R, W, A = H.R, H.W, H.A


def _tables(a):
    return [H._run(R, a.group_of, a.n_cls * 4, off=a.cls_offset * 4), H._run(R, a.bin_first, (a.n_cls // 32 + 1) * 4, off=a.cls_offset // 32 * 4)]


def _group_similarity_split(a, ret):
    return [H._run(R, a.e_split, H._up8(a.rows) * a.dim * 4), H._run(R, a.t_split, a.n_cls * a.dim * 4, off=a.t_row * a.dim * 4),
            *_tables(a), H._rect(W, a.out, a.rows, a.ldo * 4, a.n_groups * 4), H._run(A, a.range_flag, 4)]


def _group_rows(a, ret):
    return [H._rect(R, a.block, a.rows, a.ld * 4, a.n_cls * 4), *_tables(a), H._rect(W, a.out, a.rows, a.ldo * 4, a.n_groups * 4)]


def _flag_line() -> int:
    """The line of csrc/split_gemm_p8.hip on which the class-max epilogue stores the flag."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wedetect_amd", "csrc", "split_gemm_p8.hip")
    lines = open(src).read().splitlines()
    body = max(i for i, l in enumerate(lines) if "p8_group_epilogue(" in l and l.startswith("__device__"))     # the definition follows the declaration
    return next(i for i in range(body, len(lines)) if "*p.range_flag = 1u;" in lines[i]) + 1


def declare() -> None:
    if "groups.group_rows" in H.ACCESS:
        return
    H.ACCESS.update({
        "groups.group_similarity_split": _group_similarity_split,
        "groups.group_rows": _group_rows,
    })
    H.BENIGN.append(("groups.group_similarity_split", "range_flag",
                     f"csrc/split_gemm_p8.hip:{_flag_line()} — `if (p.range_flag) *p.range_flag = 1u;` in p8_group_epilogue"))


declare()
