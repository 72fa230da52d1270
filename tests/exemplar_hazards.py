"""The exemplar wrappers of wedetect_amd/exemplar.py declared to the happens-before checker (tests/hazards.py): what each launch
reads and writes, from its scalar arguments (include/wedetect_hip_exemplar.h, "Extents:").  Extended at import time, as
tests/topn_hazards.py does: every test module of the exemplar prompts imports this one, and pytest imports every test module
before it runs the first test."""
from tests import hazards as H

R, W = H.R, H.W


def _exemplar_assign(a, ret):
    slots = a.batch * a.max_ex * a.m
    return [H._run(R, a.boxes, a.batch * a.n_anchor * 16), H._run(R, a.ex_boxes, a.batch * a.max_ex * 16), H._run(R, a.ex_count, a.batch * 4),
            H._run(R, a.meta, a.batch * 32), H._run(W, a.sel_anchors, slots * 4), H._run(W, a.sel_iou, slots * 4),
            H._run(W, a.sel_count, a.batch * 4)]


def _exemplar_pool(a, ret):
    return [H._run(R, a.level_embed, 3 * a.n_slot * a.dim * 4), H._run(R, a.sel_anchors, a.n_slot * 4), H._run(R, a.sel_iou, a.n_slot * 4),
            H._run(R, a.cls_off, (a.n_cls + 1) * 4), H._whole(R, a.cls_slot), H._run(W, a.bank, a.n_cls * a.dim * 4),
            H._run(W, a.support, a.n_cls * 4)]


def declare() -> None:
    if "exemplar.exemplar_pool" in H.ACCESS:
        return
    H.ACCESS.update({
        "exemplar.exemplar_assign": _exemplar_assign,
        "exemplar.exemplar_pool": _exemplar_pool,
    })


declare()
