"""The bank-tuning wrappers of wedetect_amd/tune.py declared to the happens-before checker (tests/hazards.py): what each launch
reads and writes, from its scalar arguments (include/wedetect_hip_tune.h, "Extents:").  Extended at import time, as
tests/exemplar_hazards.py does: every test module of the bank tuning imports this one, and pytest imports every test module
before it runs the first test."""
from tests import hazards as H

R, W = H.R, H.W


def _k_pad(n_cls):
    return (n_cls + 31) // 32 * 32


def _tune_targets(a, ret):
    slots, rows = a.batch * a.max_ex * a.m, a.batch * a.n_anchor
    return [H._run(R, a.sel_anchors, slots * 4), H._run(R, a.sel_iou, slots * 4), H._run(R, a.ex_cls, a.batch * a.max_ex * 4),
            H._run(W, a.pos_cls, rows * 4), H._run(W, a.pos_y, rows * 4)]


def _tune_grad(a, ret):
    kp = _k_pad(a.n_cls)
    return [H._run(R, a.embed, a.rows * a.dim * 4), H._run(R, a.pos_cls, a.rows * 4), H._run(R, a.pos_y, a.rows * 4),
            H._run(R, a.bank, a.n_cls * a.dim * 4), H._run(W, a.slabs, a.n_split * kp * a.dim * 4),
            H._run(W, a.loss_parts, a.n_split * (kp // 32) * 4)]


def _tune_update(a, ret):
    kp, row = _k_pad(a.n_cls), a.n_cls * a.dim * 4
    return [H._run(R, a.slabs, a.n_slab * kp * a.dim * 4), H._run(R, a.loss_parts, a.n_slab * (kp // 32) * 4),
            H._run(R, a.trainable, a.n_cls), H._run(W, a.w, row), H._run(W, a.m, row), H._run(W, a.v, row), H._run(W, a.bank, row),
            H._run(W, a.loss_out, 4, off=4 * a.step), H._run(W, a.status, 4)]


def declare() -> None:
    if "tune.tune_grad" in H.ACCESS:
        return
    H.ACCESS.update({
        "tune.tune_targets": _tune_targets,
        "tune.tune_grad": _tune_grad,
        "tune.tune_update": _tune_update,
    })


declare()
