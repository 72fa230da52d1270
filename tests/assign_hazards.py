"""The wrappers of wedetect_amd/assign.py declared to the happens-before checker (tests/hazards.py): what each launch reads and
writes, from its scalar arguments (include/addons/wedetect_hip_assign.h, "Extents:").  Extended at import time, as
tests/track_hazards.py does: every test module of the assignment imports this one, and pytest imports every test module before it
runs the first test.  wd_track_step_optimal touches what wd_track_step touches."""
from tests import hazards as H
from tests import track_hazards as TH

R, W = H.R, H.W


def _assign_max_raw(a, ret):
    cells = a.n_a * a.n_b * 4
    return [H._rect(R, a.val, a.n_prob, a.ld_prob * 4, cells), H._run(W, a.match_a, a.n_prob * a.n_a * 4),
            H._run(W, a.match_b, a.n_prob * a.n_b * 4), H._run(W, a.total, a.n_prob * 8), H._run(W, a.status, a.n_prob * 4)]


def declare() -> None:
    if "assign.track_step_optimal" in H.ACCESS:
        return
    H.ACCESS.update({
        "assign.assign_max_raw": _assign_max_raw,
        "assign.track_step_optimal": TH._track_step,
    })


declare()
