"""The tracking wrappers of wedetect_amd/track.py declared to the happens-before checker (tests/hazards.py): what each launch
reads and writes, from its scalar arguments (include/wedetect_hip_track.h, "Extents:").  Extended at import time, as
tests/exemplar_hazards.py does: every test module of the tracker imports this one, and pytest imports every test module before it
runs the first test.  The state is read and written by every step — declared written, whole: two steps on one state are ordered
or they are a hazard."""
from tests import hazards as H

R, W = H.R, H.W


def _track_reset(a, ret):
    return [H._whole(W, a.state), H._run(R, a.seq_mask, a.n_seq * 4)]


def _track_step(a, ret):
    n_img = a.n_seq * a.n_frame
    rows = n_img * a.max_out
    return [H._whole(W, a.state), H._whole(W, a.workspace), H._run(R, a.boxes, rows * 16), H._run(R, a.scores, rows * 4),
            H._run(R, a.labels, rows * 4), H._run(R, a.count, n_img * 4), H._run(R, a.embed, rows * a.dim * 4),
            H._run(W, a.track_ids, rows * 4), H._run(W, a.track_hits, rows * 4)]


def _track_export(a, ret):
    slots = a.n_seq * a.max_tracks
    return [H._whole(R, a.state)] + [H._run(W, t, slots * 4) for t in (a.ids, a.labels, a.scores, a.hits, a.misses)] + \
        [H._run(W, a.boxes, slots * 16), H._run(W, a.seq_info, a.n_seq * 16), H._run(W, a.vel, slots * 16),
         H._run(W, a.embed, slots * a.dim * 4)]


def declare() -> None:
    if "track.track_step" in H.ACCESS:
        return
    H.ACCESS.update({
        "track.track_reset": _track_reset,
        "track.track_step": _track_step,
        "track.track_export": _track_export,
    })


declare()
