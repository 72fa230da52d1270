"""The optimal association (``track.Tracker(assignment="optimal")``, wd_track_step_optimal) beside the greedy one
(wd_track_step, whose code is untouched), on the same inputs, in one process, on alternating legs.

    python scripts/track_assign_bench.py [--size base] [--batch 32] [--hw 640] [--max-tracks 128] [--k 12]

The setup of scripts/track_bench.py: synthetic weights and seeded images (the same batch every step: a static video in steady
state), an fp16x3 tower calibrated once, an 80-row bank, ``high_thr`` at the median of the kept scores (a crowded scene) and at
their 0.9 quantile.  Per regime, K rounds of the legs ALTERNATELY, each timed by the wall clock around a full drain:

  embed              ``detect(with_embed=True)`` + counts: the step both trackers run behind
  track1 / trackB    that step + ``Tracker.update`` for one video of B frames / for B cameras, greedy and optimal

then the two step kernels alone on the step's rows, alternately, each between two device events; and, on the host, how many
round-1 and round-2 associations of tests/assign_ref.OptRefTracker (fed with the device's rows, one video, two calls) differ from
the greedy picks on the same candidates.  Recorded, not asserted.  Writes the measurement section of profiles/track_assign.txt
(everything from the line that starts with "# == measurement" on; what stands before it — the ISA table — is kept)."""
import argparse
import dataclasses
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
MARK = "# == measurement"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="base")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=640)
    ap.add_argument("--max-tracks", type=int, default=128)
    ap.add_argument("--k", type=int, default=12, help="rounds of the alternating legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_assign.txt"))
    args = ap.parse_args(argv)

    import torch
    from tests import assign_ref as A
    from tests import track_ref as R
    from wedetect_amd import track as T
    from wedetect_amd import weights as W
    from wedetect_amd.engine import EMBED_DIM, ImageTower
    from wedetect_amd.pack import pack

    assert torch.cuda.is_available(), "a measurement needs the device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, hw = args.batch, args.hw
    tower = ImageTower(args.size, pack(W.make_state_dict(args.size), args.size), B, hw, hw, max_classes=80, precision="fp16x3")
    x = torch.from_numpy(W.make_images(B, hw, hw)).cuda()
    meta = tower.identity_meta()
    meta[:, 7] = 1.0
    tower.calibrate(x)
    bank = torch.from_numpy(W.make_text_bank(80)).cuda()
    kw = dict(normalize_text=True, score_thr=0.001, iou_thr=0.7, nms="mmcv")

    def step():
        res = tower.detect(x, bank, meta, with_embed=True, **kw)
        return res, res["count"].tolist()

    res, counts = step()
    say(f"{MARK}: scripts/track_assign_bench.py on {torch.cuda.get_device_name(0)} ({platform.node()}); model {args.size}, batch {B} x {hw} x "
        f"{hw}, fp16x3, 80 classes, max_out {tower.max_out}, max_tracks {args.max_tracks}, K = {args.k} alternating rounds")
    stat = lambda v: f"mean {v.mean():9.3f} ms  median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}  std {v.std():7.3f}"
    for q in (0.5, 0.9):
        kept = torch.cat([res["scores"][b, :n] for b, n in enumerate(counts)]).cpu().numpy()
        p = T.TrackParams(high_thr=float(np.quantile(kept, q)), low_thr=float(np.quantile(kept, q / 2)), new_thr=float(np.quantile(kept, q)))
        trackers = {(a, n): T.Tracker(n, args.max_tracks, EMBED_DIM, p, assignment=a) for a in T.ASSIGNMENTS for n in (1, B)}
        last = {}

        def leg(key):
            r, _ = step()
            last[key] = trackers[key].update(r, B // key[1])
            torch.cuda.synchronize()

        legs = {"embed": step}
        legs.update({key: (lambda key=key: leg(key)) for key in trackers})
        for _ in range(2):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        per = {n: [] for n in legs}
        for _ in range(args.k):
            for n, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                per[n].append((time.perf_counter() - t0) * 1e3)
        t = {n: np.asarray(v) for n, v in per.items()}
        med = {n: float(np.median(v)) for n, v in t.items()}
        info = {key: tr.tracks() for key, tr in trackers.items()}
        hi = int((res["scores"] >= p.high_thr).sum()) // B
        say(f"## high_thr at the {q} quantile of the kept scores ({p.high_thr:.4f}; rows at or above it per image: about {hi}), low_thr at the "
            f"{q / 2} quantile ({p.low_thr:.4f}); rows kept per image {min(counts)} .. {max(counts)}")
        for a in T.ASSIGNMENTS:
            say(f"{a:8s}: live tracks, one video {len(info[(a, 1)][0]['ids'])} (status {info[(a, 1)][0]['status']}), cameras "
                f"{min(len(s['ids']) for s in info[(a, B)])} .. {max(len(s['ids']) for s in info[(a, B)])}; rows with an id in the last "
                f"step {int((last[(a, 1)][0] > 0).sum())} / {int((last[(a, B)][0] > 0).sum())}")
        say(f"rows whose id differs between the two trackers in the last step: one video "
            f"{int((last[('greedy', 1)][0] != last[('optimal', 1)][0]).sum())}, cameras {int((last[('greedy', B)][0] != last[('optimal', B)][0]).sum())}")
        say(f"step with_embed=True                           : {stat(t['embed'])}")
        for n, what in ((1, f"one video of {B} frames"), (B, f"{B} cameras")):
            for a in T.ASSIGNMENTS:
                say(f"step + track, {what:22s} {a:8s}: {stat(t[(a, n)])}")
            say(f"medians, {what}: optimal - greedy = {med[('optimal', n)] - med[('greedy', n)]:+.3f} ms; tracker behind the step: greedy "
                f"{med[('greedy', n)] - med['embed']:.3f} ms, optimal {med[('optimal', n)] - med['embed']:.3f} ms")
        say(f"noise of this run (largest std of a leg): {max(v.std() for v in t.values()):.3f} ms")
        # ---- the two kernels alone on the step's rows, alternately
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kt = {key: [] for key in trackers}
        for _ in range(max(args.k, 20)):
            for key in trackers:
                ev[0].record()
                trackers[key].update(res, B // key[1])
                ev[1].record()
                torch.cuda.synchronize()
                kt[key].append(ev[0].elapsed_time(ev[1]))
        for n, what in ((1, f"1 workgroup x {B} frames"), (B, f"{B} workgroups x 1 frame")):
            for a, name in (("greedy", "wd_track_step"), ("optimal", "wd_track_step_optimal")):
                say(f"kernel {name:21s} {what:24s}: {stat(np.asarray(kt[(a, n)]))}")
        # ---- how often the optimum differs from the greedy picks on these inputs (host reference on the device's rows, two calls)
        rows = [res[k].cpu().numpy() for k in ("bboxes", "scores", "labels", "count", "embeddings")]
        ref = A.OptRefTracker(1, args.max_tracks, EMBED_DIM, R.Params(**{f.name: getattr(p, f.name) for f in dataclasses.fields(p)}))
        for _ in range(2):
            ref.step(*rows, B)
        say(f"reference on these rows, one video, 2 x {B} frames: round-1 associations {ref.calls_by_round[0]}, of which "
            f"{ref.differs_by_round[0]} differ from greedy's; round-2 associations {ref.calls_by_round[1]}, of which {ref.differs_by_round[1]} "
            f"differ; smallest uniqueness margin {ref.assign_margin:.3e}")
    head = ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        head = old[:old.index(MARK)] if MARK in old else old
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(head + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
