"""Tracking (``track.Tracker`` behind an in-line ``ImageTower.detect`` step) beside the plain step, beside the step that only
gathers the embeddings, and beside the host route it replaces, in one process.

    python scripts/track_bench.py [--size base] [--batch 32] [--hw 640] [--max-tracks 128] [--k 12]

Synthetic weights and seeded images (the same batch every step: a static video in steady state, every track matched in every
frame), an fp16x3 tower calibrated once, an 80-row bank.  No trained weights are here, so the score thresholds are set from the
first step's own scores, twice — ``high_thr`` at the median of the kept rows (a crowded scene: every slot taken) and at their 0.9
quantile (about 30 tracked rows per frame), ``low_thr`` at half that quantile — to give both rounds work; the counts that result
are printed.  K rounds of the legs ALTERNATELY, each timed by the wall clock around a full drain and
ending, like ``predict``, with the counts on the host:

  predict      ``detect(with_embed=False)`` + counts
  embed        ``detect(with_embed=True)`` + counts: the step ``track`` runs — isolates the tracker from the cost of gathering
  track n_seq  ``detect(with_embed=True)`` + counts + ``Tracker.update`` (one launch), for one video of B frames and for B cameras
  host         ``detect(with_embed=True)`` + download of rows and embeddings + tests/track_ref.py (numpy, its margin bookkeeping
               switched off; written to be read, not to be fast: an upper figure for a host tracker), one video

and ``wd_track_step`` alone on the step's rows, each between two device events.  Recorded, not asserted: prints everything and
writes profiles/track.txt.
"""
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="base")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=640)
    ap.add_argument("--max-tracks", type=int, default=128)
    ap.add_argument("--k", type=int, default=12, help="rounds of the alternating legs")
    ap.add_argument("--host-k", type=int, default=3, help="rounds of the host route (numpy: slow)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track.txt"))
    args = ap.parse_args(argv)

    import torch
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

    def step(with_embed):
        res = tower.detect(x, bank, meta, with_embed=with_embed, **kw)
        return res, res["count"].tolist()

    res, counts = step(True)
    say(f"# {torch.cuda.get_device_name(0)} on {platform.node()}; model {args.size}, batch {B} x {hw} x {hw}, fp16x3, 80 classes, max_out "
        f"{tower.max_out}, max_tracks {args.max_tracks}, K = {args.k} rounds (host route {args.host_k})")
    for q in (0.5, 0.9):                                                   # a crowded scene (half of the rows tracked) and a sparser one
        kept = torch.cat([res["scores"][b, :n] for b, n in enumerate(counts)]).cpu().numpy()
        p = T.TrackParams(high_thr=float(np.quantile(kept, q)), low_thr=float(np.quantile(kept, q / 2)), new_thr=float(np.quantile(kept, q)))
        trackers = {1: T.Tracker(1, args.max_tracks, EMBED_DIM, p), B: T.Tracker(B, args.max_tracks, EMBED_DIM, p)}
        rp = R.Params(**{f.name: getattr(p, f.name) for f in dataclasses.fields(p)})
        ref = R.RefTracker(1, args.max_tracks, EMBED_DIM, rp, margins=False)   # the rule alone, without the tests' bookkeeping

        last = {}

        def leg_track(n_seq):
            r, c = step(True)
            last[n_seq] = trackers[n_seq].update(r, B // n_seq)
            torch.cuda.synchronize()
            return last[n_seq]

        def leg_host():
            r, c = step(True)
            rows = [r[k].cpu().numpy() for k in ("bboxes", "scores", "labels", "count", "embeddings")]
            return ref.step(*rows, B)

        legs = {"predict": lambda: step(False), "embed": lambda: step(True), "track1": lambda: leg_track(1), "trackB": lambda: leg_track(B)}
        for _ in range(2):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        per = {n: [] for n in legs}
        per["host"] = []
        for i in range(args.k):
            for n, fn in list(legs.items()) + ([("host", leg_host)] if i < args.host_k else []):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                per[n].append((time.perf_counter() - t0) * 1e3)
        info = {n: tr.tracks() for n, tr in trackers.items()}
        ids1 = last[1][0]
        hi = int((res["scores"] >= p.high_thr).sum()) // B
        say(f"## high_thr at the {q} quantile of the kept scores, low_thr at the {q / 2} quantile")
        say(f"rows kept per image {min(counts)} .. {max(counts)}; high_thr {p.high_thr:.4f} (rows at or above it per image: about {hi}), low_thr "
            f"{p.low_thr:.4f}; live tracks: one video {len(info[1][0]['ids'])} (status {info[1][0]['status']}), cameras "
            f"{min(len(t['ids']) for t in info[B])} .. {max(len(t['ids']) for t in info[B])}; rows with an id in the last step "
            f"{int((ids1 > 0).sum())}")
        stat = lambda v: f"mean {v.mean():9.3f} ms  median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}  std {v.std():7.3f}"
        t = {n: np.asarray(v) for n, v in per.items()}
        say(f"step predict (no embeddings)          : {stat(t['predict'])}")
        say(f"step with_embed=True                  : {stat(t['embed'])}")
        say(f"step + track, one video of {B:3d} frames : {stat(t['track1'])}")
        say(f"step + track, {B:3d} cameras            : {stat(t['trackB'])}")
        say(f"step + download + numpy reference     : {stat(t['host'])}")
        med = {n: float(np.median(v)) for n, v in t.items()}
        say(f"medians: track - embed = {med['track1'] - med['embed']:.3f} ms (one video), {med['trackB'] - med['embed']:.3f} ms (cameras); embed - predict = "
            f"{med['embed'] - med['predict']:.3f} ms; track / predict = {med['track1'] / med['predict']:.4f} and {med['trackB'] / med['predict']:.4f}; host route - embed = "
            f"{med['host'] - med['embed']:.1f} ms; noise of this run (largest std of a device leg) "
            f"{max(t[n].std() for n in legs):.3f} ms")
        # ---- the kernel alone on the step's rows
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kt = {1: [], B: []}
        for _ in range(max(args.k, 20)):
            for n_seq in (1, B):
                ev[0].record()
                trackers[n_seq].update(res, B // n_seq)
                ev[1].record()
                torch.cuda.synchronize()
                kt[n_seq].append(ev[0].elapsed_time(ev[1]))
        say(f"kernel wd_track_step, 1 workgroup x {B} frames : {stat(np.asarray(kt[1]))}")
        say(f"kernel wd_track_step, {B} workgroups x 1 frame : {stat(np.asarray(kt[B]))}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
