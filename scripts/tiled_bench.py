"""Tiled inference of one large image, three ways, in one process.

    python scripts/tiled_bench.py [--size base] [--hw 2160,3840] [--k 80] [--tile-batch 32] [--classes 80]

A seeded 2160 x 3840 image (smooth content plus a little noise), the detector with synthetic weights and an 80-class bank,
every leg warmed, then K rounds of the three legs ALTERNATELY (a, b, c, a, b, c, ...), each timed by the wall clock around a
full drain:

  (a) ``YOLOWorldDetector.predict_tiled``: upload, one cut launch, pipelined steps, one merge, one download;
  (b) the route on the plain API: host crops (numpy slices, the overview through the test pipeline), ``predict`` on the same
      groups of tiles — which reads the counts back after every step — every tile's rows downloaded, the merge in numpy
      (tests/tile_ref.py on oracle.postprocess.mmcv_batched_nms);
  (c) the floor: the same pipelined steps on tiles that are already on the device — no upload, no cut, no merge; one read of
      the last step's counts ends it.

Reported: the three legs (mean, min, max, the spread of each), (a) - (c) = what the upload, the cut, the stacking copies, the
merge and the download cost, and whether (a) <= (b) beyond the leg-to-leg noise of this run (the larger of the two spreads).
Also checked: (a) and (b) return the same rows.  Prints everything and writes profiles/tiled.txt.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_image(h: int, w: int, seed: int = 2026) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    chans = []
    for c in range(3):
        a = np.zeros((h, w), np.float32)
        for _ in range(3):
            fx, fy, ph = rng.uniform(0.003, 0.04), rng.uniform(0.003, 0.04), rng.uniform(0, 6.28)
            a += rng.uniform(20, 45) * np.sin(fx * xx + ph) * np.cos(fy * yy + ph * 0.7)
        chans.append(127 + a + rng.normal(0, 6, (h, w)).astype(np.float32))
    return np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="base")
    ap.add_argument("--hw", default="2160,3840")
    ap.add_argument("--k", type=int, default=80)
    ap.add_argument("--tile-batch", type=int, default=32)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--edge-margin", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled.txt"))
    args = ap.parse_args(argv)

    import torch
    from tests import tile_ref as R
    from wedetect_amd import tiling as G
    from wedetect_amd import weights as W
    from wedetect_amd.detector import YOLOWorldDetector

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    H, Wd = (int(v) for v in args.hw.split(","))
    img = make_image(H, Wd)
    names = [f"class {k}" for k in range(args.classes)]
    model = YOLOWorldDetector(args.size, max_classes=args.classes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict(args.size).items()})
    model.cuda().eval()
    bank = torch.from_numpy(W.make_text_bank(args.classes)).cuda()
    model.set_text_embeddings(bank, [[n] for n in names])
    tile = tuple(model.img_scale)
    plan = G.plan_tiles(H, Wd, tile, args.overlap)
    steps = G.step_sizes(len(plan), args.tile_batch)
    say(f"# {torch.cuda.get_device_name(0)}; model {args.size}, {args.classes} classes, image {H}x{Wd}, tile {tile[0]}x{tile[1]}, overlap "
        f"{args.overlap}: {G.n_crops(plan)} crops + {len(plan) - G.n_crops(plan)} overview, steps {steps}, K = {args.k}")

    kw_t = dict(tile=tile, overlap=args.overlap, tile_batch=args.tile_batch, edge_margin=args.edge_margin)

    def leg_a():
        stats = {}
        s = model.predict_tiled(img, stats=stats, **kw_t)
        return s.pred_instances, stats

    def leg_b():
        return R.user_route(model, img, tile, args.overlap, True, args.tile_batch, args.edge_margin, args.classes, witness=False), None

    # (c): tiles on the device already, the same pipelined steps, nothing else
    total = sum(b for _, b in steps)
    padded = G.pad_plan(plan, total)
    tiles_np = R.cut(img, padded, tile)
    canvas, _ = R.pipeline_canvas(img, tile)
    tiles_dev = torch.from_numpy(tiles_np).cuda()
    k_ov = int(np.nonzero(padded["kind"] == G.OVERVIEW)[0][0])
    tiles_dev[k_ov] = canvas.flip(-1)                        # the pipeline's canvas is BGR
    og = G.overview_geometry(H, Wd, tile)
    meta = torch.from_numpy(G.tile_meta(padded, tile, og["meta"])).cuda()
    step_kw = model._step_kw()

    def leg_c():
        lo = 0
        res = tower = None
        for _, b in steps:
            tower = model._h.tower(b, tile[0], tile[1])
            model._h.calibrate_first(tower, tiles_dev[lo:lo + b])
            res = tower.detect(tiles_dev[lo:lo + b], bank, meta[lo:lo + b], overlap_post=True, **step_kw)
            lo += b
        tower.wait_post()
        return res["count"].tolist(), None

    with torch.no_grad():
        for fn in (leg_a, leg_b, leg_c, leg_a, leg_b, leg_c):       # warm every tower shape, every buffer, every table
            fn()
        a0, st = leg_a()
        b0, _ = leg_b()
        n = b0["count"]
        same = (len(a0.scores) == n and torch.equal(a0.bboxes, torch.from_numpy(b0["boxes"][:n]))
                and torch.equal(a0.scores, torch.from_numpy(b0["scores"][:n]))
                and torch.equal(a0.labels, torch.from_numpy(b0["labels"][:n]).to(torch.int64)))
        say(f"(a) and (b) return the same {n} rows: {same}; predict_tiled stats {st}")
        per = {"a": [], "b": [], "c": []}
        for r in range(args.k):
            for name, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                per[name].append((time.perf_counter() - t) * 1e3)
    A, B, C = (np.asarray(per[k]) for k in "abc")
    desc = {"a": "predict_tiled", "b": "host crops + predict + numpy merge", "c": "floor: pipelined steps only"}
    for name, v in (("a", A), ("b", B), ("c", C)):
        say(f"({name}) {desc[name]:36s}: mean {v.mean():8.2f} ms  median {np.median(v):8.2f}  min {v.min():8.2f}  max {v.max():8.2f}  "
            f"std {v.std():6.2f}  ({1e3 / v.mean():.2f} images/s, {len(plan) * 1e3 / v.mean():.0f} tiles/s)")
    noise = max(A.std(), B.std())
    say(f"(a) - (c) = {A.mean() - C.mean():.2f} ms (median {np.median(A) - np.median(C):.2f}): upload + cut + stacking copies + merge + download")
    say(f"(b) - (a) = {B.mean() - A.mean():.2f} ms; leg-to-leg noise of this run (larger std of the two legs) {noise:.2f} ms; "
        f"(a) <= (b) beyond the noise: {bool(A.mean() <= B.mean() + noise)}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if (same and A.mean() <= B.mean() + noise) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
