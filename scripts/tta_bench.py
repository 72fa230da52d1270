"""Flip test-time augmentation of one batch, three ways, in one process.

    python scripts/tta_bench.py [--size base] [--batch 32] [--k 20] [--classes 80]

A batch of seeded 427 x 641 images (smooth content plus a little noise) through the test pipeline's letter step (640 x 640
canvases on the device, and a host copy of them), the detector with synthetic weights and an 80-class bank, every leg warmed,
then K rounds of the three legs ALTERNATELY (a, b, c, a, b, c, ...), each timed by the wall clock around a full drain:

  (a) the device flip of the batch (``wd_flip_u8``, one launch) + ``YOLOWorldDetector.predict_views``: one pipelined step per
      view, one merge, one download;
  (b) the route on the plain API: the flipped view made on the host (``np.flip`` of the host canvases) and uploaded,
      ``predict`` per view — which reads the counts back after every step — every view's rows downloaded, the un-flip and the
      merge in numpy (tests/views_ref.py on oracle.postprocess.mmcv_batched_nms);
  (c) the floor: two bare pipelined steps on views that are already on the device — no flip, no merge; one read of the last
      step's counts ends it.

Reported: the three legs (mean, median, min, max, std), (a) - (c) = what the flip, the stacking copies, the merge and the
download cost, and whether (a) <= (b) beyond the leg-to-leg noise of this run (the larger of the two spreads).  Also checked:
(a) and (b) return the same rows.  Prints everything and writes profiles/tta.txt.
"""
import argparse
import os
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
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--hw", default="427,641")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta.txt"))
    args = ap.parse_args(argv)

    import torch
    from scripts.tiled_bench import make_image
    from tests import views_ref as R
    from wedetect_amd import views as VW
    from wedetect_amd import weights as W
    from wedetect_amd.detector import YOLOWorldDetector
    from wedetect_amd.pipeline import Compose
    from wedetect_amd.tta import DEFAULT_TTA_MODEL

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    H, Wd = (int(v) for v in args.hw.split(","))
    B = args.batch
    names = [f"class {k}" for k in range(args.classes)]
    model = YOLOWorldDetector(args.size, max_classes=args.classes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict(args.size).items()})
    model.cuda().eval()
    bank = torch.from_numpy(W.make_text_bank(args.classes)).cuda()
    model.set_text_embeddings(bank, [[n] for n in names])
    hh, ww = model.img_scale
    tta_cfg = DEFAULT_TTA_MODEL["tta_cfg"]
    keys = ("img_id", "ori_shape", "img_shape", "scale_factor", "pad_param", "flip", "flip_direction")
    pipe = Compose([dict(type="LoadImageFromFile"), dict(type="WeDetectKeepRatioResize", scale=(ww, hh)),
                    dict(type="WeDetectLetterResize", scale=(ww, hh), allow_scale_up=False, pad_val=dict(img=114)),
                    dict(type="RandomFlip", prob=0.0), dict(type="PackDetInputs", meta_keys=keys)])
    items = [pipe(dict(img=np.ascontiguousarray(make_image(H, Wd, seed=100 + i)[:, :, ::-1]), img_id=i)) for i in range(B)]
    plain_hwc = torch.stack([it["inputs"].permute(1, 2, 0) for it in items]).contiguous()      # [B, H, W, 3] BGR, device
    plain_host = plain_hwc.cpu().numpy()
    s_plain = [it["data_samples"] for it in items]
    s_flip = [type(s)(metainfo=s.metainfo) for s in s_plain]
    for s in s_flip:
        s.set_metainfo(dict(flip=True, flip_direction="horizontal"))
    flipped_hwc = torch.empty_like(plain_hwc)
    say(f"# {torch.cuda.get_device_name(0)}; model {args.size}, {args.classes} classes, batch {B} of {H}x{Wd} images on {hh}x{ww} canvases, "
        f"views: horizontal flip + plain, merge NMS {tta_cfg['nms']['iou_threshold']}, {tta_cfg['max_per_img']} per image, K = {args.k}")

    fresh = lambda samples: [type(s)(metainfo=s.metainfo) for s in samples]
    chw = lambda t: t.permute(0, 3, 1, 2)

    def leg_a():
        VW.flip_u8(plain_hwc, flipped_hwc, "horizontal")
        stats = {}
        out = model.predict_views([(chw(flipped_hwc), fresh(s_flip)), (chw(plain_hwc), fresh(s_plain))], tta_cfg, stats=stats)
        return out, stats

    def leg_b():
        flipped = torch.from_numpy(np.ascontiguousarray(plain_host[:, :, ::-1]))
        return R.user_route(model, [(chw(flipped), fresh(s_flip)), (chw(plain_hwc), fresh(s_plain))], tta_cfg, witness=False), None

    rgb = [flipped_hwc.flip(-1).contiguous(), plain_hwc.flip(-1).contiguous()]                 # the tower reads RGB
    from wedetect_amd.detector import letterbox_meta
    meta = torch.tensor([letterbox_meta(s.metainfo, hh, ww, True) for s in s_plain], dtype=torch.float32).cuda()
    step_kw = model._step_kw()

    def leg_c():
        tower = model._h.tower(B, hh, ww)
        res = None
        for x in rgb:
            model._h.calibrate_first(tower, x)
            res = tower.detect(x, bank, meta, overlap_post=True, **step_kw)
        tower.wait_post()
        return res["count"].tolist(), None

    with torch.no_grad():
        VW.flip_u8(plain_hwc, flipped_hwc, "horizontal")
        rgb[0] = flipped_hwc.flip(-1).contiguous()
        for fn in (leg_a, leg_b, leg_c, leg_a, leg_b, leg_c):       # warm the tower, every buffer, every table
            fn()
        a0, st = leg_a()
        b0, _ = leg_b()
        same = all(len(s.pred_instances.scores) == int(b0["count"][i])
                   and torch.equal(s.pred_instances.bboxes, torch.from_numpy(b0["boxes"][i, :b0["count"][i]]))
                   and torch.equal(s.pred_instances.scores, torch.from_numpy(b0["scores"][i, :b0["count"][i]]))
                   and torch.equal(s.pred_instances.labels, torch.from_numpy(b0["labels"][i, :b0["count"][i]]).to(torch.int64))
                   for i, s in enumerate(a0))
        say(f"(a) and (b) return the same rows ({int(b0['count'].sum())} over the batch; rows per view going in "
            f"{b0['per_view_in'].sum(1).tolist()}): {same}; predict_views stats {st}")
        per = {"a": [], "b": [], "c": []}
        for r in range(args.k):
            for name, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                per[name].append((time.perf_counter() - t) * 1e3)
    A, Bm, C = (np.asarray(per[k]) for k in "abc")
    desc = {"a": "device flip + predict_views", "b": "host flip + predict per view + numpy merge", "c": "floor: two pipelined steps only"}
    for name, v in (("a", A), ("b", Bm), ("c", C)):
        say(f"({name}) {desc[name]:44s}: mean {v.mean():8.2f} ms  median {np.median(v):8.2f}  min {v.min():8.2f}  max {v.max():8.2f}  "
            f"std {v.std():6.2f}  ({B * 1e3 / v.mean():.0f} images/s)")
    noise = max(A.std(), Bm.std())
    say(f"(a) - (c) = {A.mean() - C.mean():.2f} ms (median {np.median(A) - np.median(C):.2f}): flip + input repack + stacking copies + merge + download")
    say(f"(b) - (a) = {Bm.mean() - A.mean():.2f} ms; leg-to-leg noise of this run (larger std of the two legs) {noise:.2f} ms; "
        f"(a) <= (b) beyond the noise: {bool(A.mean() <= Bm.mean() + noise)}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if (same and A.mean() <= Bm.mean() + noise) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
