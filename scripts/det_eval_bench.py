"""Times the device box-mAP evaluation (wedetect_amd.det_eval) end to end — host preparation of the pair layout,
the match / sort / accumulate kernels, the copies back and the numpy summarize — on seeded synthetic sets:

    coco  5 000 images, 80 classes, ~7 gts and 300 dets per image (COCO val2017 size)
    lvis  4 809 images, 1 203 classes, ~50 k gts, 300 dets per image (LVIS minival size)

    python scripts/det_eval_bench.py [--sets coco lvis] [--reps 5] [--ref-images N]

Each set: one warm-up call, then ``--reps`` timed calls, each bracketed by HIP events on the current stream (the
events see the host preparation as idle stream time, so the interval is the wall-clock cost of the call).  With
``--ref-images N`` the float64 numpy restatement (tests/det_eval_ref.py: the libraries' loops in Python, single
thread) is also timed on the first N images of the COCO-size set, as HOST-side context: it is not a measurement
of pycocotools itself.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_set(seed, n_img, n_cat, gts_mean, dets_per_img, lvis):
    rng = np.random.default_rng(seed)
    img_ids = rng.permutation(n_img * 3)[:n_img] + 1
    cat_ids = rng.permutation(n_cat * 2)[:n_cat] + 1
    images, anns, dets = [], [], []
    for i in img_ids:
        ng = int(rng.poisson(gts_mean))
        gc = cat_ids[rng.integers(0, n_cat, ng)]
        xy = rng.uniform(0, 560, (ng, 2))
        wh = rng.uniform(4, 220, (ng, 2))
        for c, p, s in zip(gc, xy, wh):
            a = dict(id=len(anns) + 1, image_id=int(i), category_id=int(c), bbox=[*p.tolist(), *s.tolist()],
                     area=float(s[0] * s[1]))
            if not lvis:
                a["iscrowd"] = int(rng.random() < 0.01)
            anns.append(a)
        im = dict(id=int(i), file_name=f"{int(i):012d}.jpg")
        if lvis:
            present = set(gc.tolist())
            im["neg_category_ids"] = [int(c) for c in cat_ids[rng.integers(0, n_cat, 8)] if int(c) not in present]
            im["not_exhaustive_category_ids"] = [c for c in present if rng.random() < 0.1]
        images.append(im)
        near = int(dets_per_img * 0.7) if ng else 0
        src = rng.integers(0, max(ng, 1), near)
        b_near = np.concatenate([xy[src], xy[src] + wh[src]], 1) + rng.normal(0, 6, (near, 4)) if ng else np.zeros((0, 4))
        c_near = gc[src] if ng else np.zeros(0, np.int64)
        far = dets_per_img - near
        p = rng.uniform(0, 560, (far, 2))
        b_far = np.concatenate([p, p + rng.uniform(4, 220, (far, 2))], 1)
        c_far = cat_ids[rng.integers(0, n_cat, far)]
        dets.append(dict(image_id=int(i), bboxes=np.concatenate([b_near, b_far]).astype(np.float32),
                         scores=rng.random(dets_per_img).astype(np.float32),
                         category_ids=np.concatenate([c_near, c_far]).astype(np.int64)))
    cats = [dict(id=int(c), name=f"c{int(c)}", frequency="rcf"[k % 3]) for k, c in enumerate(cat_ids)]
    return dict(images=images, annotations=anns, categories=cats), dets


SETS = {"coco": dict(seed=1, n_img=5000, n_cat=80, gts_mean=7.3, dets_per_img=300, lvis=False),
        "lvis": dict(seed=2, n_img=4809, n_cat=1203, gts_mean=10.4, dets_per_img=300, lvis=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["coco", "lvis"], choices=sorted(SETS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-images", type=int, default=0)
    args = ap.parse_args()
    import torch
    from wedetect_amd import det_eval
    torch.cuda.set_device(0)
    for name in args.sets:
        ann, dets = make_set(**SETS[name])
        fn = det_eval.lvis_evaluate if SETS[name]["lvis"] else det_eval.coco_evaluate
        fn(ann, dets)                                            # warm-up (module loads, first launches)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ev = fn(ann, dets)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(json.dumps(dict(set=name, images=len(ann["images"]), categories=len(ann["categories"]),
                              gts=len(ann["annotations"]), dets=int(sum(len(d["scores"]) for d in dets)),
                              device_eval_ms_median=round(float(np.median(ms)), 1), device_eval_ms=[round(m, 1) for m in ms],
                              AP=round(float(ev["stats"][0]), 4))), flush=True)
    if args.ref_images:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import det_eval_ref as R
        ann, dets = make_set(**SETS["coco"])
        keep = {im["id"] for im in ann["images"][:args.ref_images]}
        ann = dict(ann, images=ann["images"][:args.ref_images], annotations=[a for a in ann["annotations"] if a["image_id"] in keep])
        dets = [d for d in dets if d["image_id"] in keep]
        t0 = time.perf_counter()
        ref = R.coco_eval(ann, dets)
        t_ref = time.perf_counter() - t0
        t0 = time.perf_counter()
        ev = det_eval.coco_evaluate(ann, dets)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        same = all(np.array_equal(ev[k], ref[k]) for k in ("precision", "recall", "scores", "stats"))
        print(json.dumps(dict(set=f"coco[:{args.ref_images}]", host_numpy_restatement_s=round(t_ref, 2),
                              device_eval_s=round(t_dev, 3), equal=same,
                              note="host-side context: the float64 restatement in Python, one thread")), flush=True)


if __name__ == "__main__":
    main()
