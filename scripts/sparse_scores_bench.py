"""Sparse scores (``sparse_scores=True``) beside the default multi-label step and the single-label step, in one process.

    python scripts/sparse_scores_bench.py [--size base] [--batch 32] [--hw 640] [--classes 1203,13204] [--cap 65536] [--k 10] [--kernel-k 20]

Synthetic weights, seeded images and banks, an fp16x3 tower calibrated once.  The weights are synthetic, so the score distribution
says nothing about real data: per bank size the threshold is CHOSEN from the dense step's own scores — the largest, over the
images, of the (cap / 2)-th largest score of an image, so that every image holds at most cap / 2 candidates and none overflows —
and written down; the evaluation threshold 0.001 is reported as it falls (candidates seen, share of images that overflowed).

  steps    K rounds of three in-line steps ALTERNATELY (a, b, c, a, b, c, ...) at the chosen threshold, each timed by the wall clock
           around a full drain: (a) ``ImageTower.detect`` as it is by default — the score tensor [B, N, K], top-k over B x N x K
           candidates; (b) ``detect(sparse_scores=True)``; (c) ``detect(best_class=True)``, the floor.
  kernels  on the SAME operands (the step's own split embeddings and split bank), ALTERNATELY, each between two device events:
           ``wd_similarity_split`` + ``wd_topk_candidates`` and (memset of the counters +) ``wd_sparse_similarity_split`` +
           ``wd_sparse_select``.

Reported: mean / median / min / max / std per leg, the ratios, and the run-to-run noise of the same run (the largest std of the
legs) the ratios are to be read against; per threshold the candidates seen per image (min / median / max) and the share of images
that overflowed.  Checked before timing: the sparse step's kept rows equal the dense step's on the unfolded head.  Prints everything
and writes profiles/sparse_scores.txt.
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
    ap.add_argument("--hw", type=int, default=640)
    ap.add_argument("--classes", default="1203,13204")
    ap.add_argument("--cap", type=int, default=65536, help="sparse_cap: list entries per image")
    ap.add_argument("--k", type=int, default=10, help="rounds of the alternating steps")
    ap.add_argument("--kernel-k", type=int, default=20, help="rounds of the alternating kernel launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_scores.txt"))
    args = ap.parse_args(argv)

    import torch
    from wedetect_amd import lib as L
    from wedetect_amd import sparse as SP
    from wedetect_amd import weights as W
    from wedetect_amd.engine import EMBED_DIM, ImageTower
    from wedetect_amd.pack import pack

    assert torch.cuda.is_available(), "a measurement needs the device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, hw, cap = args.batch, args.hw, args.cap
    tower = ImageTower(args.size, pack(W.make_state_dict(args.size), args.size), B, hw, hw, max_classes=80, precision="fp16x3")
    x = torch.from_numpy(W.make_images(B, hw, hw)).cuda()
    meta = tower.identity_meta()
    meta[:, 7] = 1.0                                         # the mmdet order: rescale before NMS
    tower.calibrate(x)
    rows, n = B * tower.ntot, tower.ntot
    say(f"# {torch.cuda.get_device_name(0)}; model {args.size}, batch {B} x {hw} x {hw} ({rows} region rows), fp16x3, sparse_cap {cap}, "
        f"steps K = {args.k}, kernels K = {args.kernel_k}")
    base_kw = dict(normalize_text=True, iou_thr=0.7, with_embed=False, nms="mmcv")
    stat = lambda v: f"mean {v.mean():9.3f} ms  median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}  std {v.std():7.3f}"
    seen_line = lambda r: (lambda s, st: f"candidates seen per image min {int(s.min())} / median {int(np.median(s))} / max {int(s.max())}; "
                           f"images overflowed {float((st == 1).mean()):.2%}")(r["sparse_seen"].cpu().numpy(), r["sparse_status"].cpu().numpy())
    ok = True
    for k_cls in (int(v) for v in args.classes.split(",")):
        bank = torch.from_numpy(W.make_text_bank(k_cls)).cuda()
        say(f"## K = {k_cls}: score tensor {rows * k_cls * 4 / 2 ** 30:.2f} GiB, lists {B * cap * 8 / 2 ** 20:.1f} MiB")
        # ---- the threshold, from the dense scores of this very batch (the unfolded head both legs' candidates come from)
        fold = tower.fold_text
        tower.fold_text = False
        tower.features(x, num_classes=k_cls)
        dense = tower.similarity(bank, normalize=True).view(B, -1)
        thr = max(float(torch.topk(dense[b], cap // 2, sorted=True).values[-1]) for b in range(B))
        per_img = (dense > thr).sum(dim=1)
        say(f"threshold chosen from the dense scores: {thr:.9g} (max over images of the {cap // 2}-th largest score); "
            f"candidates per image min {int(per_img.min())} / max {int(per_img.max())}")
        kw = dict(score_thr=thr, **base_kw)
        ref = {k_: v.clone() for k_, v in tower.detect(x, bank, meta, **kw).items()}
        got = tower.detect(x, bank, meta, sparse_scores=True, sparse_cap=cap, **kw)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(got[k_], ref[k_])) for k_ in ref)
        ok &= same
        say(f"sparse step equals the dense step on the unfolded head (bboxes, scores, labels, anchors, count): {same}")
        say(f"at {thr:.6g}: {seen_line(got)}")
        r001 = tower.detect(x, bank, meta, sparse_scores=True, sparse_cap=cap, score_thr=0.001, **base_kw)
        torch.cuda.synchronize()
        say(f"at 0.001 (the evaluation threshold, as it falls on synthetic weights): {seen_line(r001)}")
        tower.fold_text = fold
        del dense, per_img
        legs = {"a multi-label (default)": lambda: tower.detect(x, bank, meta, **kw),
                "b sparse_scores": lambda: tower.detect(x, bank, meta, sparse_scores=True, sparse_cap=cap, **kw),
                "c best_class": lambda: tower.detect(x, bank, meta, best_class=True, **kw)}
        for _ in range(2):                                   # warm every buffer, the fold, the split bank
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        per = {name: [] for name in legs}
        kept = {}
        for _ in range(args.k):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                per[name].append((time.perf_counter() - t0) * 1e3)
                kept[name] = int(r["count"].sum())
        v = {name: np.asarray(t) for name, t in per.items()}
        for name in legs:
            say(f"step {name:<24}: {stat(v[name])}  ({B * 1e3 / v[name].mean():.0f} images/s, {kept[name]} rows kept)")
        a, b_, c = (v[name] for name in legs)
        noise = max(t.std() for t in v.values())
        say(f"step ratio b / a = {b_.mean() / a.mean():.3f} (medians {np.median(b_) / np.median(a):.3f}), c / a = {c.mean() / a.mean():.3f}; "
            f"noise of this run (largest std of the legs) {noise:.3f} ms; b faster than a beyond the noise: {bool(b_.mean() + noise < a.mean())}; "
            f"b not slower than a beyond the noise: {bool(b_.mean() <= a.mean() + noise)}")
        say(f"sparse_overflows {tower.sparse_overflows}, sparse_declined {tower.sparse_declined}")
        # ---- the launches on the step's own operands
        tower.detect(x, bank, meta, sparse_scores=True, sparse_cap=cap, **kw)      # leaves embed_s of this batch and the split bank
        torch.cuda.synchronize()
        ts = tower._split_text(bank, True)
        unscale = ts[1] / tower.sscale.get("embed", 1.0)
        seg = (n, tower.off[1], tower.off[2], tower.lvl_scale, tower.lvl_bias)
        if k_cls > tower.max_classes:
            tower._alloc_post(k_cls)
        out = tower.scores.view(-1)[: rows * k_cls].view(rows, k_cls)
        lst, state, status = tower._sparse_list, tower._sparse_state, tower._sparse_status
        lcap = lst.shape[1]
        thr32 = float(np.float32(thr))

        def materialising():
            L.similarity_split(tower.embed_s, rows, ts[0], unscale, out, k_cls, EMBED_DIM, k_cls, seg=seg, sigmoid=True)
            L.topk_candidates(out, B, n * k_cls, thr32, tower.nms_pre, tower.cand_idx, tower.cand_score, tower.cand_count, tower.topk_ws)

        def fused():
            state.zero_()
            SP.sparse_similarity_split(tower.embed_s, rows, ts[0], unscale, k_cls, EMBED_DIM, n, k_cls, thr32, lst, lcap, state, seg=seg)
            SP.sparse_select(lst, lcap, state, B, tower.nms_pre, tower.cand_idx, tower.cand_score, tower.cand_count, status)

        materialising()
        want = [t.clone() for t in (tower.cand_idx, tower.cand_score, tower.cand_count)]
        fused()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(p, q)) for p, q in zip(want, (tower.cand_idx, tower.cand_score, tower.cand_count)))
        ok &= same
        say(f"fused + select candidates equal wd_similarity_split + wd_topk_candidates: {same}")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kt = {"materialising": [], "fused": []}
        for _ in range(args.kernel_k):
            for name, fn in (("materialising", materialising), ("fused", fused)):
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                kt[name].append(ev[0].elapsed_time(ev[1]))
        m, f = np.asarray(kt["materialising"]), np.asarray(kt["fused"])
        say(f"kernels wd_similarity_split + wd_topk_candidates      : {stat(m)}")
        say(f"kernels wd_sparse_similarity_split + wd_sparse_select : {stat(f)}  (with the memset of the counters)")
        say(f"kernel ratio sparse / dense = {f.mean() / m.mean():.3f} (medians {np.median(f) / np.median(m):.3f}); noise of this run "
            f"{max(m.std(), f.std()):.3f} ms")
        del bank, out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
