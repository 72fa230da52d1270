"""Single-label detection (``best_class=True``) beside the multi-label step, in one process.

    python scripts/best_class_bench.py [--size base] [--batch 32] [--hw 640] [--classes 1203,13204] [--k 10] [--kernel-k 30]

Synthetic weights, seeded images and banks, an fp16x3 tower calibrated once.  Per bank size:

  steps    K rounds of two in-line steps ALTERNATELY (multi, best, multi, best, ...), each timed by the wall clock around a full
           drain: (multi) ``ImageTower.detect`` as it is by default — the score tensor [B, N, K], top-k over B x N x K candidates,
           class-aware NMS; (best) ``detect(best_class=True, agnostic_nms=True)`` — keys [B x N], top-k over B x N candidates.
  kernels  the two similarity launches on the SAME operands (the step's own split embeddings and split bank), ALTERNATELY,
           each between two device events: ``wd_similarity_split`` into the score tensor and ``wd_best_similarity_split`` into
           the keys (the clearing memset of the keys is timed with it: the step pays it too).

Reported: mean / median / min / max / std per leg, the ratio best / multi of the steps and fused / materialising of the kernels,
and the run-to-run noise of the same run (the larger std of the two legs) the ratios are to be read against.  Checked before
timing: the fused keys equal ``wd_best_rows`` over the materialised scores.  Prints everything and writes profiles/best_class.txt.
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
    ap.add_argument("--k", type=int, default=10, help="rounds of the alternating steps")
    ap.add_argument("--kernel-k", type=int, default=30, help="rounds of the alternating kernel launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_class.txt"))
    args = ap.parse_args(argv)

    import torch
    from wedetect_amd import best as BS
    from wedetect_amd import lib as L
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
    meta[:, 7] = 1.0                                         # the mmdet order: rescale before NMS
    tower.calibrate(x)
    rows = B * tower.ntot
    say(f"# {torch.cuda.get_device_name(0)}; model {args.size}, batch {B} x {hw} x {hw} ({rows} region rows), fp16x3, steps K = {args.k}, "
        f"kernels K = {args.kernel_k}")
    kw = dict(normalize_text=True, score_thr=0.001, iou_thr=0.7, with_embed=False, nms="mmcv")
    stat = lambda v: f"mean {v.mean():9.3f} ms  median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}  std {v.std():7.3f}"
    ok = True
    for k_cls in (int(v) for v in args.classes.split(",")):
        bank = torch.from_numpy(W.make_text_bank(k_cls)).cuda()
        legs = {"multi": lambda: tower.detect(x, bank, meta, **kw),
                "best": lambda: tower.detect(x, bank, meta, best_class=True, agnostic_nms=True, **kw)}
        for _ in range(2):                                   # warm every buffer, the fold, the split bank
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        per = {n: [] for n in legs}
        kept = {}
        for _ in range(args.k):
            for n, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                per[n].append((time.perf_counter() - t0) * 1e3)
                kept[n] = int(r["count"].sum())
        m, b = np.asarray(per["multi"]), np.asarray(per["best"])
        say(f"## K = {k_cls}: score tensor {rows * k_cls * 4 / 2 ** 30:.2f} GiB, keys {rows * 8 / 2 ** 20:.2f} MiB")
        say(f"step multi-label             : {stat(m)}  ({B * 1e3 / m.mean():.0f} images/s, {kept['multi']} rows kept)")
        say(f"step best_class + agnostic   : {stat(b)}  ({B * 1e3 / b.mean():.0f} images/s, {kept['best']} rows kept)")
        say(f"step ratio best / multi = {b.mean() / m.mean():.3f} (medians {np.median(b) / np.median(m):.3f}); noise of this run "
            f"(larger std of the two legs) {max(m.std(), b.std()):.3f} ms")
        # ---- the two similarity launches on the step's own operands
        tower.detect(x, bank, meta, best_class=True, agnostic_nms=True, **kw)      # leaves embed_s of this batch and the split bank
        torch.cuda.synchronize()
        ts = tower._split_text(bank, True)
        unscale = ts[1] / tower.sscale.get("embed", 1.0)
        seg = (tower.ntot, tower.off[1], tower.off[2], tower.lvl_scale, tower.lvl_bias)
        if k_cls > tower.max_classes:
            tower._alloc_post(k_cls)
        out = tower.scores.view(-1)[: rows * k_cls].view(rows, k_cls)
        key, kref = torch.zeros(rows, dtype=torch.int64, device="cuda"), torch.zeros(rows, dtype=torch.int64, device="cuda")

        def materialising():
            L.similarity_split(tower.embed_s, rows, ts[0], unscale, out, k_cls, EMBED_DIM, k_cls, seg=seg, sigmoid=True)

        def fused():
            key.zero_()
            BS.best_similarity_split(tower.embed_s, rows, ts[0], unscale, k_cls, EMBED_DIM, key, 0, seg=seg)

        materialising(); fused()
        BS.best_rows(out, B, tower.ntot, k_cls, k_cls, kref)
        torch.cuda.synchronize()
        same = bool(torch.equal(key, kref))
        ok &= same
        say(f"fused keys equal wd_best_rows over the materialised scores: {same}")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kt = {"materialising": [], "fused": []}
        for _ in range(args.kernel_k):
            for n, fn in (("materialising", materialising), ("fused", fused)):
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                kt[n].append(ev[0].elapsed_time(ev[1]))
        a, f = np.asarray(kt["materialising"]), np.asarray(kt["fused"])
        say(f"kernel wd_similarity_split        : {stat(a)}")
        say(f"kernel wd_best_similarity_split   : {stat(f)}  (with the memset of the keys)")
        noise = max(a.std(), f.std())
        say(f"kernel ratio fused / materialising = {f.mean() / a.mean():.3f} (medians {np.median(f) / np.median(a):.3f}); noise of this run "
            f"{noise:.3f} ms; fused <= materialising beyond the noise: {bool(f.mean() <= a.mean() + noise)}")
        del bank, out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
