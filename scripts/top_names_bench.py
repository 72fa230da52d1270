"""The n best names per box (``best_class=True, top_names=n``) beside the best-class and the dense multi-label step, in one process.

    python scripts/top_names_bench.py [--size base] [--batch 32] [--hw 640] [--classes 1203,13204] [--k 10] [--kernel-k 30]
                                      [--bank-rows 1000000]

Synthetic weights, seeded images and banks, an fp16x3 tower calibrated once.  Per bank size:

  steps    K rounds of three in-line steps ALTERNATELY, each timed by the wall clock around a full drain: (a) ``ImageTower.detect`` as
           it is by default — the only route to a second name there was: the score tensor [B, N, K]; (b) ``detect(best_class=True)``;
           (c) ``detect(best_class=True, top_names=5)``.
  kernels  (d) ``wd_best_similarity_split`` against ``wd_topn_similarity_split`` with n = 1, 5, 8 on the SAME operands (the step's own
           split embeddings and split bank), ALTERNATELY, each between two device events, the clearing memset of the keys included.
  regions  (e) ``parallel.RegionNamer`` (n = 5) against ``parallel.BankScorer`` on 32 x 300 regions and a bank of --bank-rows rows
           (0 skips the leg).

Reported: mean / median / min / max / std per leg, the ratios (c)/(a), (c)/(b), the kernel ratios against the best-class kernel and
the (e) ratio, with the run-to-run noise (the larger std of the legs compared) they are to be read against.  Checked before timing:
the n = 1 keys equal the best-class keys and slot 0 of every n equals them.  Prints everything and writes profiles/top_names.txt.
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
    ap.add_argument("--bank-rows", type=int, default=1000000, help="rows of the bank of leg (e); 0 skips it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_names.txt"))
    args = ap.parse_args(argv)

    import torch
    from wedetect_amd import best as BS
    from wedetect_amd import parallel as P
    from wedetect_amd import topn as TN
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
        legs = {"a dense": lambda: tower.detect(x, bank, meta, **kw),
                "b best": lambda: tower.detect(x, bank, meta, best_class=True, **kw),
                "c top5": lambda: tower.detect(x, bank, meta, best_class=True, top_names=5, **kw)}
        for _ in range(2):                                   # warm every buffer, the fold, the split bank
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
        a, b, c = (np.asarray(per[n]) for n in legs)
        say(f"## K = {k_cls}: score tensor {rows * k_cls * 4 / 2 ** 30:.2f} GiB, keys (n = 5) {rows * 40 / 2 ** 20:.2f} MiB")
        say(f"step (a) dense multi-label        : {stat(a)}")
        say(f"step (b) best_class               : {stat(b)}")
        say(f"step (c) best_class + top_names=5 : {stat(c)}")
        noise = max(a.std(), c.std())
        say(f"step ratio (c)/(a) = {np.median(c) / np.median(a):.3f} of medians, (c)/(b) = {np.median(c) / np.median(b):.3f}; noise of this run "
            f"(larger std of (a), (c)) {noise:.3f} ms; (c) beats (a) beyond the noise: {bool(np.median(c) + noise < np.median(a))}")
        # ---- (d) the launches on the step's own operands
        tower.detect(x, bank, meta, best_class=True, **kw)   # leaves embed_s of this batch and the split bank
        torch.cuda.synchronize()
        ts = tower._split_text(bank, True)
        unscale = ts[1] / tower.sscale.get("embed", 1.0)
        seg = (tower.ntot, tower.off[1], tower.off[2], tower.lvl_scale, tower.lvl_bias)
        kbest = torch.zeros(rows, dtype=torch.int64, device="cuda")
        keys = {n: torch.zeros(rows, n, dtype=torch.int64, device="cuda") for n in (1, 5, 8)}

        def best():
            kbest.zero_()
            BS.best_similarity_split(tower.embed_s, rows, ts[0], unscale, k_cls, EMBED_DIM, kbest, 0, seg=seg)

        def topn(n):
            keys[n].zero_()
            TN.topn_similarity_split(tower.embed_s, rows, ts[0], unscale, k_cls, EMBED_DIM, n, keys[n], 0, seg=seg)

        kernels = [("best", best)] + [(f"top{n}", (lambda n=n: topn(n))) for n in keys]
        for _, fn in kernels:
            fn()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(keys[n][:, 0], kbest)) for n in keys)
        ok &= same
        say(f"slot 0 of n = 1, 5, 8 equals the best-class keys: {same}")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kt = {n: [] for n, _ in kernels}
        for _ in range(args.kernel_k):
            for n, fn in kernels:
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                kt[n].append(ev[0].elapsed_time(ev[1]))
        kt = {n: np.asarray(v) for n, v in kt.items()}
        say(f"kernel wd_best_similarity_split        : {stat(kt['best'])}  (with the memset of the keys)")
        for n in keys:
            v = kt[f"top{n}"]
            say(f"kernel wd_topn_similarity_split n = {n}  : {stat(v)}  ratio to best {np.median(v) / np.median(kt['best']):.3f} "
                f"(noise {max(v.std(), kt['best'].std()):.3f} ms)")
        del bank, keys, kbest
    # ---- (e) regions against a large bank
    if args.bank_rows > 0:
        n_img, r = 32, 300
        g = torch.Generator(device="cuda").manual_seed(7)
        big = torch.nn.functional.normalize(torch.randn(args.bank_rows, EMBED_DIM, device="cuda", generator=g), dim=-1)
        e = torch.randn(n_img, r, EMBED_DIM, device="cuda", generator=g) * 0.8
        scales = torch.rand(n_img, r, device="cuda", generator=g) + 1.0
        bias = torch.rand(n_img, r, device="cuda", generator=g) * 2 - 3
        count = torch.full((n_img,), r, dtype=torch.int32, device="cuda")
        scorer, namer = P.BankScorer(big), P.RegionNamer(big, 5)
        out = torch.empty(n_img, args.bank_rows, device="cuda")
        legs = {"scorer": lambda: scorer(e, count, scales, bias, out=out), "namer": lambda: namer(e, count, scales, bias)}
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
        s_, n_ = np.asarray(per["scorer"]), np.asarray(per["namer"])
        say(f"## (e) {n_img} x {r} regions against {args.bank_rows} names (one host read of the range flag per call in both legs)")
        say(f"BankScorer (max over regions)     : {stat(s_)}")
        say(f"RegionNamer n = 5                 : {stat(n_)}")
        say(f"ratio namer / scorer = {np.median(n_) / np.median(s_):.3f} of medians; noise {max(s_.std(), n_.std()):.3f} ms")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
