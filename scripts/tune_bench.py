"""Bank tuning (``wedetect_amd.tune.BankTuner``) beside the same optimisation step in torch, in one process.

    python scripts/tune_bench.py [--size base] [--batch 32] [--hw 640] [--classes 80,1203] [--boxes 16] [--k 20]

Synthetic weights and seeded images, an fp16x3 tower calibrated once; the labelled boxes are decoded boxes of the batch itself,
pushed by a few pixels, with random classes.  One cached chunk of batch x anchors rows.  Per class count, K rounds of the legs
ALTERNATELY, each timed by the wall clock around a full drain:

  fused   one optimisation step: ``wd_tune_grad`` on the chunk + ``wd_tune_update`` (the [rows, K] matrix is never written)
  torch   the same step in torch on the same device: T = W / |W|, logits [rows, K] = a * (E @ T^T) + b materialised under
          autograd, binary_cross_entropy_with_logits against a dense target matrix built beforehand, backward, torch.optim.Adam

and, between device events, ALTERNATELY: ``wd_tune_grad`` alone (its FLOPs 4 * rows * K_pad * 768 over its time against the
fp32-input MFMA peak of 157.3 TFLOP/s) and ``wd_tune_update`` alone.  Then ``BankTuner.add_batch`` against ``features()`` alone,
alternately.  Checked before timing: the first step's dW of the two formulations agrees.  Recorded, not asserted: prints everything
and writes profiles/tune.txt.
"""
import argparse
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_MFMA_PEAK = 157.3e12


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="base")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=640)
    ap.add_argument("--classes", default="80,1203")
    ap.add_argument("--boxes", type=int, default=16, help="labelled boxes per image")
    ap.add_argument("--m", type=int, default=4, help="anchors per labelled box")
    ap.add_argument("--k", type=int, default=20, help="rounds of the alternating legs")
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tune.txt"))
    args = ap.parse_args(argv)

    import torch
    import torch.nn.functional as F
    from wedetect_amd import tune as TN
    from wedetect_amd import weights as W
    from wedetect_amd.engine import ImageTower
    from wedetect_amd.pack import pack

    assert torch.cuda.is_available(), "a measurement needs the device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, hw, E, m = args.batch, args.hw, args.boxes, args.m
    tower = ImageTower(args.size, pack(W.make_state_dict(args.size), args.size), B, hw, hw, max_classes=80, precision="fp16x3")
    x = torch.from_numpy(W.make_images(B, hw, hw)).cuda()
    meta = tower.identity_meta()
    meta[:, 7] = 1.0
    tower.calibrate(x)
    _, boxes = tower.features(x)
    g = torch.Generator().manual_seed(5)
    pick = torch.randint(0, tower.ntot, (B, E), generator=g).cuda()
    gt_boxes = (torch.gather(boxes, 1, pick[:, :, None].expand(B, E, 4)) + torch.tensor([-3.0, -2.0, 2.0, 3.0], device="cuda")).contiguous()
    gt_count = torch.full((B,), E, dtype=torch.int32, device="cuda")
    stat = lambda v: f"mean {v.mean():9.3f} ms  median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}  std {v.std():7.3f}"
    say(f"# {torch.cuda.get_device_name(0)} on {platform.node()}; model {args.size}, batch {B} x {hw} x {hw} ({tower.ntot} anchors per image, "
        f"{B * tower.ntot} rows, {B * tower.ntot * 3072 / 1e6:.0f} MB of embeddings), fp16x3 tower, {E} boxes per image, m = {m}, K = {args.k} rounds")

    for K in [int(v) for v in args.classes.split(",")]:
        gt_cls = torch.randint(0, K, (B, E), generator=g).to(torch.int32).cuda()
        tuner = TN.BankTuner(tower)
        c = tuner.add_batch(x, meta, gt_boxes, gt_count, gt_cls, m, 0.1)
        rows, kp = c["rows"], TN.k_pad(K)
        bank0 = torch.from_numpy(W.make_text_bank(K)).cuda()
        bank0 = bank0 / bank0.norm(dim=1, keepdim=True)
        s = TN.plan(rows, K)
        inv_norm = 1.0 / max(float(c["pos_sum"]), 1.0)
        f32 = dict(dtype=torch.float32, device="cuda")
        w, bank = bank0.clone(), bank0.clone()
        mm, vv = torch.zeros_like(w), torch.zeros_like(w)
        slabs, parts = torch.empty(s, kp, TN.DIM, **f32), torch.empty(s, kp // 32, **f32)
        loss, status = torch.zeros(4096, **f32), torch.zeros(1, dtype=torch.int32, device="cuda")
        tr = torch.ones(K, dtype=torch.uint8, device="cuda")
        step = [0]

        def k_grad():
            TN.tune_grad(c["E"], rows, tower.ntot, tower.off[1], tower.off[2], tower.lvl_scale, tower.lvl_bias, c["pos_cls"], c["pos_y"], bank, K,
                         inv_norm, s, slabs, parts)

        def k_update():
            TN.tune_update(slabs, s, parts, K, w, mm, vv, bank, tr, args.lr, 0.9, 0.999, 1e-8, step[0], loss, status)
            step[0] = (step[0] + 1) % 4096

        def leg_fused():
            k_grad()
            k_update()

        # the torch formulation: dense targets built once, outside the timed step
        lv = ((torch.arange(rows, device="cuda") % tower.ntot >= tower.off[1]).long() + (torch.arange(rows, device="cuda") % tower.ntot >= tower.off[2]).long())
        a_r = torch.tensor(tower.lvl_scale, **f32)[lv][:, None]
        b_r = torch.tensor(tower.lvl_bias, **f32)[lv][:, None]
        y = torch.zeros(rows, K, **f32)
        pc = c["pos_cls"].reshape(-1).long()
        hit = pc >= 0
        y[hit.nonzero().flatten(), pc[hit]] = c["pos_y"].reshape(-1)[hit]
        wt = bank0.clone().requires_grad_(True)
        opt = torch.optim.Adam([wt], lr=args.lr, betas=(0.9, 0.999), eps=1e-8)

        def leg_torch():
            opt.zero_grad(set_to_none=True)
            t = wt / wt.norm(dim=1, keepdim=True)
            z = a_r * (c["E"] @ t.t()) + b_r                                # [rows, K], kept for backward
            l = F.binary_cross_entropy_with_logits(z, y, reduction="sum") * inv_norm
            l.backward()
            opt.step()
            return l

        # the first step of both from the same rows: dW agrees
        leg_fused()
        opt.zero_grad(set_to_none=True)
        t = wt / wt.norm(dim=1, keepdim=True)
        l0 = F.binary_cross_entropy_with_logits(a_r * (c["E"] @ t.t()) + b_r, y, reduction="sum") * inv_norm
        l0.backward()
        torch.cuda.synchronize()
        dw_f, dw_t = mm / (1 - 0.9), wt.grad
        rel = float(((dw_f - dw_t).norm(dim=1) / dw_t.norm(dim=1)).max())
        say(f"## K = {K} (K_pad {kp}, {kp // 32} class blocks x {s} splits = {kp // 32 * s} workgroups); positives {int(hit.sum())}, norm {1 / inv_norm:.2f}")
        say(f"first step: loss fused {float(loss[0]):.6f} torch {float(l0):.6f}; max over classes of |dW fused - dW torch| / |dW torch| {rel:.2e}")
        legs = {"fused": leg_fused, "torch": leg_torch}
        for _ in range(3):
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
        tt = {n: np.asarray(v) for n, v in per.items()}
        say(f"step fused (grad + update)         : {stat(tt['fused'])}")
        say(f"step torch (logits under autograd) : {stat(tt['torch'])}")
        say(f"torch / fused (medians) {np.median(tt['torch']) / np.median(tt['fused']):.2f}; logits the torch step materialises: {rows * K * 4 / 1e6:.0f} MB")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kt = {"grad": [], "update": []}
        for _ in range(max(args.k, 20)):
            for n, fn in (("grad", k_grad), ("update", k_update)):
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                kt[n].append(ev[0].elapsed_time(ev[1]))
        gr, up = np.asarray(kt["grad"]), np.asarray(kt["update"])
        flops = 4.0 * rows * kp * TN.DIM
        say(f"kernel wd_tune_grad   : {stat(gr)}")
        say(f"kernel wd_tune_update : {stat(up)}   ({s} slabs of {kp * TN.DIM * 4 / 1e6:.2f} MB)")
        say(f"wd_tune_grad: {flops / 1e9:.1f} GFLOP (4 * rows * K_pad * 768) in {np.median(gr):.3f} ms = {flops / np.median(gr) / 1e9:.1f} TFLOP/s = "
            f"{100 * flops / (np.median(gr) * 1e-3) / FP32_MFMA_PEAK:.1f} % of the fp32-input MFMA peak ({FP32_MFMA_PEAK / 1e12:.1f} TFLOP/s); E is read "
            f"{2 * kp // 32} times ({2 * kp // 32 * rows * 3072 / 1e9:.2f} GB through L2)")

    # ---- add_batch against features() alone
    gt_cls = torch.randint(0, 80, (B, E), generator=g).to(torch.int32).cuda()
    tuner = TN.BankTuner(tower, max_cache_bytes=1 << 40)

    def leg_add():
        tuner.truncate(0)
        tuner.add_batch(x, meta, gt_boxes, gt_count, gt_cls, m, 0.1)

    legs = {"add_batch": leg_add, "features": lambda: tower.features(x)}
    for _ in range(2):
        for fn in legs.values():
            fn()
    per = {n: [] for n in legs}
    for _ in range(args.k):
        for n, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            per[n].append((time.perf_counter() - t0) * 1e3)
    tt = {n: np.asarray(v) for n, v in per.items()}
    say("## the cache")
    say(f"call BankTuner.add_batch : {stat(tt['add_batch'])}")
    say(f"features alone           : {stat(tt['features'])}")
    say(f"beyond features (medians): {np.median(tt['add_batch']) - np.median(tt['features']):.3f} ms (the clone of {B * tower.ntot * 3072 / 1e6:.0f} MB, "
        f"the assignment, the targets, the sum)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
