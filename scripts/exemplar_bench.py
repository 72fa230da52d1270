"""Exemplar prompts (``ImageTower.exemplar_bank``) beside a torch formulation and beside one ``predict``-like step, in one process.

    python scripts/exemplar_bench.py [--size base] [--batch 8] [--hw 640] [--examples 16] [--m 4] [--k 20]

Synthetic weights and seeded images, an fp16x3 tower calibrated once; the example boxes are decoded boxes of the batch itself, pushed
by a few pixels.  K rounds of the legs ALTERNATELY, each timed by the wall clock around a full drain:

  exemplar  ``ImageTower.exemplar_bank``: features (the head stops at c2) + assign + gather + three embedding GEMMs + pool
  torch     the same result formulated in torch on the same device: features with ``tower.embed`` materialised, broadcast IoU
            [B, E, N], ``topk``, gather, normalise, weighted sum, normalise
  detect    one in-line ``ImageTower.detect`` step of the same batch against an 80-row bank (what ``predict`` runs)
  features  ``ImageTower.features`` alone: what the first two legs share

and the two kernels on the call's own operands, ALTERNATELY, each between two device events.  Checked before timing: the torch
formulation selects the same anchors and its bank agrees within 1e-5.  Recorded, not asserted: prints everything and writes
profiles/exemplar.txt.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="base")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=640)
    ap.add_argument("--examples", type=int, default=16, help="example boxes per image")
    ap.add_argument("--m", type=int, default=4, help="anchors per example box")
    ap.add_argument("--k", type=int, default=20, help="rounds of the alternating legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exemplar.txt"))
    args = ap.parse_args(argv)

    import torch
    import torch.nn.functional as F
    from wedetect_amd import exemplar as EX
    from wedetect_amd import weights as W
    from wedetect_amd.engine import EMBED_DIM, ImageTower
    from wedetect_amd.pack import pack

    assert torch.cuda.is_available(), "a measurement needs the device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, hw, E, m = args.batch, args.hw, args.examples, args.m
    tower = ImageTower(args.size, pack(W.make_state_dict(args.size), args.size), B, hw, hw, max_classes=80, precision="fp16x3")
    x = torch.from_numpy(W.make_images(B, hw, hw)).cuda()
    meta = tower.identity_meta()
    meta[:, 7] = 1.0
    tower.calibrate(x)
    _, boxes = tower.features(x)
    g = torch.Generator().manual_seed(5)
    pick = torch.randint(0, tower.ntot, (B, E), generator=g).cuda()
    ex_boxes = (torch.gather(boxes, 1, pick[:, :, None].expand(B, E, 4)) + torch.tensor([-3.0, -2.0, 2.0, 3.0], device="cuda")).contiguous()
    ex_count = torch.full((B,), E, dtype=torch.int32, device="cuda")
    # class e = example e of every image
    S = E * m
    slots = torch.tensor([[b * S + e * m + j for b in range(B) for j in range(m)] for e in range(E)], dtype=torch.int32)
    cls_off = (torch.arange(E + 1, dtype=torch.int32) * (B * m)).cuda()
    cls_slot = slots.reshape(-1).cuda()
    bank80 = torch.from_numpy(W.make_text_bank(80)).cuda()
    kw = dict(normalize_text=True, score_thr=0.001, iou_thr=0.7, with_embed=False, nms="mmcv")
    min_iou = 0.1

    def leg_exemplar():
        return tower.exemplar_bank(x, meta, ex_boxes, ex_count, cls_off, cls_slot, m, min_iou)

    def leg_torch():
        embed, bx = tower.features(x)                                    # [B, N, 768] materialised by the head
        e = ex_boxes[:, :, None, :]
        n = bx[:, None, :, :]
        area_e = (e[..., 2] - e[..., 0]) * (e[..., 3] - e[..., 1])
        area_n = (n[..., 2] - n[..., 0]) * (n[..., 3] - n[..., 1])
        w = (torch.minimum(e[..., 2], n[..., 2]) - torch.maximum(e[..., 0], n[..., 0])).clamp_min(0)
        h = (torch.minimum(e[..., 3], n[..., 3]) - torch.maximum(e[..., 1], n[..., 1])).clamp_min(0)
        inter = w * h
        iou = inter / (area_e + area_n - inter)                          # [B, E, N]
        iou = torch.where(iou > min_iou, iou, torch.zeros_like(iou))
        top, idx = iou.topk(m, dim=2)                                    # ties: torch's order, not the anchor's
        rows = torch.gather(embed, 1, idx.reshape(B, E * m)[:, :, None].expand(B, E * m, EMBED_DIM)).view(B, E, m, EMBED_DIM)
        acc = (F.normalize(rows, dim=-1) * top[..., None]).sum(dim=(0, 2))
        return F.normalize(acc, dim=-1), idx, top

    legs = {"exemplar": leg_exemplar, "torch": leg_torch, "detect": lambda: tower.detect(x, bank80, meta, **kw),
            "features": lambda: tower.features(x)}
    for _ in range(2):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    res = leg_exemplar()
    bank = res["bank"].clone()
    sel = res["sel_anchors"].view(B, E, m).clone()
    tb, tidx, ttop = leg_torch()
    torch.cuda.synchronize()
    same_sel = bool(torch.equal(torch.where(ttop > 0, tidx, torch.full_like(tidx, -1)).sort(dim=2).values, sel.long().sort(dim=2).values))
    d_bank = float((tb - bank).abs().max())
    say(f"# {torch.cuda.get_device_name(0)} on {platform.node()}; model {args.size}, batch {B} x {hw} x {hw} ({tower.ntot} anchors per image), fp16x3, "
        f"{E} examples per image, m = {m}, {E} classes of {B * m} slots, K = {args.k} rounds")
    say(f"torch formulation: same anchors per example {same_sel}; max |bank - torch| {d_bank:.2e}; support min {int(res['support'].min())}")
    per = {n: [] for n in legs}
    for _ in range(args.k):
        for n, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            per[n].append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: f"mean {v.mean():9.3f} ms  median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}  std {v.std():7.3f}"
    t = {n: np.asarray(v) for n, v in per.items()}
    say(f"call exemplar_bank                 : {stat(t['exemplar'])}")
    say(f"call torch formulation (with embed): {stat(t['torch'])}")
    say(f"step detect, 80 classes            : {stat(t['detect'])}")
    say(f"features alone                     : {stat(t['features'])}")
    say(f"beyond features: exemplar {np.median(t['exemplar']) - np.median(t['features']):.3f} ms, torch "
        f"{np.median(t['torch']) - np.median(t['features']):.3f} ms (medians); exemplar / detect = "
        f"{np.median(t['exemplar']) / np.median(t['detect']):.3f}; noise of this run (largest std) {max(v.std() for v in t.values()):.3f} ms")
    # ---- the two kernels on the call's own operands
    ex = tower._ex
    rows = B * S

    def k_assign():
        EX.exemplar_assign(tower.boxes, tower.ntot, ex_boxes, ex_count, meta, E, B, m, min_iou, ex["sel_anchors"], ex["sel_iou"], ex["sel_count"])

    def k_pool():
        EX.exemplar_pool(ex["t"], EMBED_DIM, tower.off[1], tower.off[2], ex["sel_anchors"], ex["sel_iou"], rows, cls_off, cls_slot, E,
                         ex["bank"], ex["support"])

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kt = {"assign": [], "pool": []}
    for _ in range(max(args.k, 20)):
        for n, fn in (("assign", k_assign), ("pool", k_pool)):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            kt[n].append(ev[0].elapsed_time(ev[1]))
    a, p = np.asarray(kt["assign"]), np.asarray(kt["pool"])
    say(f"kernel wd_exemplar_assign ({E} x {B} workgroups, {tower.ntot} boxes each): {stat(a)}")
    say(f"kernel wd_exemplar_pool   ({E} workgroups, {B * m} rows each)            : {stat(p)}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
