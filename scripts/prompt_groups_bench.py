"""Prompt groups (``detect(prompt_groups=plan)``) beside what the dense step offers for the same class lists, in one process.

    python scripts/prompt_groups_bench.py [--size base] [--batch 32] [--hw 640] [--k 10] [--kernel-k 30]

Synthetic weights, seeded images and banks, an fp16x3 tower calibrated once; the plan is the LVIS-en class-text list of
tests/golden (1203 classes, 1983 prompts, 2048 padded rows).  Every step leg runs on the unfolded head (``fold_text`` off).

  steps    K rounds of the legs ALTERNATELY, each timed by the wall clock around a full drain:
           (a) the route without this mode: ``features`` + ``similarity`` over the 2048 padded prompts, the class maximum in torch
               (one ``index_select`` + ``maximum`` per prompt position, ten for this list), ``postprocess``;
           (b) ``detect(prompt_groups=plan)`` with the fused launch (``group_fused = True``, $WEDETECT_GROUP_FUSED=1);
           (b2) the same as the tower runs it by default (wd_similarity_split blocks + wd_group_rows);
           (c) the dense step over the 1203 first captions: the same output size with 0.6 x the GEMM — the floor.
  kernels  ``wd_group_similarity_split`` against ``wd_similarity_split`` on the SAME operands (the step's own split embeddings and
           split bank) and against ``wd_similarity_split`` + ``wd_group_rows``, ALTERNATELY, each between two device events.

Reported: mean / median / min / max / std per leg and the ratios, with the run-to-run noise (the larger std of the legs compared)
they are to be read against.  Checked before timing: the fused launch equals wd_group_rows over wd_similarity_split's output, and
(b) equals (a), tensor for tensor.  Prints everything and writes profiles/prompt_groups.txt.
"""
import argparse
import json
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
    ap.add_argument("--k", type=int, default=10, help="rounds of the alternating steps")
    ap.add_argument("--kernel-k", type=int, default=30, help="rounds of the alternating kernel launches")
    ap.add_argument("--texts", default=os.path.join(ROOT, "tests", "golden", "lvis_v1_class_texts.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_groups.txt"))
    args = ap.parse_args(argv)

    import torch
    from wedetect_amd import groups as PG
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
    with open(args.texts, encoding="utf-8") as f:
        pg = PG.PromptGroups.from_texts(json.load(f))
    tower = ImageTower(args.size, pack(W.make_state_dict(args.size), args.size), B, hw, hw, max_classes=80, precision="fp16x3")
    tower.fold_text = False
    x = torch.from_numpy(W.make_images(B, hw, hw)).cuda()
    meta = tower.identity_meta()
    meta[:, 7] = 1.0                                         # the mmdet order: rescale before NMS
    tower.calibrate(x)
    rows, G, K = B * tower.ntot, pg.G, pg.K_pad
    flat = torch.from_numpy(W.make_text_bank(pg.P)).cuda()
    bank = pg.pad_bank(flat)
    first = flat.index_select(0, pg.first_of().cuda()).contiguous()
    say(f"# {torch.cuda.get_device_name(0)}; model {args.size}, batch {B} x {hw} x {hw} ({rows} region rows), fp16x3, unfolded head; "
        f"plan {pg}; steps K = {args.k}, kernels K = {args.kernel_k}")
    say(f"# score tensor over the padded prompts {rows * K * 4 / 2 ** 30:.2f} GiB, class scores {rows * G * 4 / 2 ** 30:.2f} GiB")
    thr, iou = 0.001, 0.7
    kw = dict(normalize_text=True, score_thr=thr, iou_thr=iou, with_embed=False, nms="mmcv")
    # the class maximum in torch: column j of every class (clamped to its last prompt), one gather per prompt position
    go = pg.group_of.numpy()
    starts = np.flatnonzero(np.r_[True, go[1:] != go[:-1]])
    lens = np.diff(np.r_[starts, K])
    cols = [torch.from_numpy(starts + np.minimum(j, lens - 1)).cuda() for j in range(int(lens.max()))]

    def torch_class_max(s):
        out = s.index_select(2, cols[0])
        for c in cols[1:]:
            out = torch.maximum(out, s.index_select(2, c))
        return out

    def leg_a():
        tower.wait_post(reads=True)
        tower.features(x, num_classes=K)
        return tower.postprocess(torch_class_max(tower.similarity(bank, normalize=True)), thr, meta, iou, False, "mmcv")

    def leg_b(fused=True):
        was, tower.group_fused = tower.group_fused, fused
        try:
            return tower.detect(x, bank, meta, prompt_groups=pg, **kw)
        finally:
            tower.group_fused = was

    legs = {"a": leg_a, "b": leg_b, "b2": lambda: leg_b(False), "c": lambda: tower.detect(x, first, meta, **kw)}
    snap = lambda r: {n: v.clone() for n, v in r.items()}
    for _ in range(2):                                       # warm every buffer and the split banks
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ra, rb, rb2 = snap(leg_a()), snap(leg_b()), snap(leg_b(False))
    torch.cuda.synchronize()
    same = all(bool(torch.equal(ra[n], rb[n])) and bool(torch.equal(ra[n], rb2[n])) for n in ra)
    say(f"(b) and (b2) equal (a), tensor for tensor: {same}; kept rows per image {ra['count'].tolist()[:4]} ...")
    ok = same
    per = {n: [] for n in legs}
    for _ in range(args.k):
        for n, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            per[n].append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: f"mean {v.mean():9.3f} ms  median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}  std {v.std():7.3f}"
    a, b, b2, c = (np.asarray(per[n]) for n in legs)
    say(f"step (a) dense over {K} rows + torch class max + postprocess : {stat(a)}")
    say(f"step (b) prompt_groups, fused launch (WEDETECT_GROUP_FUSED=1) : {stat(b)}")
    say(f"step (b2) prompt_groups, the default: similarity + group_rows : {stat(b2)}")
    say(f"step (c) dense over the {G} first captions (the floor)       : {stat(c)}")
    noise = max(a.std(), b.std())
    say(f"step ratio (b)/(a) = {np.median(b) / np.median(a):.3f} of medians, (b2)/(a) = {np.median(b2) / np.median(a):.3f}, (b)/(c) = "
        f"{np.median(b) / np.median(c):.3f}; noise of this run (larger std of (a), (b)) {noise:.3f} ms; (b) at or below (a) beyond the noise: "
        f"{bool(np.median(b) + noise <= np.median(a))}")
    # ---- the launches on the step's own operands
    leg_b()
    torch.cuda.synchronize()
    ts = tower._split_text(bank, True)
    unscale = ts[1] / tower.sscale.get("embed", 1.0)
    seg = (tower.ntot, tower.off[1], tower.off[2], tower.lvl_scale, tower.lvl_bias)
    _, god, bfd = pg.device("cuda")
    dense = torch.empty(rows, K, device="cuda")
    out_f, out_r = torch.empty(rows, G, device="cuda"), torch.empty(rows, G, device="cuda")

    def k_dense():
        L.similarity_split(tower.embed_s, rows, ts[0], unscale, dense, K, EMBED_DIM, K, seg=seg, sigmoid=True)

    def k_fused():
        PG.group_similarity_split(tower.embed_s, rows, ts[0], unscale, K, EMBED_DIM, god, bfd, 0, out_f, G, G, seg=seg)

    def k_two():
        k_dense()
        PG.group_rows(dense, rows, K, K, god, bfd, 0, out_r, G, G)

    kernels = [("dense", k_dense), ("fused", k_fused), ("two", k_two)]
    for _, fn in kernels:
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_f, out_r))
    ok &= same
    say(f"wd_group_similarity_split equals wd_group_rows over wd_similarity_split's output: {same}")
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
    say(f"kernel wd_similarity_split ({K} columns)            : {stat(kt['dense'])}")
    say(f"kernel wd_group_similarity_split ({G} classes)      : {stat(kt['fused'])}")
    say(f"kernels wd_similarity_split + wd_group_rows           : {stat(kt['two'])}")
    kn = max(kt["dense"].std(), kt["fused"].std())
    say(f"kernel ratio fused / dense = {np.median(kt['fused']) / np.median(kt['dense']):.3f} of medians, fused / two = "
        f"{np.median(kt['fused']) / np.median(kt['two']):.3f}; noise (larger std of dense, fused) {kn:.3f} ms; fused at or below dense beyond "
        f"the noise: {bool(np.median(kt['fused']) + kn <= np.median(kt['dense']))}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
