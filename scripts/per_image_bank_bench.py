"""Per-image class banks: the two measurements of profiles/per_image_bank.txt.

    python scripts/per_image_bank_bench.py [--kernel] [--e2e] [--tree DIR]        (no flag: both)

--kernel  wd_similarity_grouped at B = 32, N = 8400, 32 banks of 80 rows, against (a) the shared-bank launch of wd_conv_gemm
          at the same shape and (b) the obvious alternative, 32 launches of wd_conv_gemm with offset pointers on one stream;
          one ragged line (counts uniform in 1 ... 80).  Device events around batches of launches, the three forms
          alternating inside every repeat, median of the repeats; the algorithmic bytes (embeddings read once, scores
          written once, banks) over the time give the achieved HBM rate — the contraction is memory-bound at K = 80
          (0.83 GB of embeddings against 41 GFLOP).
--e2e     YOLOWorldDetector.predict, Base, 32 images at 640 x 640, 32 distinct ``texts`` of 80 captions (a stub text encoder),
          median wall time of repeated calls (each ends in the host read of the kept counts) after warm-up.  Uses the
          detector's public surface only, so ``--tree DIR`` runs the same measurement on another checkout of the project
          (the parent commit, built in DIR; ``--label`` names it in the output) in the same session.
"""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--e2e", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this commit")
ap.add_argument("--shared-first", action="store_true", help="--e2e: time the one-bank batch before the 32-bank batch")
ap.add_argument("--repeats", type=int, default=15)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np          # noqa: E402
import torch                # noqa: E402

from wedetect_amd import lib as L               # noqa: E402
from wedetect_amd import weights as W           # noqa: E402

B, N, K, DIM = 32, 8400, 80, 768
SEG = (N, 6400, 8000, (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def kernel_bench():
    g = torch.Generator(device="cuda").manual_seed(1)
    e = torch.randn(B, N, DIM, device="cuda", generator=g) * 0.8
    banks = torch.nn.functional.normalize(torch.randn(B, K, DIM, device="cuda", generator=g), dim=-1)
    out = torch.empty(B, N, K, device="cuda")
    full = torch.full((B,), K, dtype=torch.int32, device="cuda")
    ragged = torch.randint(1, K + 1, (B,), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    ragged_d = ragged.cuda()
    forms = {
        "grouped, counts all 80 (one launch)": lambda: L.similarity_grouped(e, banks, full, out, B, N, K, DIM, K, SEG),
        "(a) shared bank, one wd_conv_gemm launch": lambda: L.conv_gemm(e, banks[0], None, out, batch=1, hin=1, win=B * N, cin=DIM, lda=DIM,
                                                                       n=K, ldc=K, sigmoid=True, seg=SEG),
        "(b) 32 wd_conv_gemm launches, offset pointers": lambda: [L.conv_gemm(e[b], banks[b], None, out[b], batch=1, hin=1, win=N, cin=DIM,
                                                                             lda=DIM, n=K, ldc=K, sigmoid=True, seg=SEG) for b in range(B)],
        f"grouped, ragged counts 1..80 (sum {int(ragged.sum())})": lambda: L.similarity_grouped(e, banks, ragged_d, out, B, N, K, DIM, K, SEG),
    }
    for fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, fn in forms.items():
            times[k].append(event_ms(fn, 10))
    # grouped == (b) bit for bit (same images, same banks): the comparison is between equal results
    forms["grouped, counts all 80 (one launch)"]()
    ref = out.clone()
    forms["(b) 32 wd_conv_gemm launches, offset pointers"]()
    torch.cuda.synchronize()
    print(f"kernel: B = {B}, N = {N}, K = {K}, dim {DIM}; grouped == 32 launches bit for bit: {torch.equal(ref, out)}")
    bytes_ = (B * N * DIM + B * N * K + B * K * DIM) * 4
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"  {k:52s} median {med[k] * 1e3:8.1f} us  (min {min(v) * 1e3:8.1f}, max {max(v) * 1e3:8.1f}; {args.repeats} x 10 launches)"
              f"  {bytes_ / med[k] / 1e9:7.2f} TB/s of algorithmic bytes")
    ks = list(forms)
    print(f"  grouped / (a) = {med[ks[0]] / med[ks[1]]:.3f}   (b) / grouped = {med[ks[2]] / med[ks[0]]:.3f}   ragged / full = {med[ks[3]] / med[ks[0]]:.3f}")


def _stub_encoder(texts):
    rows = []
    for t in texts:
        g = torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(t)) % (2 ** 31))
        rows.append(torch.randn(DIM, generator=g))
    return torch.stack(rows)


def e2e_bench():
    from wedetect_amd import detector as D
    sd = W.make_state_dict("base", seed=2026, num_prompts=0)
    model = D.YOLOWorldDetector("base", max_classes=K, text_encoder=_stub_encoder)
    model.load_state_dict({"state_dict": {n: torch.from_numpy(v) for n, v in sd.items()}})
    model.cuda().eval()
    rgb = W.make_images(B, 640, 640, seed=5)
    chw = [torch.from_numpy(np.ascontiguousarray(im[..., ::-1].transpose(2, 0, 1))).cuda() for im in rgb]
    texts = [[f"image {i} class {j}" for j in range(K)] for i in range(B)]
    mk = lambda tx: [D.DetDataSample(metainfo=dict(ori_shape=(640, 640), scale_factor=(1.0, 1.0), texts=tx[i])) for i in range(B)]

    def run(tx):
        t0 = time.perf_counter()
        res = model.predict(chw, mk(tx))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, sum(len(r.pred_instances) for r in res)

    legs = [("32 distinct banks of 80 rows", texts), ("one bank of 80 rows for all 32 images", [texts[0]] * B)]
    for name, tx in (legs[::-1] if args.shared_first else legs):
        for _ in range(3):
            run(tx)
        ts = [run(tx) for _ in range(args.repeats)]
        ms = [t for t, _ in ts]
        print(f"e2e [{args.label}] predict, Base, {B} x 640 x 640, {name}: median {statistics.median(ms):7.2f} ms "
              f"(min {min(ms):7.2f}, max {max(ms):7.2f}; {args.repeats} calls, {ts[0][1]} kept rows)", flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a HIP device: nothing here is measured on the host"
    if args.kernel or not args.e2e:
        kernel_bench()
    if args.e2e or not args.kernel:
        e2e_bench()
