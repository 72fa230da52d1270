"""Golden fixture of the per-image class banks: tests/golden/per_image_bank.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_per_image.py [--search]

WeDetect-Base, B = 4, 128 x 128 (the size of net_base_b2_128.npz), seeded weights and images as the other cases, four seeded
banks with counts [80, 1, 37, 12].  Two things are pinned:

1. The per-image contraction itself.  The reference's BNContrastiveHead.forward with ``w`` of shape [B, K, 768] — four
   DIFFERENT banks of equal K, as the reference requires — must be torch.equal to the oracle's 3-D branch
   (oracle/ref_cpu.head_level), level by level.  Needs the reference tree (like make_golden.py); nothing of it is stored.
2. The ragged case.  Per image, the oracle's head on THAT image's pyramid features with THAT image's own 2-D bank: these
   scores — not a zero-padded 3-D run, whose batched einsum differs from the 2-D one by CPU BLAS blocking (up to 8e-7) — are
   the expected scores, stored as checksums / samples (``checksum`` / ``put`` of make_golden.py).  The kept lists come from
   oracle/postprocess.py per image with its own K in both post-process forms (mmdet: score_thr 0.001, rescale, mmcv NMS;
   Uni form: score_thr 0, torchvision NMS on network coordinates) and are stored whole, with their decision margins.

Seeds are searched (``--search``: image seed x bank seed base, make_golden.py's margin machinery) for decisions far from
flipping; the generator REFUSES to write a case whose smallest effective iou / pair / cut margin is not above ROBUST_MIN — the
bound tests/test_gpu_configs.py demands for exactness.  The chosen seeds are kept below so that the fixture regenerates
without the search.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                        # noqa: E402  (puts the repository root on sys.path)

from oracle import postprocess as opp           # noqa: E402
from oracle import ref_cpu as orc               # noqa: E402
from wedetect_amd import weights as W           # noqa: E402
from wedetect_amd.arch import HD, get_arch      # noqa: E402

ARCH, B, HW = "base", 4, 128
COUNTS = (80, 1, 37, 12)
SEED_W = 2026
# (image seed, bank seed base): bank i is make_text_bank(COUNTS[i], seed=base + i) * 1.7 (not unit-norm on purpose).
# Output of --search, which starts at the seeds of the other cases (1234 / 4321).
SEEDS = (1234, 4321)
EQUAL_K = 80                                    # K of the equal-K [B, K, 768] run against the reference


def banks_for(base: int):
    return [W.make_text_bank(k, seed=base + i) * np.float32(1.7) for i, k in enumerate(COUNTS)]


def letterbox_meta(i: int):
    """Synthetic letterbox metadata per image, as case_network: pad (top, bottom, left, right), scale (w, h), ori (h, w)."""
    if i % 2 == 0:
        return (8.0, 8.0, 0.0, 0.0), (0.5, 0.5), (int((HW - 16) / 0.5), int(HW / 0.5))
    return (0.0, 0.0, 12.0, 12.0), (0.8, 0.8), (int(HW / 0.8), int((HW - 24) / 0.8))


def per_image_expected(sd, p, banks):
    """Image i -> (head_flat of the oracle on image i alone with its own 2-D bank, mmdet-form result, Uni-form result)."""
    ls = np.asarray([sd[HD + f"cls_contrasts.{l}.logit_scale"].item() for l in range(3)], dtype=np.float32)
    cb = np.asarray([sd[HD + f"cls_contrasts.{l}.bias"].item() for l in range(3)], dtype=np.float32)
    out = []
    for i, bank in enumerate(banks):
        flat = orc.head_flat(sd, [f[i:i + 1] for f in p], torch.from_numpy(bank), normalize_text=True)
        boxes, scores = flat["boxes"][0].numpy(), flat["scores"][0].numpy()
        pad, sf, ori = letterbox_meta(i)
        mm = opp.mmdet_predict_image(boxes, scores, pad, sf, ori, effective=True)
        un = opp.uni_predict_image(boxes, flat["embed"][0].numpy(), scores, flat["level_of"].numpy(), ls, cb, effective=True)
        out.append((flat, mm, un))
    return out


def smallest_effective_margin(exp) -> float:
    """min over images and both forms of the effective iou / pair / cut margins (the kept-row gap is the tie-run allowance
    of tests/util.compare_kept_lists, as for the margin-robust goldens of make_golden.py)."""
    return float(min(min(o["eff_margins"][[0, 1, 3]]) for _, mm, un in exp for o in (mm, un)))


def search(trials_img: int = 8, trials_bank: int = 8):
    sd = orc.to_torch(W.make_state_dict(ARCH, seed=SEED_W, num_prompts=256))
    best = (-1.0, None)
    with torch.no_grad():
        for s_img in range(SEEDS[0], SEEDS[0] + trials_img):
            _, p = orc.forward_features(sd, get_arch(ARCH), W.make_images(B, HW, HW, seed=s_img))
            for s_bank in range(SEEDS[1], SEEDS[1] + 10 * trials_bank, 10):
                m = smallest_effective_margin(per_image_expected(sd, p, banks_for(s_bank)))
                print(f"images {s_img} banks {s_bank}: smallest effective margin {m:.3g}", flush=True)
                if m > best[0]:
                    best = (m, (s_img, s_bank))
                if m > mg.ROBUST_MIN:
                    return best
    return best


def reference_equal_k(sd_np, p_orc, base: int) -> None:
    """BNContrastiveHead.forward of the reference with a [B, K, 768] bank of B different banks == the oracle's 3-D branch."""
    gp = mg.import_generate_proposal()
    model, _ = mg.load_uni_model(gp, ARCH, 256, SEED_W)
    sd = orc.to_torch(sd_np)
    text_b = torch.from_numpy(np.stack([W.make_text_bank(EQUAL_K, seed=base + i) * np.float32(1.7) for i in range(B)]))
    with torch.no_grad():
        outs = model.bbox_head(p_orc, text_b)
        for l in range(3):
            _, lg_orc, bb_orc = orc.head_level(sd, l, p_orc[l], text_b, normalize_text=True)
            mg.must_equal(f"per_image.mm_logits{l} [B, K, 768]", outs[l][0], lg_orc)
            mg.must_equal(f"per_image.mm_bbox{l}", outs[l][1], bb_orc)


def main() -> None:
    assert os.path.isdir(mg.REF), "reference tree not present: goldens can only be generated in the build container"
    if "--search" in sys.argv:
        print("best:", search())
        return
    s_img, s_bank = SEEDS
    sd_np = W.make_state_dict(ARCH, seed=SEED_W, num_prompts=256)
    sd = orc.to_torch(sd_np)
    imgs = W.make_images(B, HW, HW, seed=s_img)
    with torch.no_grad():
        _, p = orc.forward_features(sd, get_arch(ARCH), imgs)
        reference_equal_k(sd_np, p, s_bank)
        banks = banks_for(s_bank)
        exp = per_image_expected(sd, p, banks)
    fx = dict(arch=ARCH, b=B, hw=HW, seed_w=SEED_W, seed_img=s_img, seed_bank=s_bank, num_prompts=256,
              counts=np.asarray(COUNTS, dtype=np.int32), robust_min=np.float64(mg.ROBUST_MIN))
    for i, (flat, mm, un) in enumerate(exp):
        mg.put(fx, f"img{i}.scores", mg.checksum(flat["scores"][0]))          # [N, K_i] row-major
        mg.put(fx, f"img{i}.boxes", mg.checksum(flat["boxes"][0]))
        pad, sf, ori = letterbox_meta(i)
        fx[f"img{i}.pad"], fx[f"img{i}.sf"], fx[f"img{i}.ori"] = np.asarray(pad), np.asarray(sf), np.asarray(ori)
        for form, o in (("mm", mm), ("uni", un)):
            for key in ("bboxes", "scores", "labels", "anchors"):
                fx[f"{form}.img{i}.{key}"] = o[key]
            fx[f"{form}.img{i}.margins"] = mg._margins(o)
            fx[f"{form}.img{i}.eff_margins"] = o["eff_margins"]
            assert int(o["labels"].max()) < COUNTS[i]
            print(f"  {form} img{i} (K = {COUNTS[i]}): kept {o['scores'].shape[0]}, margins {fx[f'{form}.img{i}.margins']}, "
                  f"effective {o['eff_margins']}")
    m = smallest_effective_margin(exp)
    print(f"smallest effective iou / pair / cut margin {m:.3g} (ROBUST_MIN {mg.ROBUST_MIN:g})")
    if not m > mg.ROBUST_MIN:
        raise SystemExit(f"REFUSED: smallest effective margin {m:.3g} is not above ROBUST_MIN {mg.ROBUST_MIN:g}; run --search "
                         "and put the seeds it finds into SEEDS")
    fx["min_eff_margin"] = np.float64(m)
    path = os.path.join(mg.OUT, "per_image_bank.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
