"""Per-image class banks, host side (run with -m "not gpu"): the fixture and the oracle, the C ABI's new entry, the padding
argument the post-process rests on, and the detector's bank packing."""
import os
import re

import numpy as np
import pytest
import torch

from tests.util import assert_close, check_checksum, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "per_image_bank.npz"


def _banks(fx):
    from wedetect_amd import weights as W
    return [W.make_text_bank(int(k), seed=int(fx["seed_bank"]) + i) * np.float32(1.7) for i, k in enumerate(fx["counts"])]


def test_fixture_loads_and_the_oracle_reproduces_it():
    """tests/golden/make_golden_per_image.py wrote, per image, the oracle's head on that image's features with that image's OWN
    2-D bank (counts 80 / 1 / 37 / 12).  The oracle alone must reproduce scores and boxes (another BLAS threading may move the
    last bit: 1e-5, as for the other network goldens) and both kept lists."""
    from oracle import postprocess as opp
    from oracle import ref_cpu as orc
    from wedetect_amd import weights as W
    from wedetect_amd.arch import HD, get_arch
    fx = golden(FIXTURE)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", FIXTURE)) < 100 * 1024
    arch, b, hw = str(fx["arch"]), int(fx["b"]), int(fx["hw"])
    assert (arch, b, hw) == ("base", 4, 128) and fx["counts"].tolist() == [80, 1, 37, 12]
    assert float(fx["min_eff_margin"]) > float(fx["robust_min"]) == 2e-5
    sd = orc.to_torch(W.make_state_dict(arch, seed=int(fx["seed_w"]), num_prompts=int(fx["num_prompts"])))
    imgs = W.make_images(b, hw, hw, seed=int(fx["seed_img"]))
    ls = np.asarray([sd[HD + f"cls_contrasts.{l}.logit_scale"].item() for l in range(3)], np.float32)
    cb = np.asarray([sd[HD + f"cls_contrasts.{l}.bias"].item() for l in range(3)], np.float32)
    with torch.no_grad():
        _, p = orc.forward_features(sd, get_arch(arch), imgs)
        for i, bank in enumerate(_banks(fx)):
            k = int(fx["counts"][i])
            flat = orc.head_flat(sd, [f[i:i + 1] for f in p], torch.from_numpy(bank), normalize_text=True)
            assert tuple(flat["scores"].shape) == (1, 336, k)
            check_checksum(f"img{i} scores", flat["scores"][0], fx, f"img{i}.scores", 1e-5, 1e-5)
            check_checksum(f"img{i} boxes", flat["boxes"][0], fx, f"img{i}.boxes", 1e-4, 1e-5)
            boxes, scores = flat["boxes"][0].numpy(), flat["scores"][0].numpy()
            mm = opp.mmdet_predict_image(boxes, scores, tuple(float(v) for v in fx[f"img{i}.pad"]),
                                         tuple(float(v) for v in fx[f"img{i}.sf"]), tuple(int(v) for v in fx[f"img{i}.ori"]))
            un = opp.uni_predict_image(boxes, flat["embed"][0].numpy(), scores, flat["level_of"].numpy(), ls, cb)
            for form, o in (("mm", mm), ("uni", un)):
                assert o["scores"].shape[0] == fx[f"{form}.img{i}.scores"].shape[0]
                assert_close(f"{form} img{i} kept scores", o["scores"], fx[f"{form}.img{i}.scores"], 1e-6)
                same = np.mean((o["anchors"] == fx[f"{form}.img{i}.anchors"]) & (o["labels"] == fx[f"{form}.img{i}.labels"]))
                assert same > 0.98, f"{form} img{i}: only {same:.3f} of the kept (anchor, label) rows in the fixture's order"
                assert int(fx[f"{form}.img{i}.labels"].max()) < k and int(o["labels"].max()) < k
                assert min(fx[f"{form}.img{i}.eff_margins"][[0, 1, 3]]) > 2e-5


def test_oracle_3d_branch_is_the_per_image_2d_contraction():
    """The oracle's 'bchw,bkc->bkhw' branch with B different equal-K banks against its 2-D branch image by image: the same
    contraction up to the CPU BLAS's blocking (measured 8e-7 on the scores at the fixture's case; 1e-5 here)."""
    from oracle import ref_cpu as orc
    from wedetect_amd import weights as W
    g = torch.Generator().manual_seed(5)
    sd = orc.to_torch(W.make_state_dict("tiny", seed=2026, num_prompts=8))
    from wedetect_amd.arch import get_arch
    with torch.no_grad():
        _, p = orc.forward_features(sd, get_arch("tiny"), W.make_images(3, 64, 64, seed=9))
        text = torch.randn(3, 5, 768, generator=g)
        f3 = orc.head_flat(sd, p, text, normalize_text=True)
        for i in range(3):
            f2 = orc.head_flat(sd, [f[i:i + 1] for f in p], text[i], normalize_text=True)
            assert_close(f"img{i}", f3["scores"][i], f2["scores"][0], 1e-5)


def test_abi_declares_and_exports_the_grouped_similarity():
    from wedetect_amd import build as wb
    from wedetect_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "wedetect_hip.h")).read()
    assert re.search(r"\bint\s+wd_similarity_grouped\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "yolo_world.py:94-96" in hdr and "yolo_world_head.py:90-108" in hdr
    assert "wd_similarity_grouped" in L.EXPORTS and hasattr(L.LIB, "wd_similarity_grouped") and callable(L.similarity_grouped)
    assert L.ABI_VERSION == 15 and L.LIB.wd_abi_version() == 15
    assert "return 15;" in open(os.path.join(ROOT, "wedetect_amd", "csrc", "abi.hip")).read()
    assert "similarity_grouped.hip" in wb.SOURCES and wb.NO_SCRATCH["similarity_grouped.hip"] == ["similarity_grouped_kernel"]
    # argument contract, checked before any launch (no device needed): null pointers, ldo < k_max, dim % 4, level ends
    three = (L.C.c_float * 3)(1.0, 1.0, 1.0)
    bad = L.LIB.wd_similarity_grouped
    assert bad(0, 0, 0, 0, 1, 8, 4, 768, 4, 4, 6, three, three, 1, None) == -1
    assert bad(16, 16, 0, 16, 1, 8, 4, 768, 3, 4, 6, three, three, 1, None) == -1          # ldo < k_max
    assert bad(16, 16, 0, 16, 1, 8, 4, 766, 4, 4, 6, three, three, 1, None) == -1          # dim % 4
    assert bad(16, 16, 0, 16, 1, 8, 4, 768, 4, 6, 4, three, three, 1, None) == -1          # seg_end0 > seg_end1
    assert bad(16, 16, 0, 16, 1, 8, 4, 768, 4, 4, 9, three, three, 1, None) == -1          # seg_end1 > rows
    assert bad(16, 24, 0, 16, 1, 8, 4, 768, 4, 4, 6, three, three, 1, None) == -1          # bank not 16-byte aligned


@pytest.mark.parametrize("k,k_pad", [(37, 80), (1, 8), (12, 16), (80, 88), (37, 48)])
def test_zero_padded_columns_never_change_the_candidates(k, k_pad):
    """What ImageTower.postprocess rests on with per-image banks: scores [N, K] zero-padded to [N, k_pad] give the same
    candidates in the same order — flat index anchor * k_pad + class is lexicographic in (anchor, class) like anchor * K +
    class, and +0 never passes ``score > thr`` with thr >= 0.  8400 anchors, 30 % exact ties, thresholds 0 ... 0.5, cuts at
    50 ... 30000, against oracle/postprocess.filter_scores_and_topk."""
    from oracle import postprocess as opp
    rng = np.random.default_rng(100 + k)
    n = 8400
    s = rng.random((n, k), dtype=np.float32)
    tie = rng.random((n, k)) < 0.3
    s[tie] = rng.choice(np.asarray([0.0, 0.125, 0.3, 0.5, 0.75], np.float32), size=int(tie.sum()))
    sp = np.zeros((n, k_pad), np.float32)
    sp[:, :k] = s
    assert not np.signbit(sp[:, k:]).any()
    for thr in (0.0, 0.001, 0.3, 0.5):
        for cut in (50, 300, 30000):
            a = opp.filter_scores_and_topk(s, thr, cut)
            b = opp.filter_scores_and_topk(sp, thr, cut)
            for x, y, what in zip(a, b, ("scores", "labels", "anchors")):
                assert np.array_equal(x, y), f"K {k} -> {k_pad}, thr {thr}, cut {cut}: {what} differ"
            assert int(b[1].max(initial=0)) < k


def test_bank_packing_padding_counts_rounding_and_cache_key():
    from wedetect_amd import detector as D
    assert D.BANK_K_ROUND % 4 == 0
    assert [D.round_bank_k(k) for k in (1, 15, 16, 17, 37, 80, 81, 1203)] == [16, 16, 16, 32, 48, 80, 96, 1216]
    with pytest.raises(ValueError):
        D.round_bank_k(0)
    g = torch.Generator().manual_seed(3)
    a, b1, c = (torch.randn(k, 768, generator=g) for k in (37, 1, 12))
    # all samples carry ONE bank object -> the shared path (no packing), whatever the batch size
    assert D.bank_pack_key([a]) is None and D.bank_pack_key([a, a, a]) is None
    # an equal COPY is another object: per-image path
    assert D.bank_pack_key([a, a.clone()]) is not None
    key = D.bank_pack_key([a, b1, c, a])
    assert key == (id(a), id(b1), id(c), id(a)) and key != D.bank_pack_key([b1, a, c, a])
    with pytest.raises(ValueError):
        D.bank_pack_key([])
    packed, counts = D.pack_image_banks([a, b1, c, a])
    assert tuple(packed.shape) == (4, 48, 768) and packed.dtype == torch.float32 and packed.is_contiguous()
    assert counts.dtype == torch.int32 and counts.tolist() == [37, 1, 12, 37]
    for i, t in enumerate((a, b1, c, a)):
        k = t.shape[0]
        assert torch.equal(packed[i, :k], t), "rows are copied as they are (normalisation happens on the device)"
        assert bool((packed[i, k:] == 0).all()) and not bool(torch.signbit(packed[i, k:]).any())
    # one image with a single class, alone with a longer one
    packed, counts = D.pack_image_banks([b1, a.double()[:17]])
    assert tuple(packed.shape) == (2, 32, 768) and counts.tolist() == [1, 17] and torch.equal(packed[0, 0], b1[0])
    assert torch.equal(packed[1, :17], a[:17])
    for bad in (torch.zeros(3, 767), torch.zeros(0, 768), torch.zeros(768)):
        with pytest.raises(ValueError):
            D.pack_image_banks([a, bad])


def test_detector_caches_the_packed_bank_of_a_recurring_combination():
    """YOLOWorldDetector._packed_for: None for one shared object; the same packed tensor OBJECT for the same bank objects
    again (not rebuilt per step); a new one for another order; bounded; cleared with the checkpoint."""
    from wedetect_amd.detector import YOLOWorldDetector
    det = YOLOWorldDetector("tiny", max_classes=8)
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(5, 768, generator=g), torch.randn(3, 768, generator=g)
    cpu = torch.device("cpu")
    assert det._packed_for([a, a], cpu) is None
    p1 = det._packed_for([a, b], cpu)
    p2 = det._packed_for([a, b], cpu)
    assert p1[0] is p2[0] and p1[1] is p2[1] and p1[1].tolist() == [5, 3]
    p3 = det._packed_for([b, a], cpu)
    assert p3[0] is not p1[0] and p3[1].tolist() == [3, 5]
    for i in range(det.PACKED_BANKS_MAX + 3):
        det._packed_for([a, torch.zeros(2, 768)], cpu)
    assert len(det._packed_banks) <= det.PACKED_BANKS_MAX
