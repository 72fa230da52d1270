"""Per-image class banks on the device: wd_similarity_grouped alone against float64, its bit identity with the shared-bank
launch, the whole step against the CPU fixture (tests/golden/per_image_bank.npz) and against shared-bank steps of the same
tower, and YOLOWorldDetector.predict running ONE tower step for a batch of samples with different ``texts``."""
import numpy as np
import pytest
import torch

from tests.util import assert_close, assert_no_relaxations, check_checksum, compare_kept_lists, golden, to_np

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
SEG_SCALE, SEG_BIAS = (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9)          # tests/test_gpu_split.py: the similarity launch's test values
TILE_N = 80                                                         # column tile of wd_similarity_grouped


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g) * scale


# ------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("b_,ntot,ends,k_max,ldo,counts", [
    # N = 8400 (131 full row tiles + one of 16 rows per image), k_max no multiple of 4, vector stores with a scalar tail,
    # counts 0 / 1 / one below, at and one above the column-tile edge / everything
    (6, 8400, (6400, 8000), 163, 168, [0, 1, TILE_N - 1, TILE_N, TILE_N + 1, 163]),
    # fewer rows than one row tile (64), 4-byte stores only (ldo odd), an image without classes in the middle
    (3, 40, (32, 38), 7, 7, [7, 0, 3]),
    # one full column tile, unaligned rows (ldo = 83) with spare columns
    (2, 84, (64, 80), 80, 83, [80, 37]),
    # a second column tile that no image reaches: zero fill only
    (2, 84, (64, 80), 96, 96, [12, 80]),
    # count = NULL: every image takes all k_max rows
    (2, 84, (64, 80), 12, 12, None),
])
@pytest.mark.parametrize("sigmoid", [True, False])
def test_similarity_grouped_matches_float64_pads_with_plus_zero_and_stays_in_bounds(b_, ntot, ends, k_max, ldo, counts, sigmoid):
    """Valid elements against float64 within the bound the shared-bank contraction is held to (tests/test_gpu_split.py, same
    generator / scales / biases: 2e-6 after the sigmoid, 2e-5 on raw logits, rtol 1e-6); padded elements == 0 with the sign bit
    clear; columns [k_max, ldo) of every row and the rows behind the last image untouched."""
    from wedetect_amd import lib as L
    dim = 768
    e = _rand((b_, ntot, dim), 301, 0.8)
    t = torch.nn.functional.normalize(_rand((b_, k_max, dim), 302), dim=-1)
    seg = (ntot, ends[0], ends[1], SEG_SCALE, SEG_BIAS)
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    buf = torch.full((b_ * ntot + 3, ldo), 7.0, device="cuda")
    out = buf[: b_ * ntot].view(b_, ntot, ldo)
    L.similarity_grouped(e, t, cnt, out, b_, ntot, k_max, dim, ldo, seg, sigmoid=sigmoid)
    torch.cuda.synchronize()
    assert bool((buf[b_ * ntot:] == 7.0).all()), "rows behind the last image were written"
    assert bool((out[:, :, k_max:] == 7.0).all()), "columns at or beyond k_max were written"
    pos = torch.arange(ntot, device="cuda")
    lvl = (pos >= ends[0]).long() + (pos >= ends[1]).long()
    sc = torch.tensor(SEG_SCALE, device="cuda", dtype=torch.float64)[lvl][None, :, None]
    bi = torch.tensor(SEG_BIAS, device="cuda", dtype=torch.float64)[lvl][None, :, None]
    ref = torch.einsum("bnc,bkc->bnk", e.double(), t.double()) * sc + bi
    if sigmoid:
        ref = torch.sigmoid(ref)
    tol = 2e-6 if sigmoid else 2e-5
    for b in range(b_):
        c = k_max if counts is None else counts[b]
        pad = out[b, :, c:k_max]
        assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), f"image {b}: padding is not +0"
        err = assert_close(f"similarity_grouped image {b} (count {c}) vs float64", out[b, :, :c], ref[b, :, :c], tol, 1e-6)
        print(f"[per-image] B {b_} N {ntot} k_max {k_max} ldo {ldo} sigmoid {sigmoid} image {b} count {c}: max|d| {err:.3g}")


def test_similarity_grouped_rejects_a_host_count_and_bad_shapes():
    from wedetect_amd import lib as L
    e, t = _rand((2, 84, 768), 1), _rand((2, 8, 768), 2)
    out = torch.empty(2, 84, 8, device="cuda")
    seg = (84, 64, 80, SEG_SCALE, SEG_BIAS)
    with pytest.raises(L.WedetectHipError):
        L.similarity_grouped(e, t, torch.tensor([8, 8], dtype=torch.int32), out, 2, 84, 8, 768, 8, seg)      # host tensor
    with pytest.raises(L.WedetectHipError):
        L.similarity_grouped(e, t, torch.tensor([8, 8], device="cuda"), out, 2, 84, 8, 768, 8, seg)          # int64
    with pytest.raises(L.WedetectHipError):
        L.similarity_grouped(e, t, None, out, 2, 84, 8, 768, 7, seg)                                         # ldo < k_max


# ------------------------------------------------------------------------------------------ 2. bit identity with the shared path
def _tower(arch, b, hw, precision, max_classes=80, **kw):
    from wedetect_amd import weights as W
    from wedetect_amd.engine import ImageTower
    from wedetect_amd.pack import pack
    sd = W.make_state_dict(arch, seed=2026, num_prompts=256)
    return ImageTower(arch, pack(sd, arch), b, hw, hw, max_classes=max_classes, precision=precision, **kw)


@BOTH
@pytest.mark.parametrize("normalize", [True, False])
def test_per_image_similarity_is_bit_identical_to_the_shared_bank_call(precision, normalize):
    """similarity(bank3d, counts)[b, :, :count[b]] == similarity(bank3d[b, :count[b]])[b], bit for bit, at counts on both sides
    of the shared path's tile choices (1, 7: 48-wide tiles; 80: 64 x 80; 81: 96; 256: 128-wide), same tower, same head()."""
    from wedetect_amd import lib as L
    from wedetect_amd import weights as W
    counts = [1, 7, 80, 81, 256]
    b_ = len(counts)
    tower = _tower("base", b_, 128, precision, max_classes=256)
    tower.backbone(torch.from_numpy(W.make_images(b_, 128, 128, seed=31)).cuda())
    tower.neck()
    tower.head()
    bank3 = _rand((b_, 256, 768), 77, 1.3)
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    got = tower.similarity(bank3, normalize=normalize, text_counts=cnt).clone()
    assert tuple(got.shape) == (b_, tower.ntot, 256)
    for b, c in enumerate(counts):
        ref = tower.similarity(bank3[b, :c].contiguous(), normalize=normalize)
        assert tuple(ref.shape) == (b_, tower.ntot, c)
        assert torch.equal(got[b, :, :c].view(torch.int32), ref[b].view(torch.int32)), f"image {b} (count {c}): bits differ from the shared-bank call"
        assert bool((got[b, :, c:] == 0).all()) and not bool(torch.signbit(got[b, :, c:]).any())
    # text_counts None = all k_max rows
    full = tower.similarity(bank3, normalize=normalize).clone()
    ref = tower.similarity(bank3[4].contiguous(), normalize=normalize)
    assert torch.equal(full[4], ref[4])
    # contract violations
    for bad_text, bad_cnt in ((bank3[:3], None), (bank3.double(), None), (bank3.cpu(), None), (bank3[:, :, :767], None),
                              (bank3, cnt.cpu()), (bank3, cnt.long()), (bank3, cnt[:3]), (bank3[0], cnt)):
        with pytest.raises(L.WedetectHipError):
            tower.similarity(bad_text, normalize=normalize, text_counts=bad_cnt)


# ------------------------------------------------------------------------------------------ 3. the whole step against the fixture
def _fixture_inputs(fx):
    from wedetect_amd import weights as W
    counts = [int(v) for v in fx["counts"]]
    banks = [W.make_text_bank(k, seed=int(fx["seed_bank"]) + i) * np.float32(1.7) for i, k in enumerate(counts)]
    bank3 = np.zeros((len(counts), max(counts), 768), np.float32)
    for i, bk in enumerate(banks):
        bank3[i, : counts[i]] = bk
    imgs = W.make_images(int(fx["b"]), int(fx["hw"]), int(fx["hw"]), seed=int(fx["seed_img"]))
    return counts, torch.from_numpy(bank3).cuda(), torch.from_numpy(imgs).cuda()


@BOTH
def test_detect_with_per_image_banks_matches_the_cpu_fixture(precision):
    """Base, B = 4, 128 x 128, counts 80 / 1 / 37 / 12: scores 1e-3 and boxes 1e-2 against the oracle's per-image runs, both kept
    lists through compare_kept_lists (the fixture's effective margins exceed 2e-5: no relaxation but a tie run), labels < count."""
    from oracle import postprocess as opp
    fx = golden("per_image_bank.npz")
    counts, bank3, x = _fixture_inputs(fx)
    b_, hw = int(fx["b"]), int(fx["hw"])
    tower = _tower(str(fx["arch"]), b_, hw, precision)
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    meta = torch.tensor([[float(fx[f"img{i}.pad"][2]), float(fx[f"img{i}.pad"][0]), 0.0, float(fx[f"img{i}.sf"][0]),
                          float(fx[f"img{i}.sf"][1]), float(fx[f"img{i}.ori"][1]), float(fx[f"img{i}.ori"][0]), 1.0] for i in range(b_)],
                        dtype=torch.float32).cuda()
    tag = f"per-image fixture [{precision}]"
    forms = (("mm", dict(score_thr=0.001, nms="mmcv"), meta, lambda bx: bx),
             ("uni", dict(score_thr=0.0, nms="torchvision"), tower.identity_meta(),
              lambda bx: opp.unletterbox(bx, (0.0, 0.0), 1.0, (hw, hw))))
    for form, kw, m, ref_box in forms:
        res = {k: v.clone() for k, v in tower.detect(x, bank3, m, normalize_text=True, text_counts=cnt, **kw).items()}
        torch.cuda.synchronize()
        scores = tower.scores.view(-1)[: b_ * tower.ntot * bank3.shape[1]].view(b_, tower.ntot, bank3.shape[1])
        for i, c in enumerate(counts):
            check_checksum(f"{tag} img{i} scores", scores[i, :, :c].contiguous(), fx, f"img{i}.scores", 1e-3, 1e-3)
            check_checksum(f"{tag} img{i} boxes", tower.boxes[i], fx, f"img{i}.boxes", 1e-2, 1e-5)
            assert bool((scores[i, :, c:] == 0).all())
            n = int(res["count"][i])
            assert n > 0 and int(res["labels"][i, :n].max()) < c and int(res["labels"][i, :n].min()) >= 0, (form, i)
            assert min(fx[f"{form}.img{i}.eff_margins"][[0, 1, 3]]) > 2e-5
            compare_kept_lists(f"{tag} {form} img{i} (K = {c})", res["anchors"][i, :n], res["labels"][i, :n], res["scores"][i, :n],
                               fx[f"{form}.img{i}.anchors"], fx[f"{form}.img{i}.labels"], fx[f"{form}.img{i}.scores"],
                               fx[f"{form}.img{i}.margins"], got_boxes=res["bboxes"][i, :n], ref_boxes=ref_box(fx[f"{form}.img{i}.bboxes"]),
                               eff_margins=fx[f"{form}.img{i}.eff_margins"], allow=("tie_run",))
    assert_no_relaxations(tag, allow_tie_runs=True)


# ------------------------------------------------------------------------------------------ 4. the whole step, device-internal
KEYS = ("bboxes", "scores", "labels", "anchors")


def _assert_image_equal(name, got, b, ref, rb):
    n = int(ref["count"][rb])
    assert int(got["count"][b]) == n, f"{name}: kept {int(got['count'][b])} vs {n}"
    for k in KEYS:
        assert torch.equal(got[k][b, :n], ref[k][rb, :n]), f"{name}: {k} differ"


@BOTH
def test_per_image_step_equals_shared_bank_steps_image_by_image_in_line_and_pipelined(precision):
    """Base, B = 8, 320 x 320, eight banks with different counts: image b of the per-image step == image b of a shared-bank
    step of the SAME tower with bank b (kept rows of bboxes / scores / labels / anchors and the count, torch.equal); then five
    back-to-back detect(overlap_post=True) steps with different images and banks, no host synchronisation in between, equal
    the in-line steps bit for bit."""
    from wedetect_amd import weights as W
    b_, hw = 8, 320
    counts = [80, 1, 37, 12, 5, 64, 17, 33]
    tower = _tower("base", b_, hw, precision)
    meta = tower.identity_meta()
    kw = dict(normalize_text=True, score_thr=0.001, nms="mmcv")
    steps = []
    for s in range(5):
        cs = counts[s:] + counts[:s]
        bank3 = torch.zeros(b_, 80, 768, device="cuda")
        for i, c in enumerate(cs):
            bank3[i, :c] = _rand((c, 768), 1000 + 10 * s + i, 1.7)
        x = torch.from_numpy(W.make_images(b_, hw, hw, seed=50 + s)).cuda()
        steps.append((x, bank3, torch.tensor(cs, dtype=torch.int32, device="cuda"), cs))
    inline = []
    for x, bank3, cnt, cs in steps:
        inline.append({k: v.clone() for k, v in tower.detect(x, bank3, meta, text_counts=cnt, **kw).items()})
    torch.cuda.synchronize()
    x, bank3, cnt, cs = steps[0]
    for b, c in enumerate(cs):
        ref = tower.detect(x, bank3[b, :c].contiguous(), meta, **kw)
        torch.cuda.synchronize()
        _assert_image_equal(f"[{precision}] image {b} (count {c}) per-image vs shared-bank step", inline[0], b, ref, b)
        n = int(ref["count"][b])
        assert n > 0 and int(inline[0]["labels"][b, :n].max()) < c
    piped = []
    for x, bank3, cnt, cs in steps:
        res = tower.detect(x, bank3, meta, text_counts=cnt, overlap_post=True, **kw)
        tower.wait_post()                                   # a stream-side wait: the host does not block
        piped.append({k: v.clone() for k, v in res.items()})
    torch.cuda.synchronize()
    for s, (got, ref) in enumerate(zip(piped, inline)):
        for b in range(b_):
            _assert_image_equal(f"[{precision}] pipelined step {s} image {b}", got, b, ref, b)


# ------------------------------------------------------------------------------------------ 5. the detector
def _stub_encoder(texts):
    """Deterministic stand-in for the text tower: a row per caption, seeded by the caption."""
    rows = []
    for t in texts:
        g = torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(t)) % (2 ** 31))
        rows.append(torch.randn(768, generator=g) * 1.3)
    return torch.stack(rows)


@BOTH
def test_predict_runs_one_step_for_samples_with_different_texts(precision, monkeypatch):
    """8 samples of one shape with 8 different ``texts``: ONE call of _TowerHolder.detect (the parent commit ran 8 steps of batch 1),
    labels below each sample's class count, and every sample's result torch.equal to that of a B = 8 SHARED-bank batch in which
    all samples carry its texts (not a B = 1 call: towers of different batch sizes may differ in low-order bits, engine.py);
    equal texts take the shared path without launching the grouped kernel."""
    from wedetect_amd import detector as D
    from wedetect_amd import lib as L
    from wedetect_amd import weights as W
    sd_np = W.make_state_dict("nano")
    model = D.YOLOWorldDetector("nano", test_cfg=dict(max_per_img=50), max_classes=16, precision=precision, text_encoder=_stub_encoder)
    model.load_state_dict({"state_dict": {n: torch.from_numpy(v) for n, v in sd_np.items()}})
    model.cuda().eval()
    rgb = W.make_images(8, 128, 128, seed=91)
    chw = [torch.from_numpy(np.ascontiguousarray(im[..., ::-1].transpose(2, 0, 1))) for im in rgb]
    ks = [5, 1, 16, 9, 3, 12, 7, 2]
    texts = [[f"class {i}-{j}" for j in range(k)] for i, k in enumerate(ks)]
    mk = lambda tx: [D.DetDataSample(metainfo=dict(ori_shape=(128, 128), scale_factor=(1.0, 1.0), texts=tx[i])) for i in range(8)]
    calls, grouped = [], []
    orig_detect, orig_grouped = D._TowerHolder.detect, getattr(L, "similarity_grouped", None)
    monkeypatch.setattr(D._TowerHolder, "detect", lambda self, *a, **k: (calls.append(1), orig_detect(self, *a, **k))[1])
    monkeypatch.setattr(L, "similarity_grouped", lambda *a, **k: (grouped.append(1), orig_grouped(*a, **k))[1], raising=False)
    res = model.predict(chw, mk(texts))
    assert len(calls) == 1, f"{len(calls)} tower steps for one batch of 8 samples with 8 different texts"
    assert len(grouped) == 1
    mixed = [(r.pred_instances.bboxes.clone(), r.pred_instances.scores.clone(), r.pred_instances.labels.clone()) for r in res]
    for i, k in enumerate(ks):
        assert len(mixed[i][2]) > 0 and int(mixed[i][2].max()) < k and mixed[i][2].dtype == torch.int64
    # the same combination again: the packed bank is reused, still one step
    model.predict(chw, mk(texts))
    assert len(calls) == 2 and len(grouped) == 2 and len(model._packed_banks) == 1
    # all samples carry sample i's texts: a B = 8 shared-bank step (the grouped kernel is not launched) with image i's result
    for i in range(8):
        calls.clear(), grouped.clear()
        shared = model.predict(chw, mk([texts[i]] * 8))
        assert len(calls) == 1 and not grouped, "equal texts must take the shared-bank path"
        pi = shared[i].pred_instances
        assert torch.equal(pi.bboxes, mixed[i][0]) and torch.equal(pi.scores, mixed[i][1]) and torch.equal(pi.labels, mixed[i][2]), \
            f"sample {i}: the mixed-bank batch differs from the shared-bank batch with its texts"
