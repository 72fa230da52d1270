"""ImageTower.detect(prompt_groups=...) (GPU): the grouped step against ``postprocess()`` run on torch's class-wise ``amax`` of
``similarity(padded bank)`` of the SAME tower's unfolded head, tensor for tensor, in line and pipelined; a plan of singletons
against the plain dense unfolded step; a block-path plan that crosses the 4096-row chunk; the range guard's fp32 re-run; the
detector's keyword.  nano and base towers at 64 x 64 (84 anchors per image), B = 2 and 4, both precisions, random weights."""
import warnings

import numpy as np
import pytest
import torch

import tests.groups_hazards  # noqa: F401
from tests import groups_ref as GR
from tests.test_gpu_hazards import _bank, _batches, _configure
from tests.test_gpu_network import build

pytestmark = pytest.mark.gpu

HW, IOU, THR = 64, 0.7, 0.0
FIELDS = ("bboxes", "scores", "labels", "anchors", "count", "embeddings")
KW = dict(normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=True, nms="mmcv")
CHUNKED = (3, 1, 4, 1, 5, 9, 2, 6) * 130                     # 31 prompts and one padding row per bin: K_pad = 4096 + 64


def _tower(arch, b, precision):
    _, t, _ = build(arch, b, HW, num_prompts=48, precision=precision, max_classes=16)
    t.fold_text = False                                      # the dense reference runs on the unfolded head too
    return t


def _snap(r):
    torch.cuda.synchronize()
    return {n: v.clone() for n, v in r.items()}


def _plan_and_bank(sizes, seed=4321):
    from wedetect_amd.groups import PromptGroups
    pg = PromptGroups.from_sizes(sizes)
    return pg, pg.pad_bank(_bank(pg.P, seed=seed))


def _reference(t, x, bank, pg, meta):
    """postprocess() on the torch class maximum of the materialised scores of the padded bank."""
    t.features(x, num_classes=bank.shape[0])
    s = t.similarity(bank, normalize=True)
    cm = GR.class_amax(s, pg.group_of.numpy()).contiguous()
    return _snap(t.postprocess(cm, THR, meta, IOU, True, "mmcv")), cm


def _count_calls(PG):
    calls = {}
    real = PG.group_similarity_split, PG.group_rows
    PG.group_similarity_split = lambda *a, **k: (calls.__setitem__("fused", calls.get("fused", 0) + 1), real[0](*a, **k))[1]
    PG.group_rows = lambda *a, **k: (calls.__setitem__("rows", calls.get("rows", 0) + 1), real[1](*a, **k))[1]
    return calls, real


@pytest.mark.parametrize("arch,b,precision,fused", [("nano", 2, "fp16x3", True), ("nano", 4, "fp16x3", None), ("nano", 4, "fp32", None),
                                                     ("base", 4, "fp16x3", True), ("base", 2, "fp16x3", None), ("base", 2, "fp32", None)])
def test_grouped_step_equals_postprocess_of_the_class_maximum_in_line_and_pipelined(arch, b, precision, fused):
    """``fused`` None: the tower as it is built (wd_similarity_split / wd_conv_gemm blocks + wd_group_rows); True: the fused launch
    ($WEDETECT_GROUP_FUSED=1)."""
    from wedetect_amd import groups as PG
    t = _tower(arch, b, precision)
    assert t.group_fused is False                            # the default (engine.ImageTower.__init__ says why)
    if fused:
        t.group_fused = True
    pg, bank = _plan_and_bank(GR.K352)
    meta, batches = t.identity_meta(), _batches(b, HW, n=3)
    calls, real = _count_calls(PG)
    try:
        inline = [_snap(t.detect(x, bank, meta, prompt_groups=pg, **KW)) for x in batches]      # a cold tower: every buffer grows here
        assert tuple(t.scores.shape)[2] == (16 if fused else pg.K_pad)                          # the fused path never touches self.scores
        gen = t.generation
        _configure(t, depth="2")
        piped = []
        for x in batches:                                    # back to back, no host synchronisation in between
            r = t.detect(x, bank, meta, overlap_post=True, prompt_groups=pg, **KW)
            with torch.cuda.stream(t.post_stream):
                piped.append({n: v.clone() for n, v in r.items()})
        t.wait_post()
        torch.cuda.synchronize()
        assert t.generation == gen                           # warm: nothing is re-allocated
    finally:
        PG.group_similarity_split, PG.group_rows = real
    assert calls == ({"fused": 6} if fused else {"rows": 6}), calls
    assert int(t.range_flags.max()) == 0
    _configure(t, depth="1")
    for i, x in enumerate(batches):
        want, cm = _reference(t, x, bank, pg, meta)
        assert int(want["count"].min()) > 0 and int(want["labels"].max()) < pg.G
        for got in (inline[i], piped[i]):
            for n in FIELDS:
                assert torch.equal(got[n], want[n]), f"batch {i}: {n}"
        if i == 0:                                           # the scores themselves
            assert torch.equal(t.group_scores(bank, pg, True), cm)
    for bad in (dict(best_class=True), dict(sparse_scores=True), dict(best_class=True, top_names=2)):
        with pytest.raises(ValueError, match="prompt_groups"):
            t.detect(batches[0], bank, meta, prompt_groups=pg, **bad, **KW)
    with pytest.raises(Exception, match="pad_bank"):
        t.detect(batches[0], bank[:320].contiguous(), meta, prompt_groups=pg, **KW)


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_a_plan_of_singletons_equals_the_dense_unfolded_step(precision):
    t = _tower("nano", 2, precision)
    pg, bank = _plan_and_bank((1,) * 300)
    assert (pg.G, pg.K_pad) == (300, 320) and torch.equal(bank[:300], _bank(300))
    meta, x = t.identity_meta(), _batches(2, HW, n=1)[0]
    got = _snap(t.detect(x, bank, meta, prompt_groups=pg, **KW))
    dense = _snap(t.detect(x, _bank(300), meta, **KW))
    for n in FIELDS:
        assert torch.equal(got[n], dense[n]), n
    assert int(dense["count"].min()) > 0


@pytest.mark.parametrize("precision,fused", [("fp32", True), ("fp16x3", False)])
def test_block_path_plan_that_crosses_the_4096_row_chunk(precision, fused):
    """K_pad = 4096 + 64 on the block path: an fp32 tower (wd_conv_gemm blocks), and an fp16x3 tower with the fused launch switched
    off (wd_similarity_split blocks + wd_group_rows: the default)."""
    from wedetect_amd import groups as PG
    pg, bank = _plan_and_bank(CHUNKED)
    assert pg.K_pad == 4096 + 64 == PG.ROWS_CHUNK + 64
    assert all(a // 4096 == (z - 1) // 4096 for a, z in GR.class_ranges(pg.group_of.numpy()))      # next-fit: no class across row 4096
    assert int(pg.group_of[4095]) + 1 == int(pg.group_of[4096]) == int(pg.bin_first[128])
    t = _tower("nano", 2, precision)
    t.group_fused = fused
    meta, x = t.identity_meta(), _batches(2, HW, n=1)[0]
    calls, real = _count_calls(PG)
    try:
        got = _snap(t.detect(x, bank, meta, prompt_groups=pg, **KW))
    finally:
        PG.group_similarity_split, PG.group_rows = real
    assert calls == {"rows": 2} and tuple(t.scores.shape) == (2, t.ntot, 4096)
    want, _ = _reference(t, x, bank, pg, meta)
    for n in FIELDS:
        assert torch.equal(got[n], want[n]), n
    assert int(want["count"].min()) > 0


def test_range_guard_rerun_stays_grouped():
    """Embedding convs scaled out of the fp16 range: the fused launch raises the flag and stores NaN, the top-k reports the images,
    checked_counts() switches the tower to fp32 and repeats the step — grouped again, through wd_group_rows — and the result is
    the fp32 tower's grouped step."""
    from wedetect_amd import groups as PG
    pg, bank = _plan_and_bank(GR.K352)
    towers = []
    for precision in ("fp32", "fp16x3"):
        t = _tower("nano", 2, precision)
        for l in range(3):
            t.P[f"head{l}.embed.w"].mul_(3e5)
            t.P[f"head{l}.embed.b"].mul_(3e5)
        towers.append(t)
    ref, t = towers
    t.group_fused = True
    meta, x = t.identity_meta(), _batches(2, HW, n=1)[0]
    want = _snap(ref.detect(x, bank, meta, prompt_groups=pg, **KW))
    assert int(want["count"].min()) > 0 and bool(torch.isfinite(want["scores"]).all())
    run = lambda: t.detect(x, bank, meta, prompt_groups=pg, **KW)
    calls, real = _count_calls(PG)
    try:
        res = run()
        torch.cuda.synchronize()
        assert res["count"].tolist() == [-1, -1] and int(t.range_flags.max()) == 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            counts = t.checked_counts(res, run)
    finally:
        PG.group_similarity_split, PG.group_rows = real
    assert calls == {"fused": 1, "rows": 1} and t.precision == "fp32" and t.overflowed
    assert counts == want["count"].tolist()
    for n in FIELDS:
        assert torch.equal(res[n], want[n]), n
    assert int(res["labels"].max()) < pg.G


def test_detector_keyword_scores_classes_and_refuses_mixed_batches():
    from wedetect_amd import weights as W
    from wedetect_amd.detector import DetDataSample, YOLOWorldDetector
    sd_np = W.make_state_dict("nano")
    texts = [[f"c{g}n{j}" for j in range(n)] for g, n in enumerate(GR.K352)]
    flat = [p for t_ in texts for p in t_]
    bank = torch.from_numpy(W.make_text_bank(len(flat)) * np.float32(2.5))
    model = YOLOWorldDetector("nano", test_cfg=dict(max_per_img=50), max_classes=16, prompt_groups=True)
    model.load_state_dict({"state_dict": {n: torch.from_numpy(v) for n, v in sd_np.items()}})
    model.cuda().eval()
    model.set_text_embeddings(bank, texts)
    G = len(texts)
    rgb = W.make_images(2, 64, 64, seed=77)
    bgr_chw = [torch.from_numpy(np.ascontiguousarray(im[..., ::-1].transpose(2, 0, 1))) for im in rgb]
    metas = [dict(ori_shape=(100, 128), scale_factor=(0.5, 0.5), pad_param=np.array([7., 7., 0., 0.])),
             dict(ori_shape=(64, 50), scale_factor=(1.0, 1.0), pad_param=np.array([0., 0., 7., 7.]))]
    first = [t_[0] for t_ in texts]                          # what LoadText leaves in a sample: it finds the bank and its plan
    for with_texts in (False, True):
        samples = [DetDataSample(metainfo=dict(m, **(dict(texts=first) if with_texts else {}))) for m in metas]
        res = model.test_step(dict(inputs=bgr_chw, data_samples=samples))
        for r in res:
            pi = r.pred_instances
            assert 0 < len(pi.scores) <= 50 and int(pi.labels.min()) >= 0 and int(pi.labels.max()) < G
        if with_texts:
            for a, b_ in zip(res, plain):
                assert torch.equal(a.pred_instances.labels, b_.pred_instances.labels) and torch.equal(a.pred_instances.scores, b_.pred_instances.scores)
        plain = res
    # the tower ran the grouped step: its class scores are [B, N, G]
    tower = model._h.tower(2, 64, 64)
    assert tower._group_out is not None and tower._group_out.numel() >= 2 * tower.ntot * G
    # a batch whose samples carry different class lists
    model.text_encoder = lambda names: torch.from_numpy(W.make_text_bank(len(names), seed=9))
    samples = [DetDataSample(metainfo=dict(metas[0], texts=first)), DetDataSample(metainfo=dict(metas[1], texts=["cat", "dog"]))]
    with pytest.raises(NotImplementedError, match="prompt_groups"):
        model.test_step(dict(inputs=bgr_chw, data_samples=samples))
    with pytest.raises(NotImplementedError, match="prompt_groups"):
        model.predict_tiled(np.zeros((300, 300, 3), np.uint8))
