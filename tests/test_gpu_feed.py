"""The streamed loader on the GPU: the batched feed kernels against the per-image kernels (bit for bit), ``predict_stream`` of
both detectors against the serial loop on the same batches, the range-guard detour, the per-batch counters, and ``test.py
--loader stream`` against ``--loader serial`` end to end.  Images are generated from seeds."""
import json
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8 = torch.uint8


# ------------------------------------------------------------------------------------------ kernel against per-image kernels
def _ragged(canvas, b, seed):
    """b (image, family, new_h, new_w, interp) for an H x W canvas, cycling through every mode of the feed."""
    H, W = canvas
    rng = np.random.default_rng(seed)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    fit = lambda h, w: (max(1, int(round(h * min(H / h, W / w)))), max(1, int(round(w * min(H / h, W / w)))))
    kinds = [
        lambda: (img(H // 2, W // 2), "cv", H // 2, W // 2, "area"),                                   # COPY
        lambda: (img(H, W), "cv", H // 2, W // 2, "area"),                                             # AREA_FAST 2 x 2
        lambda: (img(3 * (H // 4), 3 * (W // 4)), "cv", H // 4, W // 4, "area"),                       # AREA_FAST 3 x 3
        lambda: (img(H + 37, W + 211), "cv", *fit(H + 37, W + 211), "area"),                           # general AREA
        lambda: (img(H // 3 + 1, W // 3 + 5), "cv", *fit(H // 3 + 1, W // 3 + 5), "bilinear"),         # LINEAR
        lambda: (img(H + 200, W + 77), "pil", *fit(H + 200, W + 77), None),                            # Pillow shrink
        lambda: (img(H // 5, W // 4), "pil", *fit(H // 5, W // 4), None),                              # Pillow enlarge
        lambda: (img(H // 2, 1), "pil", H, 2, None),                                                   # 1 pixel wide
    ]
    order = [0, 1, 3, 4, 5, 2, 6, 7]                       # the first five cover the five modes
    return [kinds[order[(k + seed) % len(kinds)]]() for k in range(b)]


def _per_image_reference(batch, plans, canvas, dev):
    """The canvas as the existing per-image entry points write it: wd_cv_resize_paste_u8 / wd_letterbox_u8."""
    from wedetect_amd import lib as L
    from wedetect_amd.pipeline import _PlanCache, cv_resize_pad
    from wedetect_amd.preprocess import resample_coeffs
    H, W = canvas
    out = torch.empty(len(batch), H, W, 3, dtype=u8, device=dev)
    cache = _PlanCache(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for k, ((a, kind, nh, nw, interp), p) in enumerate(zip(batch, plans)):
        src = torch.from_numpy(a).to(dev)
        h, w = a.shape[:2]
        if kind == "cv":
            cv_resize_pad(src, nh, nw, interp, canvas, p["top"], p["left"], 114, swap_rb=bool(p["swap_rb"]), plans=cache, out=out[k])
        else:
            (bh, kh), (bv, kv) = resample_coeffs(w, nw), resample_coeffs(h, nh)
            tmp = torch.empty(h * nw * 3, dtype=u8, device=dev)
            L.letterbox_u8(src, h, w, t(bh), t(kh), kh.shape[1], t(bv), t(kv), kv.shape[1], tmp, out[k], H, W, nw, nh, p["left"], p["top"],
                           (114, 114, 114))
            if p["swap_rb"]:                                # the per-image entry has no channel swap: fill is grey, flip the bytes
                out[k] = out[k].flip(-1)
    return out


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("b", [1, 5, 32])
@pytest.mark.parametrize("canvas", [(640, 640), (1280, 1280), (512, 640)])
def test_feed_batch_equals_the_per_image_kernels(canvas, b, swap):
    from wedetect_amd import feed as F
    dev = torch.device("cuda")
    H, W = canvas
    batches = [_ragged(canvas, b, seed) for seed in (range(8) if b == 1 else [0])]     # b == 1: every mode, one batch each
    for batch in batches:
        plans = []
        for a, kind, nh, nw, interp in batch:
            top, left = (H - nh) // 2, (W - nw) // 2
            plans.append(F.plan_cv(a.shape[0], a.shape[1], nh, nw, interp, top, left, 114, swap_rb=swap) if kind == "cv"
                         else F.plan_pillow(a.shape[0], a.shape[1], nh, nw, top, left, (114, 114, 114), swap_rb=swap))
        if b >= 5:
            assert {p["mode"] for p in plans} == {0, 1, 2, 3, 4}
        offs, nbytes = F.src_offsets([a.shape[:2] for a, *_ in batch])
        src = np.zeros(nbytes, np.uint8)
        for (a, *_), o in zip(batch, offs):
            src[o:o + a.size] = a.reshape(-1)
        packed = F.pack_batch(plans, offs)
        ctl = torch.from_numpy(packed["block"]).to(dev)
        tmp = torch.full((max(packed["tmp_bytes"], 256),), 0xFF, dtype=u8, device=dev)
        dst = torch.full((b, H, W, 3), 0xEE, dtype=u8, device=dev)
        F.feed_batch_u8(torch.from_numpy(src).to(dev), ctl.data_ptr(), packed["images"], ctl.data_ptr() + packed["tab_off"],
                        packed["table_elems"], tmp if packed["tmp_bytes"] else None, dst)
        ref = _per_image_reference(batch, plans, canvas, dev)
        torch.cuda.synchronize()
        for k in range(b):
            assert torch.equal(dst[k], ref[k]), (f"canvas {canvas}, image {k} (mode {plans[k]['mode']}, {batch[k][0].shape[:2]} -> "
                                                 f"{plans[k]['new_h']}x{plans[k]['new_w']}): {int((dst[k] != ref[k]).sum())} bytes differ")
        assert F.launches(packed["images"]) <= 3


# ------------------------------------------------------------------------------------------ detectors
SIZES = [(640, 480), (480, 640), (640, 427), (500, 375), (333, 500), (640, 640), (1024, 683), (200, 150), (320, 240), (427, 640),
         (612, 612), (1280, 960), (96, 180)]


def _write_images(tmp, n, seed=11):
    """n seeded JPEGs of COCO-like sizes with smooth content (+ a little noise): paths."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    paths = []
    for k in range(n):
        w, h = SIZES[k % len(SIZES)]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        chans = []
        for c in range(3):
            fx, fy, ph = rng.uniform(0.005, 0.05), rng.uniform(0.005, 0.05), rng.uniform(0, 6.28)
            chans.append(127 + 90 * np.sin(fx * xx + ph) * np.cos(fy * yy + c) + rng.normal(0, 12, (h, w)))
        a = np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)
        p = str(tmp / f"img_{k:04d}.jpg")
        Image.fromarray(a).save(p, quality=90)
        paths.append(p)
    return paths


def _pipeline_cfg(size):
    from wedetect_amd.cfgfile import Config
    cfg = Config.fromfile(os.path.join(ROOT, "config", f"wedetect_{size}.py"))
    return [p.to_dict() if hasattr(p, "to_dict") else dict(p) for p in cfg.test_dataloader.dataset.pipeline]


_SD = {}


def _state(size):
    from wedetect_amd import weights as W
    if size not in _SD:
        _SD[size] = {k: torch.from_numpy(v) for k, v in W.make_state_dict(size).items()}
    return _SD[size]


def _detector(size, precision, names, state=None):
    from wedetect_amd import weights as W
    from wedetect_amd.detector import YOLOWorldDetector
    m = YOLOWorldDetector(size, test_cfg=dict(max_per_img=100), max_classes=len(names), precision=precision)
    m.load_state_dict(state if state is not None else _state(size))
    m.cuda().eval()
    m.set_text_embeddings(torch.from_numpy(W.make_text_bank(len(names))).cuda(), [[n] for n in names])
    return m


def _serial(model, infos, pipeline, bs):
    """The loop of test.py (``predict_shard``): one image at a time through the pipeline, stack, test_step."""
    from wedetect_amd.pipeline import Compose
    pipe = Compose(pipeline)
    out = []
    for lo in range(0, len(infos), bs):
        items = [pipe(dict(i)) for i in infos[lo:lo + bs]]
        data = dict(inputs=torch.stack([it["inputs"] for it in items]), data_samples=[it["data_samples"] for it in items])
        with torch.no_grad():
            out.extend(model.test_step(data))
    return out


def _same_samples(serial, streamed):
    assert len(serial) == len(streamed)
    total = 0
    for k, (a, b) in enumerate(zip(serial, streamed)):
        pa, pb = a.pred_instances, b.pred_instances
        for key in ("bboxes", "scores", "labels"):
            x, y = getattr(pa, key), getattr(pb, key)
            assert not y.is_cuda and y.dtype == x.dtype, key
            assert torch.equal(x.cpu(), y), f"image {k}: {key} differ ({tuple(x.shape)} vs {tuple(y.shape)})"
        for key in ("img_id", "ori_shape", "scale_factor", "img_shape"):
            assert a.metainfo[key] == b.metainfo[key], key
        assert np.array_equal(a.metainfo["pad_param"], b.metainfo["pad_param"])
        total += len(pa.scores)
    assert total > 0
    return total


@pytest.mark.parametrize("size,precision", [("tiny", "fp16x3"), ("tiny", "fp32"), ("base", "fp16x3"), ("base", "fp32")])
def test_predict_stream_equals_predict(tmp_path, size, precision):
    """Six batches of four different images + a tail of two, then one batch of per-image banks with ragged class counts."""
    names = [f"class {k}" for k in range(20)]
    paths = _write_images(tmp_path, 26)
    infos = [dict(img_id=100 + k, img_path=p, texts=[[n] for n in names]) for k, p in enumerate(paths)]
    pipeline = _pipeline_cfg(size)
    m_serial, m_stream = _detector(size, precision, names), _detector(size, precision, names)
    serial = _serial(m_serial, infos, pipeline, 4)
    stats = {}
    streamed = list(m_stream.predict_stream(infos, 4, pipeline, decode_workers=4, stats=stats))
    n = _same_samples(serial, streamed)
    assert [s.metainfo["img_id"] for s in streamed] == [i["img_id"] for i in infos]
    assert stats["batches"] == 7 and stats["max_in_flight"] == 2 and stats["trips"] == 0 and stats["inline_batches"] == 0
    assert stats["feed_launches_max"] <= 3 and stats["h2d_copies_max"] <= 2 and stats["d2h_copies_max"] == 1
    assert stats["d2h_copies"] == 7 and stats["h2d_copies"] == 14 and stats["feed_launches"] == 7 and stats["decode_workers"] == 4
    t_a, t_b = m_serial._h.tower(4, 640, 640), m_stream._h.tower(4, 640, 640)
    assert t_a.fp16x3_trips == t_b.fp16x3_trips == 0 and t_a.precision == t_b.precision == precision
    # per-image banks: every image against its own class list, ragged counts, packed exactly as predict packs them
    from wedetect_amd import weights as W
    bank = torch.from_numpy(W.make_text_bank(40, seed=99)).cuda()
    per = []
    for k, cnt in enumerate((3, 17, 1, 20, 9, 12, 5, 2)):
        tx = [[f"own {k}.{j}"] for j in range(cnt)]
        m_serial._banks[tuple(t[0] for t in tx)] = m_stream._banks[tuple(t[0] for t in tx)] = bank[k:k + cnt].clone()
        per.append(dict(img_id=900 + k, img_path=paths[k], texts=tx))
    serial = _serial(m_serial, per, pipeline, 4)
    streamed = list(m_stream.predict_stream(per, 4, pipeline, decode_workers=2))
    _same_samples(serial, streamed)
    assert max(int(s.pred_instances.labels.max()) for s in streamed if len(s.pred_instances)) < 20
    print(f"{size} {precision}: {n} detections equal over 26 images; stats {stats}")


def test_predict_stream_refuses_other_pipelines(tmp_path):
    names = ["a", "b"]
    m = _detector("tiny", None, names)
    pipeline = _pipeline_cfg("tiny")
    with pytest.raises(NotImplementedError, match="WeDetectLetterResize"):
        list(m.predict_stream([], 4, pipeline[:1] + pipeline[2:]))
    assert list(m.predict_stream([], 4, pipeline)) == []
    from wedetect_amd.stream import DecodeError
    paths = _write_images(tmp_path, 3)
    infos = [dict(img_id=k, img_path=p, texts=[[n] for n in names]) for k, p in enumerate(paths)]
    infos[2]["img_path"] = str(tmp_path / "not_there.jpg")
    with pytest.raises(DecodeError, match="not_there.jpg"):
        list(m.predict_stream(infos, 2, pipeline))
    torch.cuda.synchronize()


def test_simple_detector_stream_equals_forward(tmp_path):
    from wedetect_amd import weights as W
    from wedetect_amd.detector import SimpleYOLOWorldDetector
    sd = {k: torch.from_numpy(v) for k, v in W.to_uni_keys(W.make_state_dict("tiny", num_prompts=32)).items()}

    def make():
        m = SimpleYOLOWorldDetector("tiny", prompt_dim=768, num_prompts=32, num_proposals=100)
        assert not m.load_state_dict(sd, strict=False).missing_keys
        return m.cuda().eval()
    paths = _write_images(tmp_path, 14, seed=23)
    m_serial, m_stream = make(), make()
    serial = []
    for lo in range(0, len(paths), 4):
        serial.extend(m_serial(paths[lo:lo + 4]))
    stats = {}
    streamed = list(m_stream.predict_stream(paths, 4, decode_workers=3, stats=stats))
    assert len(streamed) == len(serial) == 14
    for k, (a, b) in enumerate(zip(serial, streamed)):
        assert set(a) == set(b)
        for key in ("bboxes", "embeddings", "scores", "labels", "scales", "bias"):
            assert not b[key].is_cuda and torch.equal(a[key].cpu(), b[key]), f"image {k}: {key}"
    assert sum(len(o["scores"]) for o in streamed) > 0
    assert stats["feed_launches_max"] == 2 and stats["h2d_copies_max"] <= 2 and stats["d2h_copies_max"] == 1 and stats["max_in_flight"] == 2
    without = list(m_stream.predict_stream(paths[:5], 4, with_embeddings=False))
    assert all("embeddings" not in o for o in without) and all(torch.equal(a["bboxes"], b["bboxes"]) for a, b in zip(without, streamed))


# ------------------------------------------------------------------------------------------ range guard
def _hot_state():
    """tests/test_gpu_detector.py::test_fp16x3_range_guard_falls_back_to_fp32: one pwconv1 scaled by 3e5, undone in the following
    pwconv2 — the GELU hidden activations leave the fp16 range (an overflow raises a flag; nothing faults)."""
    from wedetect_amd import weights as W
    sd = W.make_state_dict("nano")
    hot = dict(sd)
    k1, k2 = "backbone.image_model.model.stages.2.1.pwconv1", "backbone.image_model.model.stages.2.1.pwconv2.weight"
    hot[k1 + ".weight"] = sd[k1 + ".weight"] * np.float32(3e5)
    hot[k1 + ".bias"] = sd[k1 + ".bias"] * np.float32(3e5)
    hot[k2] = sd[k2] / np.float32(3e5)
    return {n: torch.from_numpy(v) for n, v in hot.items()}


@pytest.mark.parametrize("calibrate", [False, True])
def test_stream_range_guard_trip_follows_the_serial_loop(tmp_path, monkeypatch, calibrate):
    """calibrate False: the run-time guard alone — step 0 trips while step 1 is in flight; it is discarded, batch 0 runs in
    line (fp32 fallback), the rest follows in line while the tower is in its fallback.  calibrate True: the first two batches
    are flat grey images, so the first-batch calibration sees small activations; whatever the later batches then do to the
    guard (recalibration, fallback, the return to fp16x3 after FALLBACK_RETRY = 2 clean batches), the stream does the same."""
    from wedetect_amd.engine import ImageTower
    from PIL import Image
    monkeypatch.setattr(ImageTower, "FALLBACK_RETRY", 2)
    names = [f"class {k}" for k in range(20)]
    paths = _write_images(tmp_path, 22, seed=5)
    if calibrate:
        for p in paths[:8]:
            Image.fromarray(np.full((480, 640, 3), 128, np.uint8)).save(p, quality=90)
    infos = [dict(img_id=k, img_path=p, texts=[[n] for n in names]) for k, p in enumerate(paths)]
    pipeline = _pipeline_cfg("tiny")                       # nano weights, the 640 x 640 test pipeline
    hot = _hot_state()

    def make():
        m = _detector("nano", "fp16x3", names, state=hot)
        m._h.auto_calibrate = calibrate
        return m
    m_serial, m_stream = make(), make()
    with warnings.catch_warnings(record=True) as w_serial:
        warnings.simplefilter("always")
        serial = _serial(m_serial, infos, pipeline, 4)
    stats = {}
    with warnings.catch_warnings(record=True) as w_stream:
        warnings.simplefilter("always")
        streamed = list(m_stream.predict_stream(infos, 4, pipeline, stats=stats))
    _same_samples(serial, streamed)
    t_a, t_b = m_serial._h.tower(4, 640, 640), m_stream._h.tower(4, 640, 640)
    print(f"calibrate {calibrate}: serial trips {t_a.fp16x3_trips} retries {t_a.fp16x3_retries} precision {t_a.precision}; "
          f"stream trips {t_b.fp16x3_trips} retries {t_b.fp16x3_retries} precision {t_b.precision}; stats {stats}")
    assert t_b.fp16x3_trips == t_a.fp16x3_trips and t_b.fp16x3_retries == t_a.fp16x3_retries
    assert t_b.precision == t_a.precision and t_b.overflowed == t_a.overflowed and t_b.sscale == t_a.sscale
    assert m_stream._h.precision == m_serial._h.precision
    assert sorted(str(w.message) for w in w_serial if "wedetect_amd" in str(w.message)) == \
        sorted(str(w.message) for w in w_stream if "wedetect_amd" in str(w.message))
    if not calibrate:
        assert t_a.fp16x3_trips >= 1 and stats["trips"] >= 1 and stats["inline_batches"] >= 1 and stats["reissued"] >= 1
        assert any("fp16 range" in str(w.message) for w in w_stream)
    # the two tail images form a tower of their own (2 x 640 x 640): same state there
    t_a, t_b = m_serial._h.tower(2, 640, 640), m_stream._h.tower(2, 640, 640)
    assert t_b.fp16x3_trips == t_a.fp16x3_trips and t_b.precision == t_a.precision


# ------------------------------------------------------------------------------------------ test.py end to end
def _write_dataset(tmp, lvis):
    """The synthetic sets of tests/test_gpu_det_eval.py, regenerated."""
    from PIL import Image
    rng = np.random.default_rng(7)
    names = ["person", "dog", "kite", "cup", "chair"]
    cat_ids = [3, 1, 18, 44, 62]
    (tmp / "val").mkdir(exist_ok=True)
    images, anns = [], []
    for n in range(12):
        h, w = int(rng.integers(96, 200)), int(rng.integers(96, 200))
        iid = 1000 - 37 * n
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp / "val" / f"{iid}.jpg", quality=95)
        im = dict(id=iid, width=w, height=h)
        if lvis:
            im["coco_url"] = f"http://images.cocodataset.org/val/{iid}.jpg"
            im["neg_category_ids"] = [cat_ids[int(rng.integers(0, 5))]]
            im["not_exhaustive_category_ids"] = []
        else:
            im["file_name"] = f"{iid}.jpg"
        images.append(im)
        for _ in range(int(rng.integers(0, 4))):
            x, y = float(rng.uniform(0, w - 20)), float(rng.uniform(0, h - 20))
            bw, bh = float(rng.uniform(8, w - x)), float(rng.uniform(8, h - y))
            a = dict(id=len(anns) + 1, image_id=iid, category_id=cat_ids[int(rng.integers(0, 5))], bbox=[x, y, bw, bh],
                     area=bw * bh)
            if not lvis:
                a["iscrowd"] = 0
            anns.append(a)
    cats = [dict(id=c, name=nm) for c, nm in zip(cat_ids, names)]
    if lvis:
        for k, c in enumerate(cats):
            c["frequency"] = "rcf"[k % 3]
    ann = dict(images=images, annotations=anns, categories=cats)
    path = tmp / ("lvis.json" if lvis else "coco.json")
    path.write_text(json.dumps(ann))
    texts = tmp / "texts.json"
    texts.write_text(json.dumps([[nm] for _, nm in sorted(zip(cat_ids, names))]))
    return ann, str(path), str(texts)


@pytest.mark.parametrize("lvis", [False, True])
def test_test_py_stream_loader_equals_serial_loader(tmp_path, lvis):
    from wedetect_amd import weights as W
    ann, ann_path, texts_path = _write_dataset(tmp_path, lvis)
    sd = {k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny").items()}
    ckpt = str(tmp_path / "tiny.pth")
    torch.save({"state_dict": sd, "meta": {}}, ckpt)
    bank_path = str(tmp_path / "bank.pt")
    torch.save(torch.from_numpy(np.random.default_rng(3).standard_normal((5, 768)).astype(np.float32)), bank_path)
    ds = "YOLOv5LVISV1Dataset" if lvis else "WeCocoDataset"
    opts = [f"test_dataloader.dataset.dataset.type={ds}", f"test_dataloader.dataset.dataset.data_root={tmp_path}/",
            f"test_dataloader.dataset.dataset.ann_file={ann_path}",
            f"test_dataloader.dataset.dataset.data_prefix.img={'' if lvis else 'val'}",
            f"test_dataloader.dataset.class_text_path={texts_path}", "test_dataloader.batch_size=4",
            f"test_evaluator.type={'LVISMetric' if lvis else 'CocoMetric'}", f"test_evaluator.ann_file={ann_path}"]
    got = {}
    for loader in ("serial", "stream"):
        out, wd = str(tmp_path / f"preds_{loader}.pkl"), str(tmp_path / f"wd_{loader}")
        cmd = [sys.executable, os.path.join(ROOT, "test.py"), os.path.join(ROOT, "config", "wedetect_tiny.py"), ckpt,
               "--text-bank", bank_path, "--out", out, "--work-dir", wd, "--loader", loader, "--decode-workers", "4",
               "--cfg-options", *opts]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        got[loader] = (pickle.load(open(out, "rb")), json.load(open(os.path.join(wd, "metrics.json"))))
    (pa, ma), (pb, mb) = got["serial"], got["stream"]
    assert ma == mb
    assert [q["img_id"] for q in pa] == [q["img_id"] for q in pb] == [im["id"] for im in ann["images"]]
    for a, b in zip(pa, pb):
        assert a["img_path"] == b["img_path"]
        for key in ("bboxes", "scores", "labels"):
            x, y = a["pred_instances"][key], b["pred_instances"][key]
            assert x.dtype == y.dtype and torch.equal(x, y), key
    assert sum(len(q["pred_instances"]["scores"]) for q in pb) > 0
