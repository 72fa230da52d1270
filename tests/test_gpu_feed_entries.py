"""eval_recall/eval_recall.py end to end with ``--loader stream`` (GPU): one rank over RCCL, batch 2 with a ragged tail, the
set-up of tests/test_gpu_entry.py::test_eval_recall_entry.  The streamed run must print exactly the AR@100 / AR@300 of the
serial run: the proposals are the same bits, so the evaluator sees the same boxes.
"""
from __future__ import annotations

import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_recall_stream_loader_equals_serial_loader(tmp_path, monkeypatch):
    from PIL import Image
    import generate_proposal as gp
    from wedetect_amd import detector as D
    from wedetect_amd import weights as W
    monkeypatch.setattr(gp, "model_size_of", lambda p: "nano")
    monkeypatch.setitem(D._IMG_SIZE, "nano", (128, 128))
    sd = {k: torch.from_numpy(v) for k, v in W.to_uni_keys(W.make_state_dict("nano", num_prompts=256)).items()}
    uni = str(tmp_path / "wedetect_base_uni.pth")
    torch.save(sd, uni)
    g = np.random.default_rng(18)
    sizes = [(120, 200), (128, 64), (90, 90), (128, 128), (64, 100)]
    (tmp_path / "imgs").mkdir()
    images = []
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(tmp_path / "imgs" / f"{i}.png"))
        images.append(dict(id=500 + i, file_name=f"{i}.png"))
    model = gp.load_uni_detector(uni)
    anns = []
    for i, im in enumerate(images):
        if i == 3:
            continue                                                           # an image without ground truth
        bx = model([str(tmp_path / "imgs" / im["file_name"])])[0]["bboxes"].cpu().numpy()
        x1, y1, x2, y2 = [float(v) for v in bx[min(7, len(bx) - 1)]]
        anns.append(dict(image_id=im["id"], bbox=[x1, y1, x2 - x1, y2 - y1], iscrowd=0))            # exactly one proposal
        anns.append(dict(image_id=im["id"], bbox=[1.0, 2.0, 30.0, 25.0], iscrowd=0))
    (tmp_path / "ann.json").write_text(json.dumps(dict(images=images, annotations=anns)))
    spec = importlib.util.spec_from_file_location("eval_recall_feed_entry", os.path.join(ROOT, "eval_recall", "eval_recall.py"))
    er = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(er)
    monkeypatch.setattr(er, "load_uni_detector", gp.load_uni_detector)
    built = []
    real = torch.utils.data.DataLoader
    monkeypatch.setattr(torch.utils.data, "DataLoader", lambda *a, **kw: built.append(1) or real(*a, **kw))
    out = {}
    for loader, port in (("serial", "29543"), ("stream", "29544")):
        for k, v in dict(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0").items():
            monkeypatch.setenv(k, v)
        before = len(built)
        out[loader] = er.main(["--wedetect_uni_checkpoint", uni, "--dataset", "coco", "--batch-size", "2", "--num-workers", "0",
                               "--ann-path", str(tmp_path / "ann.json"), "--image-path", str(tmp_path / "imgs"),
                               "--loader", loader, "--decode-workers", "2"])
        assert len(built) - before == (1 if loader == "serial" else 0)        # the streamed run builds no DataLoader (and no bar)
    print(f"AR@100 / AR@300: serial {out['serial']}, stream {out['stream']}")
    assert out["serial"] == out["stream"]
    assert 0.4 <= out["stream"][1] <= 1.0                                      # the planted boxes are recalled at every IoU
