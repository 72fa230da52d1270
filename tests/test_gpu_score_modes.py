"""The class-chunk boundary of the materialised score paths (GPU): a bank of ROWS_CHUNK + 8 rows is cut into a block of 4096
columns and one of 8 (``c0`` = 4096), (a) as per-image banks with counts [ROWS_CHUNK + 3, 5] — image 0 crosses the cut, image 1 lies
wholly in the first block, so its count of the second block clamps to 0 — and (b) as one shared bank on an fp32 tower.  The sparse
step must be the dense step of the same tower, field for field and bit for bit, and the best-class step tests/best_ref.py on the
dense step's own scores.  Tiny tower, 2 x 160 x 160: 525 anchors per image, text fold off; the largest tensor is 2 x 525 x 4104 floats."""
import pytest
import torch

import tests.best_hazards  # noqa: F401
import tests.sparse_hazards  # noqa: F401
from tests.test_gpu_best_detect import THR, _check, _materialised, _meta
from tests.test_gpu_hazards import _bank
from tests.test_gpu_sparse_detect import FIELDS, IOU, _snap, _threshold, _tower
from wedetect_amd import best as BS
from wedetect_amd import sparse as SP

pytestmark = pytest.mark.gpu

K = SP.ROWS_CHUNK + 8


def _banks(case):
    if case == "per_image":
        text = torch.stack([_bank(K, seed=100), _bank(K, seed=200)]).contiguous()
        return "fp16x3", text, torch.tensor([SP.ROWS_CHUNK + 3, 5], dtype=torch.int32, device="cuda")
    return "fp32", _bank(K), None


@pytest.mark.parametrize("case", ["per_image", "shared_fp32"])
def test_sparse_and_best_class_steps_across_a_chunk_boundary_equal_the_dense_step(case):
    assert BS.ROWS_CHUNK == SP.ROWS_CHUNK and K > SP.ROWS_CHUNK
    precision, text, counts = _banks(case)
    t, x = _tower(precision)
    meta = _meta(t)
    thr, seen = _threshold(t, [x], text, want=10000, counts=counts)
    kw = dict(normalize_text=True, iou_thr=IOU, with_embed=True, nms="mmcv", text_counts=counts)
    dense = _snap(t.detect(x, text, meta, score_thr=thr, **kw))
    calls = []
    real_s, real_b = SP.sparse_rows, BS.best_rows
    SP.sparse_rows = lambda *a, **kw_: (calls.append(("sparse", a[3], a[10])), real_s(*a, **kw_))[1]      # (n_cls, cls_offset)
    BS.best_rows = lambda *a, **kw_: (calls.append(("best", a[3], a[6])), real_b(*a, **kw_))[1]
    try:
        sparse = _snap(t.detect(x, text, meta, score_thr=thr, sparse_scores=True, **kw))
        best = _snap(t.detect(x, text, meta, score_thr=THR, best_class=True, **kw))
    finally:
        SP.sparse_rows, BS.best_rows = real_s, real_b
    cut = [(SP.ROWS_CHUNK, 0), (8, SP.ROWS_CHUNK)]
    assert calls == [("sparse", *c) for c in cut] + [("best", *c) for c in cut], calls
    for n in FIELDS:
        assert torch.equal(sparse[n], dense[n]), n
    assert sparse["sparse_status"].tolist() == [0, 0] and sparse["sparse_seen"].tolist() == seen
    assert int(dense["count"].min()) > 0 and int(t.range_flags.max()) == 0
    scores, boxes = _materialised(t, x, text, counts)
    _check(case, best, scores, boxes, meta, t, 10000, False, counts=None if counts is None else counts.tolist())
    if counts is not None:
        for name, r in (("dense", dense), ("sparse", sparse), ("best", best)):
            n1 = int(r["count"][1])
            assert n1 > 0 and int(r["labels"][1, :n1].max()) < 5, name
        n0 = int(dense["count"][0])
        assert int(dense["labels"][0, :n0].max()) < SP.ROWS_CHUNK + 3
