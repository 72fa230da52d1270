"""The sparse step under the happens-before checker (GPU, tests/hazards.py with the wrappers of wedetect_amd/sparse.py declared
by tests/sparse_hazards.py): different batches back to back with overlap_post=True and one in-line step behind them — every
conflicting pair of launches on different streams is ordered.  The pair to look at: the memset of the counters at the head of a
step (nh stream) against the previous step's wd_sparse_select, which reads them on the post stream.  (The checker found one
while this mode was built: ``sparse_seen`` was first returned as a view of the counters, which the next step's producers clear
ahead of its post-process — a caller's read on the post stream raced with that memset.  It is a copy made by the post-process now.)"""
import pytest
import torch

import tests.sparse_hazards  # noqa: F401
from tests import hazards as H
from tests.test_gpu_best_detect import _meta
from tests.test_gpu_hazards import _bank, _batches, _clean, _configure, _names, _stream_of_batches, _streams
from tests.test_gpu_network import build
from tests.test_gpu_sparse_detect import _threshold

pytestmark = pytest.mark.gpu

B, HW = 2, 160


@pytest.mark.parametrize("k,precision", [(300, "fp16x3"), (80, "fp16x3")])
def test_in_line_and_pipelined_sparse_steps_are_ordered(k, precision):
    _, t, _ = build("tiny", B, HW, num_prompts=48, precision=precision, max_classes=80)
    meta, batches, text = _meta(t), _batches(B, HW, n=4), _bank(k)
    thr, _ = _threshold(t, batches, text)                        # from the dense scores: no list overflows
    kw = dict(normalize_text=True, score_thr=thr, iou_thr=0.7, with_embed=True, nms="mmcv", sparse_scores=True, sparse_cap=32768)
    _configure(t, depth="2")
    t.detect(batches[0], text, meta, **kw)                       # warm: weights split, lazily sized buffers exist
    torch.cuda.synchronize()
    names = lambda: {**_names(t)(), "sparse_list": t._sparse_list, "sparse_state": t._sparse_state, "sparse_status": t._sparse_status,
                     "sparse_seen": t._sparse_seen}
    with H.track(names, _streams(t)) as tr:
        got, last = _stream_of_batches(t, batches, [text], meta, **kw)
    assert t.post_stream is not None and t._nh_stream is not None
    want = "sparse.sparse_similarity_split" if k >= t.SIM_SPLIT_MIN else "sparse.sparse_rows"
    assert tr.calls.get(want, 0) == 5 and tr.calls.get("sparse.sparse_select", 0) == 5 and tr.calls.get("lib.nms_gather", 0) == 5
    assert "lib.topk_candidates" not in tr.calls and "fold.fold_similarity" not in tr.calls
    # the counters are cleared on the stream of the producers and read on the post stream
    streams = {name: {s for n, s, _, _ in tr.model.launches if n == name} for name in (want, "sparse.sparse_select")}
    assert streams[want] == {t._nh_stream.cuda_stream, torch.cuda.current_stream().cuda_stream}
    assert streams["sparse.sparse_select"] == {t.post_stream.cuda_stream, torch.cuda.current_stream().cuda_stream}
    for g in got:
        assert g["sparse_status"].tolist() == [0, 0] and not bool(g["range_flags"].any())
    _clean(tr)
    # the checker does report the pair when the wait that orders it is left out of the model
    with H.track(names, _streams(t), ignore_wait=lambda ev: ev is t._post_done) as tr2:
        _stream_of_batches(t, batches[:2], [text], meta, **kw)
    hz = tr2.hazards()
    assert any("sparse_state" in h.buffer and "sparse.sparse_select" in h.first + h.second for h in hz), H.format_hazards(hz)
