"""The grouped step under the happens-before checker (GPU, tests/hazards.py with the wrappers of wedetect_amd/groups.py declared by
tests/groups_hazards.py): different batches back to back with overlap_post=True and one in-line step behind them — every
conflicting pair of launches on different streams is ordered.  The pair to look at: the class scores, written by the score launch
of a step (nh stream) and read by the previous step's top-k on the post stream."""
import pytest
import torch

import tests.groups_hazards  # noqa: F401
from tests import groups_ref as GR
from tests import hazards as H
from tests.test_gpu_best_detect import _meta
from tests.test_gpu_hazards import _bank, _batches, _clean, _configure, _names, _stream_of_batches, _streams
from tests.test_gpu_network import build

pytestmark = pytest.mark.gpu

B, HW = 2, 160


@pytest.mark.parametrize("sizes,fused", [(GR.K352, True), (GR.K352, False), (GR.ONE_BIN, False)])
def test_in_line_and_pipelined_grouped_steps_are_ordered(sizes, fused):
    """The fused launch, the default two launches on the fp16x3 path (the score block in ``self.scores`` is scratch of the nh
    stream), and a bank below 256 rows (wd_conv_gemm blocks)."""
    from wedetect_amd.groups import PromptGroups
    _, t, _ = build("tiny", B, HW, num_prompts=48, precision="fp16x3", max_classes=80)
    t.group_fused = fused
    pg = PromptGroups.from_sizes(sizes)
    meta, batches, text = _meta(t), _batches(B, HW, n=4), pg.pad_bank(_bank(pg.P))
    kw = dict(normalize_text=True, score_thr=0.3, iou_thr=0.7, with_embed=True, nms="mmcv", prompt_groups=pg)
    _configure(t, depth="2")
    t.detect(batches[0], text, meta, **kw)                       # warm: weights split, lazily sized buffers exist
    torch.cuda.synchronize()
    names = lambda: {**_names(t)(), "group_out": t._group_out, "group_of": pg.device(t.dev)[1], "bin_first": pg.device(t.dev)[2]}
    with H.track(names, _streams(t)) as tr:
        got, last = _stream_of_batches(t, batches, [text], meta, **kw)
    assert t.post_stream is not None and t._nh_stream is not None
    want = "groups.group_similarity_split" if fused else "groups.group_rows"
    assert tr.calls.get(want, 0) == 5 and tr.calls.get("lib.topk_candidates", 0) == 5 and tr.calls.get("lib.nms_gather", 0) == 5
    assert "fold.fold_similarity" not in tr.calls
    assert tr.calls.get("lib.similarity_split", 0) == (5 if not fused and pg.K_pad >= t.SIM_SPLIT_MIN else 0)
    # the class scores are written on the stream of the head and read on the post stream
    streams = {name: {s for n, s, _, _ in tr.model.launches if n == name} for name in (want, "lib.topk_candidates")}
    assert streams[want] == {t._nh_stream.cuda_stream, torch.cuda.current_stream().cuda_stream}
    assert streams["lib.topk_candidates"] == {t.post_stream.cuda_stream, torch.cuda.current_stream().cuda_stream}
    for g in got:
        assert not bool(g["range_flags"].any())
    _clean(tr)
    # the checker does report the pair when the wait that orders it is left out of the model
    with H.track(names, _streams(t), ignore_wait=lambda ev: ev is t._post_done) as tr2:
        _stream_of_batches(t, batches[:2], [text], meta, **kw)
    hz = tr2.hazards()
    assert any("group_out" in h.buffer and "lib.topk_candidates" in h.first + h.second for h in hz), H.format_hazards(hz)
