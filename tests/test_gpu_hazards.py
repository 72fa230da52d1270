"""The cross-stream schedules of ImageTower.detect(overlap_post=True) under the happens-before checker (tests/hazards.py), at
the smallest towers of tests/test_gpu_network.py.  Nothing here depends on size or timing: every launch's reads and writes
are recorded with its stream, the order is rebuilt from the Event / Stream calls the engine makes, and every conflicting pair
must be ordered.  An audit first ties the ACCESS table to what the kernels really change on the engine's own calls; the
sensitivity cases then remove one wait at a time FROM THE MODEL ONLY (the device still waits) and demand that the checker
names the buffer that wait protects — a mutation that reported nothing would mean the clean runs prove nothing there."""
import re

import pytest
import torch

from tests import hazards as H
from tests.test_gpu_network import build

pytestmark = pytest.mark.gpu

KW = dict(normalize_text=False, score_thr=0.0, with_embed=True)


def _batches(b, hw, n=6, seed=950):
    from wedetect_amd import weights as W
    return [torch.from_numpy(W.make_images(b, hw, hw, seed=seed + i)).cuda() for i in range(n)]


def _bank(k, seed=4321):
    from wedetect_amd import weights as W
    return torch.from_numpy(W.make_text_bank(k, seed=seed)).cuda()


def _names(t):
    """label -> tensor, evaluated when a report is written (the pipeline's buffer sets appear with the first pipelined step)."""
    def names():
        d = {"scores": t.scores, "boxes": t.boxes, "embed": t._embed, "embed_s": t.embed_s, "tmp": t.tmp, "hid": t.hid,
             "ln_part": t.ln_part, "ln_stats": t.ln_stats, "patches": t.patches, "park": t.park, "kws": t.kws, "fws": t.fws,
             "range_flags": t.range_flags, "text_norm": t.text_norm, "topk_ws": t.topk_ws, "nms_ws": t.nms_ws,
             "cand_idx": t.cand_idx, "cand_score": t.cand_score, "cand_count": t.cand_count, "out_boxes": t.out_boxes,
             "out_scores": t.out_scores, "out_labels": t.out_labels, "out_anchors": t.out_anchors, "out_count": t.out_count,
             "out_embed": t.out_embed, "kept_g": t._kept_g, "kept_t": t._kept_t, "kept_s": t._kept_s, "kept_es": t._kept_es,
             "kept_perm": t._kept_perm}
        for a in ("cat_n4", "cat_b0", "b0_t", "f0", "f_out0", "cat_n3", "cat_b1", "b1_t", "f1", "p3", "p4", "p5"):
            d[a] = getattr(t, a)
        for name, bf in t._bep.items():
            for k, v in bf.items():
                if isinstance(v, torch.Tensor):
                    d[f"{name}.{k}"] = v
        for l in range(3):
            d.update({f"hc{l}.c1": t.hc[l][0], f"hc{l}.c2": t.hc[l][1], f"hr{l}.r1": t.hr[l][0], f"hr{l}.r2": t.hr[l][1], f"hr{l}.dist": t.hr[l][2]})
        for j, xs in enumerate(t._x_sets or [t.x]):
            for i, x in enumerate(xs):
                d[f"c{i + 1}.set{j}"] = x
        for k, v in (t._slot1 or {}).items():
            if isinstance(v, torch.Tensor):
                d[f"slot1.{k}"] = v
        for i, (_, _, _, ent) in enumerate(t._text_fold):
            d.update({f"fold{i}.w0": ent["w"][0], f"fold{i}.w1": ent["w"][1], f"fold{i}.w2": ent["w"][2], f"fold{i}.b": ent["b"],
                      f"fold{i}.u": ent["u"], f"fold{i}.tn": ent["tn"]})
        return d
    return names


def _streams(t):
    def streams():
        d = {"post": t.post_stream, "nh": t._nh_stream, "bb2": (t._slot1 or {}).get("stream")}
        d.update({f"lane{i + 1}": s for i, s in enumerate(t._side)})
        d.update({f"chain{i + 1}": s for i, s in enumerate(t._chain_streams)})
        return d
    return streams


def _warm(t, x, text, meta, **kw):
    """One in-line step before tracking: weights are split and lazily sized buffers exist, so the tracked region is the
    schedule itself (the first use of a weight reads max |w| on the host, which would order everything around it)."""
    t.detect(x, text, meta, **{**KW, **kw})
    torch.cuda.synchronize()


def _stream_of_batches(t, batches, texts, meta, between=None, **kw):
    """Different batches back to back with no host synchronisation, the results cloned on the post stream, then one in-line
    step right behind — the form of the bit-identity tests of tests/test_gpu_network.py."""
    kw = {**KW, **kw}
    got = []
    for i, x in enumerate(batches):
        r = t.detect(x, texts[i % len(texts)], meta, overlap_post=True, **kw)
        with torch.cuda.stream(t.post_stream):
            got.append({k: v.clone() for k, v in r.items()})
            got[-1]["range_flags"] = t.step_range_flags.clone()      # as the detectors stage the step's flags: on the post stream
        if between is not None:
            between(i, r)
    r = t.detect(batches[0], texts[0], meta, **kw)
    t.wait_post()
    torch.cuda.synchronize()
    return got, r


def _clean(tr, min_launches=500):
    assert len(tr.model.launches) >= min_launches, f"only {len(tr.model.launches)} launches were seen"
    assert len({s for _, s, _, _ in tr.model.launches}) >= 2, "everything ran on one stream: nothing was checked"
    hz = tr.hazards()
    assert hz == [], H.format_hazards(hz)


def _configure(t, *, pipe_neck="1", depth="1", dag=True, dag_on_nh=False, chains="1"):
    t.bb_chains, t.pipe_neck, t.dag, t.bb_depth = str(chains), pipe_neck, dag, str(depth)
    t._dag_forced = dag_on_nh            # $WEDETECT_DAG=1: the side lanes under the nh stream too


# ---------------------------------------------------------------------------------------------------------------------
# the audit: ACCESS against what the kernels change, on the engine's real calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,b,hw,precision,fold,with_embed", [
    ("tiny", 3, 128, "fp32", False, True), ("tiny", 3, 128, "fp16x3", False, True), ("tiny", 3, 128, "fp16x3", True, True),
    ("base", 2, 320, "fp16x3", True, False), ("base", 2, 320, "fp16x3", False, True), ("base", 2, 320, "fp32", False, True)])
def test_audit_access_table_against_the_kernels(arch, b, hw, precision, fold, with_embed):
    """One in-line step on a cold tower with a device synchronise around every launch: operands declared R keep their bits,
    and of the operands declared W nothing changes outside the declared rectangles (workspaces are declared whole)."""
    _, t, imgs = build(arch, b, hw, num_prompts=48, precision=precision)
    t.fold_text = fold
    x, meta = torch.from_numpy(imgs).cuda(), t.identity_meta()
    big = _bank(300)                     # a bank the fp16x3 similarity kernel scores (SIM_SPLIT_MIN rows and more)
    with H.track(audit=True) as tr:
        t.detect(x, t.P["prompts"], meta, normalize_text=False, score_thr=0.0, with_embed=with_embed)
        t.detect(x, big, meta, normalize_text=True, score_thr=0.0, with_embed=with_embed)
        per_image = torch.stack([t.P["prompts"][:40]] * b).contiguous()
        t.detect(x, per_image, meta, normalize_text=True, score_thr=0.0, with_embed=with_embed,
                 text_counts=torch.full((b,), 33, dtype=torch.int32, device="cuda"))
    assert tr.mismatches == [], tr.mismatches[:8]
    assert tr.audited > 300
    need = {"lib.conv_gemm", "lib.topk_candidates", "lib.nms_gather", "lib.dfl_decode", "lib.similarity_grouped", "lib.l2norm_rows"}
    if precision == "fp16x3":
        need |= {"lib.split_weights"}
    if fold:
        need |= {"fold.fold_similarity", "fold.kept_rows_gather", "fold.kept_rows_reorder", "lib.split_weights_scaled"}
    assert need <= set(tr.calls), sorted(need - set(tr.calls))


# ---------------------------------------------------------------------------------------------------------------------
# the schedules of the tower
# ---------------------------------------------------------------------------------------------------------------------
SCHEDULES = {
    "1-post-stream-only": dict(pipe_neck="0"),
    "2-nh-depth1-dag": dict(pipe_neck="1", depth="1", dag=True, dag_on_nh=True),
    "3-nh-depth1-serial": dict(pipe_neck="1", depth="1", dag=False),
    "4-depth2": dict(pipe_neck="1", depth="2", dag=True),
    "4-depth2-dag-on-nh": dict(pipe_neck="1", depth="2", dag=True, dag_on_nh=True),
}


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("arch,b,hw", [("tiny", 3, 128), ("base", 2, 320)])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_schedule_is_ordered(schedule, arch, b, hw, precision):
    """Scenarios 1-4 in both arithmetic modes (fp16x3 towers run the folded bank by default, fp32 towers the unfolded step)."""
    _, t, _ = build(arch, b, hw, num_prompts=48, precision=precision)
    meta, batches = t.identity_meta(), _batches(b, hw)
    _configure(t, **SCHEDULES[schedule])
    _warm(t, batches[0], t.P["prompts"], meta)
    with H.track(_names(t), _streams(t)) as tr:
        _stream_of_batches(t, batches, [t.P["prompts"]], meta)
    assert t.post_stream is not None and (SCHEDULES[schedule]["pipe_neck"] == "0") == (t._nh_stream is None)
    assert SCHEDULES[schedule].get("depth") != "2" or t._slot1 is not None
    _clean(tr)


@pytest.mark.parametrize("arch,b,hw,chains,depth", [("tiny", 4, 128, 2, 1), ("tiny", 4, 128, 2, 2), ("base", 4, 256, 4, 1)])
def test_forced_image_chains_are_ordered(arch, b, hw, chains, depth):
    """Scenario 5: the backbone as 2 / 4 image chains on their own streams (under depth 2 on slot 0 only)."""
    _, t, _ = build(arch, b, hw, num_prompts=48, precision="fp16x3")
    meta, batches = t.identity_meta(), _batches(b, hw)
    _configure(t, depth=str(depth), chains=str(chains))
    assert t._n_chains() == chains
    _warm(t, batches[0], t.P["prompts"], meta)
    with H.track(_names(t), _streams(t)) as tr:
        _stream_of_batches(t, batches, [t.P["prompts"]], meta)
    assert len(t._chain_streams) == chains - 1
    _clean(tr)


@pytest.mark.parametrize("depth", [1, 2])
def test_latency_split_k_class_is_ordered(depth):
    """Scenario 6: split_k=True — every lane and both backbones in flight need split-K workspaces of their own."""
    _, t, _ = build("base", 1, 320, num_prompts=48, precision="fp16x3", split_k=True)
    meta, batches = t.identity_meta(), _batches(1, 320)
    _configure(t, depth=str(depth))
    _warm(t, batches[0], t.P["prompts"], meta)
    with H.track(_names(t), _streams(t)) as tr:
        _stream_of_batches(t, batches, [t.P["prompts"]], meta)
    assert t.kws is not None
    _clean(tr, min_launches=300)


@pytest.mark.parametrize("banks,k,with_embed", [(1, 80, True), (1, 80, False), (1, 300, True), (2, 80, True), (3, 81, True)])
def test_folded_bank_is_ordered(banks, k, with_embed):
    """Scenarios 7-9: the bank folded into the embedding conv on the caller's stream, read on nh and post — one bank (also one
    the fp16x3 similarity kernel re-scores), two banks alternating between steps, three banks so that every step evicts a fold
    entry that the post stream of the step before may still read."""
    _, t, _ = build("tiny", 3, 128, num_prompts=48, precision="fp16x3", max_classes=300)
    meta, batches = t.identity_meta(), _batches(3, 128)
    texts = [_bank(k, seed=4321 + i) for i in range(banks)]
    _configure(t, depth="2")
    _warm(t, batches[0], texts[0], meta, normalize_text=True, with_embed=with_embed)
    folds = t.fold_launches
    with H.track(_names(t), _streams(t)) as tr:
        _stream_of_batches(t, batches, texts, meta, normalize_text=True, with_embed=with_embed)
    assert t.fold_launches - folds == (0 if banks == 1 else 1 if banks == 2 else 6) and tr.calls.get("fold.fold_similarity", 0) >= 21
    _clean(tr)


def test_range_flag_ring_comes_round_behind_the_copies_of_its_previous_steps():
    """Every pipelined step stores its sticky range flags into the next pair of a ring and the caller copies that pair on the
    post stream beside the following steps: eleven steps, more than ImageTower.FLAG_RING, so that pairs are taken a second
    time — the stores of the later step must be ordered behind the copy of the earlier one, in every schedule depth."""
    _, t, _ = build("tiny", 3, 128, num_prompts=48, precision="fp16x3")
    meta, batches = t.identity_meta(), _batches(3, 128)
    assert t.FLAG_RING < 11
    for depth, pipe in (("2", "1"), ("1", "1"), ("1", "0")):
        _configure(t, depth=depth, pipe_neck=pipe)
        _warm(t, batches[0], t.P["prompts"], meta)
        with H.track(_names(t), _streams(t)) as tr:
            got, _ = _stream_of_batches(t, (batches * 2)[:11], [t.P["prompts"]], meta)
        assert len({g["range_flags"].data_ptr() for g in got}) == 11 and not bool(t.range_flags.any())
        _clean(tr)


def test_per_image_banks_are_ordered():
    """Scenario 10: one bank per image with device-side counts (wd_similarity_grouped on the nh stream)."""
    _, t, _ = build("tiny", 3, 128, num_prompts=48, precision="fp16x3")
    meta, batches = t.identity_meta(), _batches(3, 128)
    texts = [torch.stack([_bank(40, seed=s + i) for i in range(3)]).contiguous() for s in (100, 200)]
    counts = torch.tensor([40, 7, 33], dtype=torch.int32, device="cuda")
    _configure(t, depth="2")
    _warm(t, batches[0], texts[0], meta, normalize_text=True, text_counts=counts)
    with H.track(_names(t), _streams(t)) as tr:
        _stream_of_batches(t, batches, texts, meta, normalize_text=True, text_counts=counts)
    assert tr.calls.get("lib.similarity_grouped", 0) == 7
    _clean(tr)


def test_checked_counts_between_steps_is_ordered():
    """A host synchronisation in the middle of the stream: checked_counts reads the kept-row counts and the range flags."""
    _, t, _ = build("tiny", 3, 128, num_prompts=48, precision="fp16x3")
    meta, batches = t.identity_meta(), _batches(3, 128)
    _configure(t, depth="2")
    _warm(t, batches[0], t.P["prompts"], meta)
    seen = []
    with H.track(_names(t), _streams(t)) as tr:
        _stream_of_batches(t, batches, [t.P["prompts"]], meta,
                           between=lambda i, r: seen.append(t.checked_counts(r, lambda: None)) if i in (1, 2, 4) else None)
    assert len(seen) == 3 and not t.overflowed
    _clean(tr)


def test_captured_step_with_the_dag_in_capture_is_ordered():
    """GraphedDetect's warm-up steps on its side stream and the capture pass itself (the neck / head DAG forks inside the
    capture), tracked while they are issued."""
    from wedetect_amd.engine import GraphedDetect
    _, t, _ = build("tiny", 3, 128, num_prompts=48, precision="fp16x3")
    batches = _batches(3, 128, n=1)
    t.dag, t._dag_forced, t._dag_in_capture = True, True, True
    _warm(t, batches[0], t.P["prompts"], t.identity_meta())
    with H.track(_names(t), _streams(t)) as tr:
        g = GraphedDetect(t, 48, normalize_text=False, score_thr=0.0, with_embed=True)
        torch.cuda.synchronize()
    assert g.graph is not None and len(t._side) == 3
    _clean(tr, min_launches=200)


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: one wait left out of the model at a time
# ---------------------------------------------------------------------------------------------------------------------
C_SET = re.compile(r"\bc[1-4]\.set\d")
MUTATIONS = {
    "post_done": (lambda t: (lambda ev: ev is t._post_done), re.compile(r"\b(boxes|scores|embed)\b")),
    "x_free": (lambda t: (lambda ev: any(ev is e for e in t._x_free)), C_SET),
    "bb_done": (lambda t: (lambda ev: any(ev is e for e in t._bb_done)), C_SET),
    "slot1_ready": (lambda t: (lambda ev: t._slot1 is not None and ev is t._slot1["ready"]), re.compile(r"\bslot1\.img\b")),
    "post_ready": (lambda t: (lambda ev: ev is t._post_ready), re.compile(r"\bscores\b")),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_wait_left_out_of_the_model_is_reported_with_the_buffer_it_protects(mutation):
    """The depth-2 schedule (for post_ready: the same, whose fp16x3 step is the folded one) with one family of waits invisible
    to the model.  The device runs exactly what the clean test runs."""
    pred, expect = MUTATIONS[mutation]
    _, t, _ = build("tiny", 3, 128, num_prompts=48, precision="fp16x3")
    meta, batches = t.identity_meta(), _batches(3, 128)
    _configure(t, depth="2")
    _warm(t, batches[0], t.P["prompts"], meta)
    with H.track(_names(t), _streams(t), ignore_wait=pred(t)) as tr:
        _stream_of_batches(t, batches, [t.P["prompts"]], meta)
    hz = tr.hazards()
    assert tr.calls.get("fold.fold_similarity", 0) >= 21, "the fp16x3 steps of this schedule are the folded ones"
    assert tr.ignored_waits > 0, "the mutation matched no wait"
    assert hz, f"{mutation}: the model is blind to this wait"
    assert any(expect.search(h.buffer) for h in hz), H.format_hazards(hz)


# ---------------------------------------------------------------------------------------------------------------------
# schedules above the tower: the streamed feed, the tiled path, the flipped-view path
# ---------------------------------------------------------------------------------------------------------------------
def _detector_names(m, extra=None):
    def names():
        d = {}
        for key, t in m._h._towers.items():
            d.update({f"{key}:{k}": v for k, v in _names(t)().items()})
        for k, v in (extra() if extra else {}).items():
            if isinstance(v, torch.Tensor) and v.is_cuda:
                d[k] = v
        return d
    return names


def _detector_streams(m, extra=None):
    def streams():
        d = dict(extra() if extra else {})
        for t in m._h._towers.values():
            d.update(_streams(t)())
        return d
    return streams


def test_streamed_feed_is_ordered(tmp_path):
    """predict_stream on the tiny config, seven images in batches of four (a batch of four and a tail of three): the up / down
    streams with ev_up / ev_free / ev_staged / ev_d2h around the pipelined tower steps.  The decode workers' writes into the
    PINNED arenas are host writes and outside the model (only their ev_up.synchronize() is seen); the H2D copies that read
    those arenas are modelled as writes of their device destinations."""
    from tests.test_gpu_feed import _detector, _pipeline_cfg, _write_images
    names = [f"class {k}" for k in range(20)]
    infos = [dict(img_id=100 + k, img_path=p, texts=[[n] for n in names]) for k, p in enumerate(_write_images(tmp_path, 7))]
    pipeline, m = _pipeline_cfg("tiny"), _detector("tiny", "fp16x3", names)
    warm = list(m.predict_stream(infos, 4, pipeline, decode_workers=2))      # calibrates, builds the towers, splits the weights
    torch.cuda.synchronize()
    with H.track(_detector_names(m), _detector_streams(m)) as tr:
        stats = {}
        got = list(m.predict_stream(infos, 4, pipeline, decode_workers=2, stats=stats))
        torch.cuda.synchronize()
    assert len(got) == len(warm) == 7 and stats["batches"] == 2 and stats["inline_batches"] == 0
    assert tr.calls.get("feed.feed_batch_u8", 0) == 2 <= stats["feed_launches"]
    assert len({s for _, s, _, _ in tr.model.launches}) >= 5      # caller, up, down, post, nh (and the second backbone stream)
    _clean(tr, min_launches=300)


def test_tiled_detector_path_is_ordered():
    """predict_tiled (tests/test_gpu_tile.py's sizes: a 96 x 160 image as 8 crops + overview in steps of 4 + 4 + 1): each step's
    rows are stacked on the tower's post stream behind an event of their own, the merge waits for all of them."""
    from tests.test_gpu_tile import TILE, _nano, _smooth_image
    img, m = _smooth_image(96, 160, seed=7), _nano("fp16x3")
    kw = dict(tile=TILE, overlap=0.5, overview=True, tile_batch=4, edge_margin=0.0)
    m.predict_tiled(img, **kw)
    buffers = lambda: {f"tiled.{k}": v for k, v in m._tiled.items()}
    with H.track(_detector_names(m, buffers), _detector_streams(m)) as tr:
        stats = {}
        got = m.predict_tiled(img, stats=stats, **kw)
    assert stats["steps"] == 3 and stats["trips"] == 0 and not stats["inline"] and len(got.pred_instances.scores) >= 10
    assert tr.calls.get("tile.tile_cut_u8") == 1 and tr.calls.get("tile.tile_merge") == 1
    _clean(tr, min_launches=200)


def test_flipped_view_path_is_ordered():
    """predict_views (tests/test_gpu_views.py's sizes: two scales x flip, B = 2 — four views on two towers): every view's rows
    stacked on its tower's post stream, one merge behind the views' events."""
    from tests.test_gpu_views import TTA_CFG, _fresh, _items, _tta_pipeline, _views_of
    from tests.test_gpu_tile import _nano
    m = _nano("fp16x3")
    views, _ = _views_of(_items(_tta_pipeline((64, 96)), 2))
    m.predict_views(_fresh(views), TTA_CFG)
    buffers = lambda: {f"views.{k}": v for k, v in m._views.items()}
    with H.track(_detector_names(m, buffers), _detector_streams(m)) as tr:
        stats = {}
        got = m.predict_views(_fresh(views), TTA_CFG, stats=stats)
    assert stats == dict(views=4, steps=4, trips=0, inline=False, d2h_copies=1) and len(got) == 2
    assert tr.calls.get("views.views_merge") == 1 and tr.calls.get("lib.chw_to_hwc_u8") == 4
    _clean(tr, min_launches=200)
