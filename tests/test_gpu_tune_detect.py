"""Bank tuning end to end (GPU): a seeded ``tiny`` detector at 64 x 64 (84 anchors), two images, boxes taken from chosen anchors'
decoded boxes — the cached chunk against ``ImageTower.embed`` bit for bit, the first step against tests/tune_ref.py fed the same
cache, 50 steps on the device and in the reference, the tuned bank used like any bank, ``init="exemplar"``, the happens-before
checker."""
import functools

import numpy as np
import pytest
import torch

import tests.tune_hazards  # noqa: F401
from tests import hazards as H
from tests import tune_ref as R
from tests.test_gpu_exemplar_detect import B, HW, META_ROWS, _inputs, _to_original
from tests.test_gpu_tile import NAMES

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
K = 4                                                                          # class 3 has no box: it learns from negatives only
BOX_ANCHORS = [[(9, 0), (70, 1)], [(37, 0), (82, 2), (40, 1)]]                 # (anchor whose decoded box is the label, class) per image
LR, STEPS, M = 2e-3, 50, 4


@functools.lru_cache(maxsize=None)
def _world():
    """The detector, its tower, the decoded boxes of the batch, the labelled boxes, the cache of one tune_bank(fit=False) call (kept
    by the test: the detector's own cache is handed back empty) and the chunk as numpy."""
    from wedetect_amd import weights as W
    from wedetect_amd.detector import YOLOWorldDetector, _nhwc_u8
    m = YOLOWorldDetector("tiny", test_cfg=dict(max_per_img=100), max_classes=len(NAMES))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny").items()})
    m.cuda().eval()
    m.set_text_embeddings(torch.from_numpy(W.make_text_bank(len(NAMES))).cuda(), [[n] for n in NAMES])
    xs, samples = _inputs()
    x = _nhwc_u8(xs, m._h.device)
    tower = m._h.tower(B, HW, HW)
    m._h.calibrate_first(tower, x)
    _, boxes = tower.features(x)
    boxes = boxes.cpu().numpy().copy()
    assert tower.ntot == 84 and tower.off[1] == 64 and tower.off[2] == 80
    labelled = [[(_to_original(boxes[b, a], b).tolist(), c) for a, c in BOX_ANCHORS[b]] for b in range(B)]
    bank0 = torch.from_numpy(W.make_text_bank(K)).cuda()
    assert m.tune_bank(xs, samples, labelled, init=bank0, anchors_per_box=M, fit=False) is None
    tuner, m._tuner = m._tuner, None
    c = tuner.chunks[0]
    torch.cuda.synchronize()
    chunk = dict(E=c["E"].cpu().numpy(), pos_cls=c["pos_cls"].cpu().numpy().reshape(-1), pos_y=c["pos_y"].cpu().numpy().reshape(-1),
                 n_anchor=84, off1=64, off2=80, scale=tower.lvl_scale, bias=tower.lvl_bias, rows=B * 84)
    return m, tower, boxes, labelled, bank0, tuner, chunk


def test_the_cache_is_the_tower_embed_and_the_reference_targets():
    m, tower, boxes, labelled, bank0, tuner, chunk = _world()
    c = tuner.chunks[0]
    assert len(tuner.chunks) == 1 and c["rows"] == B * 84 and tuner.cache_bytes == B * 84 * (768 * 4 + 8)
    assert torch.equal(c["E"].view(B, 84, 768).view(torch.int32), tower.embed.view(torch.int32))          # bit for bit
    from tests import exemplar_ref as XR
    ex = np.zeros((B, 3, 4), f32)
    cls = np.zeros((B, 3), np.int32)
    for b in range(B):
        for e, (bx, k) in enumerate(labelled[b]):
            ex[b, e], cls[b, e] = bx, k
    ra, ri, _ = XR.assign(boxes, ex, [2, 3], META_ROWS, M, 0.1)
    pc, py = R.targets(ra, ri, cls, M, 84)
    assert np.array_equal(chunk["pos_cls"], pc.reshape(-1)) and np.array_equal(chunk["pos_y"].view(np.uint32), py.reshape(-1).view(np.uint32))
    for b in range(B):                                                         # every label owns the anchor it was cut from
        for a, k in BOX_ANCHORS[b]:
            assert pc[b, a] == k and py[b, a] > 0.999
    assert int((pc >= 0).sum()) > 5 and 3 not in pc


def test_step_one_matches_the_reference_on_the_same_cache():
    """Loss within tune_ref.loss_bound; dW per class at the metric of the kernel tests: 8 x the figure of a numpy fp32 evaluation,
    plus 4 * 2^-24 for reading dW back as m / (1 - beta1) after one step."""
    m, tower, boxes, labelled, bank0, tuner, chunk = _world()
    bank, info = tuner.fit(bank0, 1, lr=LR)
    W0 = bank0.cpu().numpy()
    l64, _, dW64, _ = R.loss_grad([chunk], W0.astype(f64))
    _, _, dW32, _ = R.loss_grad([chunk], W0, dtype=f32)
    got = info["m"].cpu().numpy().astype(f64) / (1 - 0.9)
    err, err32 = R.grad_rel_err(got, dW64), R.grad_rel_err(dW32, dW64)
    a, _ = R.row_consts(chunk["rows"], 84, 64, 80, chunk["scale"], chunk["bias"])
    z_err = float((a * np.sqrt((chunk["E"].astype(f64) ** 2).sum(axis=1))).max()) * 101 * 2.0 ** -24
    bound = R.loss_bound(float(l64), chunk["rows"], K, info["plan"][0], info["plan"][0], z_err, 1.0 / info["norm"])
    print(f"loss {info['loss'][0]:.6f} vs {float(l64):.6f} (bound {bound:.2e}); dW kernel {err.max():.2e}, numpy fp32 {err32.max():.2e}")
    assert info["norm"] == pytest.approx(R.norm_of([chunk]), rel=1e-6) and info["status"] == 0
    assert abs(info["loss"][0] - float(l64)) <= bound
    assert bool((err <= 8 * float(err32.max()) + 4 * 2.0 ** -24).all())
    assert info["positives"] == [int((chunk["pos_cls"] == k).sum()) for k in range(K)] and info["no_positive"] == [3]


def test_fifty_steps_lower_the_loss_and_raise_the_labelled_scores():
    m, tower, boxes, labelled, bank0, tuner, chunk = _world()
    bank, info = tuner.fit(bank0, STEPS, lr=LR)
    assert len(info["loss"]) == STEPS and info["status"] == 0 and info["loss"][-1] < info["loss"][0]
    # the reference's own 50 steps in float64
    W, mm, vv = bank0.cpu().numpy().astype(f64), np.zeros((K, 768)), np.zeros((K, 768))
    ref_loss = []
    for t in range(1, STEPS + 1):
        l, _, dW, _ = R.loss_grad([chunk], W)
        ref_loss.append(float(l))
        W, mm, vv, _ = R.adam_step(W, mm, vv, dW, t, LR)
    print(f"device {info['loss'][0]:.5f} -> {info['loss'][-1]:.5f}; reference {ref_loss[0]:.5f} -> {ref_loss[-1]:.5f}")
    assert ref_loss[-1] < ref_loss[0]
    got = bank.cpu().numpy().astype(f64)
    assert float(np.abs(np.sqrt((got * got).sum(axis=1)) - 1).max()) < 1e-6
    # every labelled box's own class scores higher on its anchors than before: the positives whose target lies above their
    # score at the start (a positive that starts above its IoU target is asked to come down) — the anchors the labels were cut
    # from, target ~1, are all among them
    a, b = R.row_consts(chunk["rows"], 84, 64, 80, chunk["scale"], chunk["bias"])
    T0 = bank0.cpu().numpy().astype(f64)
    T0 /= np.sqrt((T0 * T0).sum(axis=1, keepdims=True))
    E = chunk["E"].astype(f64)
    sig = lambda z: 1 / (1 + np.exp(-z))
    rows = np.nonzero(chunk["pos_cls"] >= 0)[0]
    before = sig(a[rows] * (E[rows] * T0[chunk["pos_cls"][rows]]).sum(axis=1) + b[rows])
    after = sig(a[rows] * (E[rows] * got[chunk["pos_cls"][rows]]).sum(axis=1) + b[rows])
    asked_up = chunk["pos_y"][rows] > before
    assert bool((after[asked_up] > before[asked_up]).all())
    for bi in range(B):
        for an, _ in BOX_ANCHORS[bi]:
            assert bool(asked_up[list(rows).index(bi * 84 + an)])


def test_the_tuned_bank_is_used_like_any_bank_and_exemplar_init_starts_from_the_prototypes():
    m, tower, boxes, labelled, bank0, tuner, chunk = _world()
    xs, samples = _inputs()
    text_bank, texts = m.text_feats.clone(), m.texts
    three = [[(bx, k) for bx, k in lst] for lst in labelled]                    # classes 0, 1, 2: each has a box
    try:
        proto, _ = m.exemplar_bank(xs, samples, three, ["a", "b", "c"], anchors_per_box=M)
        bank, info = m.set_tuned_bank(xs, samples, three, ["a", "b", "c"], init="exemplar", steps=5, lr=LR, anchors_per_box=M)
        assert torch.equal(info["init"].view(torch.int32), proto.view(torch.int32))                       # bit for bit
        assert m._tuner is None and info["names"] == ["a", "b", "c"] and len(info["loss"]) == 5 and info["loss"][-1] < info["loss"][0]
        assert m.texts == [["a"], ["b"], ["c"]] and torch.equal(m.text_feats, bank) and tuple(bank.shape) == (3, 768)
        preds = [s.pred_instances for s in m.predict(*_inputs())]
        assert all(bool(torch.isfinite(p.scores).all()) for p in preds) and int(torch.cat([p.labels for p in preds]).max()) < 3
        # new classes beside frozen text rows: the text rows keep their bits (unit rows in, unit rows out)
        unit = text_bank / text_bank.norm(dim=1, keepdim=True)
        mixed = torch.cat([unit, proto])
        k = unit.shape[0]
        shifted = [[(bx, k + c) for bx, c in lst] for lst in three]
        tuned, info2 = m.tune_bank(xs, samples, shifted, init=mixed, steps=3, lr=LR, frozen_rows=list(range(k)), anchors_per_box=M)
        start = mixed / mixed.norm(dim=1, keepdim=True)                        # fit() normalises every row once, before the steps
        assert torch.equal(tuned[:k].view(torch.int32), start[:k].view(torch.int32)) and not torch.equal(tuned[k:], start[k:])
        assert info2["positives"][:k] == [0] * k and min(info2["positives"][k:]) >= 1
        # two batches before one fit: the second call fits over both chunks
        assert m.tune_bank(xs, samples, three, fit=False) is None and len(m._tuner.chunks) == 1      # the default init: nothing pooled
        m.tune_reset()
        assert m._tuner is None
        assert m.tune_bank(xs, samples, three, init=proto, fit=False) is None and len(m._tuner.chunks) == 1
        with pytest.raises(ValueError, match="gt_boxes|at most 64"):                                 # a call that raises adds nothing
            m.tune_bank(xs, samples, [three[0] * 40, three[1]], init=proto, fit=False)
        assert len(m._tuner.chunks) == 1
        _, info3 = m.tune_bank(xs, samples, three, init=proto, steps=2, lr=LR)
        assert m._tuner is None and len(info3["plan"]) == 2 and info3["positives"] == [2 * n for n in info["positives"]]
    finally:
        m._tuner = None
        m.set_text_embeddings(text_bank, texts)


def test_tune_bank_and_predict_are_ordered_for_the_happens_before_checker():
    m, tower, boxes, labelled, bank0, tuner, chunk = _world()
    xs, samples = _inputs()
    text_bank, texts = m.text_feats.clone(), m.texts
    three = [[(bx, k) for bx, k in lst] for lst in labelled]
    m.tune_bank(xs, samples, three, init="exemplar", steps=1, lr=LR)           # warm: lazily sized buffers exist
    m.predict(*_inputs())
    torch.cuda.synchronize()
    try:
        with H.track() as tr:
            m.set_tuned_bank(xs, samples, three, ["a", "b", "c"], init="exemplar", steps=3, lr=LR)
            m.predict(*_inputs())
            torch.cuda.synchronize()
    finally:
        m.set_text_embeddings(text_bank, texts)
    assert tr.calls.get("tune.tune_targets", 0) == 1 and tr.calls.get("tune.tune_grad", 0) == 3 and tr.calls.get("tune.tune_update", 0) == 3
    assert tr.calls.get("exemplar.exemplar_assign", 0) == 2
    hz = tr.hazards()
    assert hz == [], H.format_hazards(hz)


def test_a_non_finite_cache_is_refused_before_the_first_step():
    """wd_tune_grad lets rows past the end of a ragged tile re-read the chunk's last row with a zero weight: an inf there would
    reach every class, so fit() reads the chunks' finiteness back with the target sums and refuses."""
    from types import SimpleNamespace
    from wedetect_amd import tune as TN
    m, tower, boxes, labelled, bank0, tuner, chunk = _world()
    bad = dict(tuner.chunks[0])
    bad["E"] = bad["E"].clone()
    bad["E"][-1, 5] = float("inf")
    bad["finite"] = torch.isfinite(bad["E"]).all()
    t = TN.BankTuner(SimpleNamespace(dev=tower.dev, lvl_scale=tower.lvl_scale, lvl_bias=tower.lvl_bias, B=B, ntot=84))
    t.chunks = [tuner.chunks[0], bad]
    with pytest.raises(ValueError, match="non-finite region embeddings"):
        t.fit(bank0, 1, lr=LR)
    t.chunks = [tuner.chunks[0]]
    _, info = t.fit(bank0, 1, lr=LR)
    assert info["status"] == 0 and np.isfinite(info["loss"][0])
