"""Guard-band tests (GPU) of include/wedetect_hip_exemplar.h, run as tests/test_gpu_topn_extents.py runs the entry points of the
top-n header (the harness of tests/test_gpu_extents.py: its Ctx / Run / Case / execute): every operand is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical — so every output
element is written — inputs unchanged) and its values are checked once against tests/exemplar_ref.py.

tests/test_cpu_exemplar.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

from typing import List

import numpy as np
import pytest
import torch

import tests.exemplar_hazards  # noqa: F401
import tests.test_gpu_extents as X
from tests import exemplar_ref as R

pytestmark = pytest.mark.gpu

f32, i32 = torch.float32, torch.int32

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


@case("wd_exemplar_assign", "3 images x 85 anchors, 5 example slots, counts 5 / 0 / 2, m 8", batch=3, n=85, max_ex=5, counts=(5, 0, 2), m=8)
@case("wd_exemplar_assign", "1 image x 1029 anchors, 1 example, m 1", batch=1, n=1029, max_ex=1, counts=(1,), m=1)
@case("wd_exemplar_assign", "2 images x 257 anchors, 16 example slots, counts 16 / 9, m 4", batch=2, n=257, max_ex=16, counts=(16, 9), m=4)
def _assign(ctx, batch, n, max_ex, counts, m, thr=0.05):
    """boxes are read up to anchor n - 1 of the last image and not beyond (the 0xFF surroundings are NaN boxes, the 0x00 ones
    empty boxes: neither may become a candidate); example rows past ex_count hold the surroundings' pattern and are not read."""
    from wedetect_amd import exemplar as EX
    g = np.random.default_rng(n)
    xy = np.round(g.random((batch, n, 2), dtype=np.float32) * 200)
    wh = np.round(g.random((batch, n, 2), dtype=np.float32) * 3 + 1) * 8
    boxes = np.concatenate([xy, xy + wh], axis=2).astype(np.float32)
    boxes[:, n - 1] = boxes[:, 0]                                             # the last anchor ties with the first
    meta = np.tile(np.array([2.0, 4.0, 0, 0.5, 0.25, 900, 900, 0], np.float32), (batch, 1))
    ex = np.zeros((batch, max_ex, 4), np.float32)
    for b in range(batch):
        for e in range(max_ex):
            net = boxes[b, (3 * e) % n] + (np.float32(4) if e % 2 else np.float32(0))
            ex[b, e] = (net - np.array([2, 4, 2, 4], np.float32)) / np.array([0.5, 0.25, 0.5, 0.25], np.float32)
    cnt = np.array(counts, np.int32)
    b_d = ctx.inp("boxes", torch.from_numpy(boxes), mis=16)
    e_d = ctx.ar.take("ex_boxes", (batch, max_ex, 4), f32, misalign=4, role="input")      # rows past ex_count: the pattern
    for b in range(batch):
        if counts[b]:
            e_d[b, :counts[b]].copy_(torch.from_numpy(ex[b, :counts[b]]))
    c_d = ctx.inp("ex_count", torch.from_numpy(cnt), mis=4)
    m_d = ctx.inp("meta", torch.from_numpy(meta), mis=4)
    sa = ctx.out("sel_anchors", (batch, max_ex * m), i32, mis=4, fillers=(-1,))
    si = ctx.out("sel_iou", (batch, max_ex * m), mis=4)
    sc = ctx.out("sel_count", (batch,), i32, mis=4)

    def launch():
        EX.exemplar_assign(b_d, n, e_d, c_d, m_d, max_ex, batch, m, thr, sa, si, sc)

    def value(o):
        ra, ri, rc = R.assign(boxes, ex, cnt, meta, m, thr)
        assert np.array_equal(o["sel_anchors"].cpu().numpy(), ra) and np.array_equal(o["sel_count"].cpu().numpy(), rc)
        assert np.array_equal(o["sel_iou"].cpu().numpy().view(np.uint32), ri.view(np.uint32))
        assert ra.reshape(batch, max_ex, m)[0, 0, 0] == 0 and (m == 1 or ra.reshape(batch, max_ex, m)[0, 0, 1] == n - 1)
    return X.Run(launch, lambda: {"sel_anchors": sa, "sel_iou": si, "sel_count": sc}, value, f"{batch} x {n} anchors, {max_ex} slots, m {m}")


@case("wd_exemplar_pool", "24 slots of 768 floats, 5 classes (one empty, one of unassigned slots)", dim=768, n_slot=24)
@case("wd_exemplar_pool", "7 slots of 12 floats, 5 classes", dim=12, n_slot=7)
def _pool(ctx, dim, n_slot):
    """level_embed rows of unassigned slots (anchor -1) and of the two levels a slot's anchor is not in are never read: they
    keep the surroundings' pattern (NaN under 0xFF)."""
    from wedetect_amd import exemplar as EX
    g = np.random.default_rng(dim)
    anchors = g.integers(0, 84, n_slot).astype(np.int32)
    anchors[[1, 4]] = -1
    lv = R.level_of(anchors, 64, 80)
    emb = (g.standard_normal((3, n_slot, dim)) * 3).astype(np.float32)
    iou = (g.random(n_slot, dtype=np.float32) * 0.8 + 0.2).astype(np.float32)
    iou[anchors < 0] = 0
    classes = [[0, 1, 2, 3], [], [1, 4], [5, 6, 0, 2], [n_slot - 1]]
    cls_off = np.cumsum([0] + [len(c) for c in classes]).astype(np.int32)
    cls_slot = np.array([s for c in classes for s in c], np.int32)
    e_d = ctx.ar.take("level_embed", (3, n_slot, dim), f32, misalign=16, role="input")
    for s in range(n_slot):
        if anchors[s] >= 0:
            e_d[lv[s], s].copy_(torch.from_numpy(emb[lv[s], s]))
    a_d = ctx.inp("sel_anchors", torch.from_numpy(anchors), mis=4)
    i_d = ctx.inp("sel_iou", torch.from_numpy(iou), mis=4)
    o_d = ctx.inp("cls_off", torch.from_numpy(cls_off), mis=4)
    s_d = ctx.inp("cls_slot", torch.from_numpy(cls_slot), mis=4)
    bank = ctx.out("bank", (len(classes), dim), mis=16)
    sup = ctx.out("support", (len(classes),), i32, mis=4)

    def launch():
        EX.exemplar_pool(e_d, dim, 64, 80, a_d, i_d, n_slot, o_d, s_d, len(classes), bank, sup)

    def value(o):
        ref, rsup = R.pool(emb, 64, 80, anchors, iou, cls_off, cls_slot)
        got, gsup = o["bank"].cpu().numpy(), o["support"].cpu().numpy()
        assert gsup.tolist() == rsup.tolist() and rsup[1] == 0 and rsup[2] == 0
        for c in range(len(classes)):
            assert float(np.abs(got[c].astype(np.float64) - ref[c]).max()) <= R.pool_bound(int(rsup[c])), c
        assert not got[1].any() and not got[2].any()
    return X.Run(launch, lambda: {"bank": bank, "support": sup}, value, f"{n_slot} slots, dim {dim}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_exemplar_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite elements"
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF")
