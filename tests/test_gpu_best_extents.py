"""Guard-band tests (GPU) of include/wedetect_hip_best.h, run as tests/test_gpu_extents.py runs the entry points of the main
header (same harness: its Ctx / Run / Case / execute): every operand is carved from a tests/arena.py Arena with guard bands,
the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical, inputs unchanged, no range flag) and its values are
checked once.  The keys are merged into, so every launch starts by restoring them.

tests/test_cpu_best.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

import math
from typing import List

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.best_hazards  # noqa: F401
import tests.test_gpu_extents as X
from tests import best_ref as R

pytestmark = pytest.mark.gpu

f32, i32, i64, u8, f64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


@case("wd_best_similarity_split", "2 x 85 rows (buffer padded to 176), 7 classes, class offset 5", b=2, ntot=85, ends=(64, 80), k=7, off=5)
@case("wd_best_similarity_split", "1 x 525 rows, 264 classes (two column tiles)", b=1, ntot=525, ends=(400, 500), k=264, off=0)
def _best_sim(ctx, b, ntot, ends, k, off, dim=768, es_scale=4.0):
    """As the wd_similarity_split case of tests/test_gpu_extents.py: the rows of e_split behind the last one keep the
    surroundings' pattern; the keys [rows] are the only thing written."""
    from wedetect_amd import best as BS
    rows = b * ntot
    rows8 = (rows + 7) // 8 * 8
    e, t = X._rand(91, rows, dim, scale=0.8), F.normalize(X._rand(92, k, dim), dim=-1)
    es_val = X.split_cpu(e * es_scale)
    es = ctx.ar.take("e_split", (rows8, dim), f32, misalign=16, role="input")
    es[:rows].copy_(es_val.cuda())
    tsc = 2.0 ** (13 - math.floor(math.log2(float(t.abs().max()))))
    ts = X._padded_split(ctx, "t_split", t, tsc)
    key = ctx.inout("key", torch.zeros(rows, dtype=i64), mis=8)
    flag = ctx.flag()
    seg = (ntot, ends[0], ends[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))

    def launch():
        key.zero_()
        BS.best_similarity_split(es, rows, ts, (1.0 / tsc) / es_scale, k, dim, key, off, seg=seg, range_flag=flag)

    def value(o):
        lvl = torch.arange(rows) % ntot
        lvl = (lvl >= ends[0]).long() + (lvl >= ends[1]).long()
        ref = torch.sigmoid((X.unsplit(es_val) / es_scale) @ t.double().T * torch.tensor(seg[3], dtype=f64)[lvl][:, None]
                            + torch.tensor(seg[4], dtype=f64)[lvl][:, None])
        s, lab = BS.unpack_key(o["key"].cpu().numpy().view(np.uint64))
        assert lab.min() >= off and lab.max() < off + k
        X.assert_close("best score", torch.from_numpy(s.copy()), ref.max(dim=1).values, *X.TOL_SIM_SPLIT)
        X.assert_close("score of the best label", ref[torch.arange(rows), torch.from_numpy(lab.astype(np.int64)) - off], ref.max(dim=1).values,
                       2 * X.TOL_SIM_SPLIT[0], X.TOL_SIM_SPLIT[1])
    return X.Run(launch, lambda: {"key": key}, value, f"rows {rows} classes {k} offset {off}", [flag])


@case("wd_best_rows", "3 x 37 rows, 70 of 83 columns, counts 0 / 1 / 70", n_img=3, rpi=37, k=70, ld=83, counts=(0, 1, 70))
@case("wd_best_rows", "2 x 5 rows, one column, count NULL", n_img=2, rpi=5, k=1, ld=1, counts=None)
def _best_rows(ctx, n_img, rpi, k, ld, counts):
    """-> wd_best_unpack: the keys, the scores and the labels are all written whole, nothing else."""
    from wedetect_amd import best as BS
    rows = n_img * rpi
    g = np.random.default_rng(3)
    sc = (np.round(g.random((rows, k), dtype=np.float32) * 32) / 32).astype(np.float32)
    s_d = ctx.inp("scores", torch.from_numpy(sc), ld=ld, mis=4)
    c_d = None if counts is None else ctx.inp("count", torch.tensor(counts, dtype=i32), mis=4)
    key = ctx.inout("key", torch.zeros(rows, dtype=i64), mis=8)
    so, lo = ctx.out("scores_out", (rows,), mis=4), ctx.out("labels_out", (rows,), i32, mis=4, fillers=(-1,))

    def launch():
        key.zero_()
        BS.best_rows(s_d, n_img, rpi, k, ld, key, 11, c_d)
        BS.best_unpack(key, rows, so, lo)

    def value(o):
        s, lab = o["scores_out"].cpu().numpy(), o["labels_out"].cpu().numpy()
        for r in range(rows):
            n = k if counts is None else counts[r // rpi]
            if n == 0:
                assert s[r] == 0 and lab[r] == -1
            else:
                best, arg = R.best_class(sc[r:r + 1, :n])
                assert s[r] == best[0] and lab[r] == arg[0] + 11
    return X.Run(launch, lambda: {"key": key, "scores_out": so, "labels_out": lo}, value, f"{n_img} x {rpi} rows, {k} columns, ld {ld}")


CASES.append(X.Case("wd_best_unpack", "with wd_best_rows above: 3 x 37 rows", CASES[-1].fn))


@case("wd_nms_gather_labeled", "agnostic below split_thr, embeddings gathered, max_out 300", mode="agnostic", max_out=300, split_thr=10000)
@case("wd_nms_gather_labeled", "agnostic per label (split_thr 64), max_out 7", mode="agnostic", max_out=7, split_thr=64)
@case("wd_nms_gather_labeled", "mmcv offsets (workspace), everything fits", mode="mmcv", max_out=1024, split_thr=10000)
def _nms_labeled(ctx, mode, max_out, split_thr, n=900, k=3, dim=32):
    """The wd_nms_gather case of tests/test_gpu_extents.py with one score per anchor and the labels in an array."""
    from wedetect_amd import best as BS
    L = ctx.L
    g = np.random.default_rng(33)
    ctr = g.random((n, 2), dtype=np.float32) * 300 + 20
    wh = g.random((n, 2), dtype=np.float32) * 80 + 2
    bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    sc = np.sort(g.random(n, dtype=np.float32))[::-1].copy()
    lb = g.integers(0, k, n).astype(np.int64)
    emb = g.standard_normal((2, n, dim)).astype(np.float32)
    counts = np.asarray([n, 0], np.int32)                           # the second image has no candidate
    perm = g.permutation(n).astype(np.int32)                       # candidate rank -> anchor
    cidx = np.full((2, n), -1, np.int32)
    cidx[0] = perm
    csc = np.zeros((2, n), np.float32)
    csc[0] = sc
    boxes, labels = np.zeros((2, n, 4), np.float32), np.full((2, n), -1, np.int32)
    boxes[0, perm], labels[0, perm] = bx, lb
    meta = np.asarray([[0, 0, 0, 1, 1, 1e9, 1e9, 0]] * 2, np.float32)
    code = BS.NMS_MMCV_AGNOSTIC if mode == "agnostic" else L.NMS_MMCV
    t = lambda a: torch.from_numpy(a)
    ci, cs, cc = ctx.inp("cand_idx", t(cidx), mis=4), ctx.inp("cand_score", t(csc), mis=4), ctx.inp("cand_count", t(counts), mis=4)
    bd, md, ed = ctx.inp("boxes", t(boxes)), ctx.inp("meta", t(meta), mis=4), ctx.inp("embed", t(emb))
    ld_ = ctx.inp("anchor_labels", t(labels), mis=4)
    ob, os_ = ctx.out("out_boxes", (2, max_out, 4)), ctx.out("out_scores", (2, max_out), mis=4)
    ol = ctx.out("out_labels", (2, max_out), i32, mis=4, fillers=(-1,))
    oa = ctx.out("out_anchors", (2, max_out), i32, mis=4, fillers=(-1,))
    oc = ctx.out("out_count", (2,), i32, mis=4, fillers=(-1,))
    oe = ctx.out("out_embed", (2, max_out, dim))
    ws = ctx.ws("workspace", L.nms_workspace_bytes(2), mis=4)

    def launch():
        BS.nms_gather_labeled(ci, cs, cc, n, bd, n, ld_, k, md, L.nms_threshold(0.7, L.NMS_MMCV), max_out, ed, dim, ob, os_, ol, oa, oc, oe, 2,
                              nms_mode=code, mode_param=split_thr, workspace=ws)

    def value(o):
        keep = R.nms_rows(bx, sc, lb, meta[0], 0.7, max_out, split_thr, mode == "agnostic")["keep"]
        c, a = o["out_count"].cpu().numpy(), o["out_anchors"].cpu().numpy()
        assert c.tolist() == [keep.shape[0], 0]
        assert np.array_equal(a[0, :c[0]], perm[keep]) and np.all(a[0, c[0]:] == -1) and np.all(a[1] == -1)
        assert np.array_equal(o["out_labels"].cpu().numpy()[0, :c[0]], lb[keep]) and np.array_equal(o["out_scores"].cpu().numpy()[0, :c[0]], sc[keep])
        assert np.array_equal(o["out_embed"].cpu().numpy()[0, :c[0]], emb[0, perm[keep]]) and not o["out_embed"].cpu().numpy()[0, c[0]:].any()
    return X.Run(launch, lambda: dict(out_boxes=ob, out_scores=os_, out_labels=ol, out_anchors=oa, out_count=oc, out_embed=oe), value,
                 f"{mode} max_out {max_out} split_thr {split_thr}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_best_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    assert not any(f0) and not any(f1), f"range flags raised: surroundings 0x00 {f0}, 0xFF {f1}"
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite elements"
    if run0.has_ws:
        _, o2, f2 = X.execute(c, 0x00, 0x00)
        assert not any(f2)
        X._same(o0, o2, "workspace 0xFF vs zero-filled")
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, flags 0")
