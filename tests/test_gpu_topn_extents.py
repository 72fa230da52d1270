"""Guard-band tests (GPU) of include/wedetect_hip_topn.h, run as tests/test_gpu_best_extents.py runs the entry points of the
best-class header (the harness of tests/test_gpu_extents.py: its Ctx / Run / Case / execute): every operand is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical, inputs unchanged, no
range flag) and its values are checked once.  The keys are merged into, so every launch starts by clearing them.

tests/test_cpu_topn.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

import math
from typing import List

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.best_hazards  # noqa: F401
import tests.test_gpu_extents as X
import tests.topn_hazards  # noqa: F401
from tests import topn_ref as R

pytestmark = pytest.mark.gpu

f32, i32, i64, u8, f64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


@case("wd_topn_similarity_split", "2 x 85 rows (buffer padded to 176), 7 classes, n 8, class offset 5", b=2, ntot=85, ends=(64, 80), k=7, off=5, n=8, affine=False)
@case("wd_topn_similarity_split", "1 x 525 rows, 264 classes (two column tiles), n 3", b=1, ntot=525, ends=(400, 500), k=264, off=0, n=3, affine=False)
@case("wd_topn_similarity_split", "1 x 85 rows, 40 classes, n 5, the row affine", b=1, ntot=85, ends=(64, 80), k=40, off=0, n=5, affine=True)
def _topn_sim(ctx, b, ntot, ends, k, off, n, affine, dim=768, es_scale=4.0):
    """As the wd_best_similarity_split case: the rows of e_split behind the last one keep the surroundings' pattern; the keys
    [rows][n] are the only thing written."""
    from wedetect_amd import topn as TN
    rows = b * ntot
    rows8 = (rows + 7) // 8 * 8
    e, t = X._rand(91, rows, dim, scale=0.8), F.normalize(X._rand(92, k, dim), dim=-1)
    es_val = X.split_cpu(e * es_scale)
    es = ctx.ar.take("e_split", (rows8, dim), f32, misalign=16, role="input")
    es[:rows].copy_(es_val.cuda())
    tsc = 2.0 ** (13 - math.floor(math.log2(float(t.abs().max()))))
    ts = X._padded_split(ctx, "t_split", t, tsc)
    key = ctx.inout("key", torch.zeros(rows, n, dtype=i64), mis=8)
    flag = ctx.flag()
    seg = (ntot, ends[0], ends[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))
    g = np.random.default_rng(5)
    rs, rb = (g.random(rows, dtype=np.float32) + 0.2), (g.random(rows, dtype=np.float32) - 2.5)
    rs_d = ctx.inp("row_scale", torch.from_numpy(rs), mis=4) if affine else None
    rb_d = ctx.inp("row_bias", torch.from_numpy(rb), mis=4) if affine else None

    def launch():
        key.zero_()
        TN.topn_similarity_split(es, rows, ts, (1.0 / tsc) / es_scale, k, dim, n, key, off, seg=None if affine else seg,
                                 row_scale=rs_d, row_bias=rb_d, range_flag=flag)

    def value(o):
        if affine:
            sc, bi = torch.from_numpy(rs).double().exp()[:, None], torch.from_numpy(rb).double()[:, None]
        else:
            lvl = torch.arange(rows) % ntot
            lvl = (lvl >= ends[0]).long() + (lvl >= ends[1]).long()
            sc, bi = torch.tensor(seg[3], dtype=f64)[lvl][:, None], torch.tensor(seg[4], dtype=f64)[lvl][:, None]
        ref = torch.sigmoid((X.unsplit(es_val) / es_scale) @ t.double().T * sc + bi)
        s, lab = TN.unpack(o["key"].cpu().numpy().view(np.uint64))
        m = min(n, k)
        assert lab[:, :m].min() >= off and lab[:, :m].max() < off + k and bool((lab[:, m:] == -1).all()) and bool((s[:, m:] == 0).all())
        assert all(len(set(r[:m].tolist())) == m for r in lab)                 # no class twice
        X.assert_close("top scores", torch.from_numpy(s[:, :m].copy()), ref.topk(m, dim=1).values, *X.TOL_SIM_SPLIT)
        X.assert_close("scores of the labels", torch.gather(ref, 1, torch.from_numpy(lab[:, :m].astype(np.int64)) - off), ref.topk(m, dim=1).values,
                       2 * X.TOL_SIM_SPLIT[0], X.TOL_SIM_SPLIT[1])
    return X.Run(launch, lambda: {"key": key}, value, f"rows {rows} classes {k} n {n} offset {off}", [flag])


@case("wd_topn_rows", "3 x 37 rows, 70 of 83 columns, counts 0 / 1 / 70, n 5", n_img=3, rpi=37, k=70, ld=83, counts=(0, 1, 70), n=5, affine=False)
@case("wd_topn_rows", "2 x 5 rows, one column, count NULL, n 8", n_img=2, rpi=5, k=1, ld=1, counts=None, n=8, affine=False)
@case("wd_topn_rows", "2 x 9 rows of logits, 33 of 40 columns, the row affine, n 4", n_img=2, rpi=9, k=33, ld=40, counts=None, n=4, affine=True)
def _topn_rows(ctx, n_img, rpi, k, ld, counts, n, affine):
    """-> wd_topn_unpack of the last slot: the keys, the scores and the labels are all written whole, nothing else."""
    from wedetect_amd import topn as TN
    rows = n_img * rpi
    g = np.random.default_rng(3)
    sc = (np.round(g.random((rows, k), dtype=np.float32) * 32) / 32).astype(np.float32)
    if affine:
        sc = (sc * 8 - 4).astype(np.float32)                  # logits
    rs, rb = (g.random(rows, dtype=np.float32) + 0.2), (g.random(rows, dtype=np.float32) - 0.5)
    s_d = ctx.inp("block", torch.from_numpy(sc), ld=ld, mis=4)
    c_d = None if counts is None else ctx.inp("count", torch.tensor(counts, dtype=i32), mis=4)
    rs_d = ctx.inp("row_scale", torch.from_numpy(rs), mis=4) if affine else None
    rb_d = ctx.inp("row_bias", torch.from_numpy(rb), mis=4) if affine else None
    key = ctx.inout("key", torch.zeros(rows, n, dtype=i64), mis=8)
    so, lo = ctx.out("scores_out", (rows,), mis=4), ctx.out("labels_out", (rows,), i32, mis=4, fillers=(-1,))
    slot = n - 1

    def launch():
        key.zero_()
        TN.topn_rows(s_d, n_img, rpi, k, ld, n, key, 11, c_d, rs_d, rb_d)
        TN.topn_unpack(key, rows, n, slot, so, lo)

    def value(o):
        s, lab = TN.unpack(o["key"].cpu().numpy().view(np.uint64))
        assert np.array_equal(o["scores_out"].cpu().numpy(), s[:, slot]) and np.array_equal(o["labels_out"].cpu().numpy(), lab[:, slot])
        for r in range(rows):
            cnt = k if counts is None else counts[r // rpi]
            if cnt == 0:
                assert not s[r].any() and bool((lab[r] == -1).all())
            elif affine:
                ref = 1.0 / (1.0 + np.exp(-(sc[r:r + 1, :cnt].astype(np.float64) * np.exp(np.float64(rs[r])) + np.float64(rb[r]))))
                ws, _ = R.top_n(ref.astype(np.float32), n)
                assert np.abs(s[r].astype(np.float64) - np.sort(ref[0])[::-1][:n]).max() <= 2e-6 and len(set(lab[r].tolist())) == n
                assert np.abs(ref[0][lab[r] - 11] - s[r]).max() <= 2e-6 and ws.shape == (1, n)
            else:
                ws, wl = R.top_n(sc[r:r + 1, :cnt], n)
                assert np.array_equal(s[r], ws[0]) and np.array_equal(lab[r], np.where(wl[0] >= 0, wl[0] + 11, -1))
    return X.Run(launch, lambda: {"key": key, "scores_out": so, "labels_out": lo}, value, f"{n_img} x {rpi} rows, {k} columns, ld {ld}, n {n}")


CASES.append(X.Case("wd_topn_unpack", "with wd_topn_rows above: the last slot of 3 x 37 rows", CASES[-1].fn))


@case("wd_topn_kept", "2 images, 40 anchors, n 3, counts 6 and 0, one anchor out of range", n=3, counts=(6, 0), max_out=9)
@case("wd_topn_kept", "2 images, 40 anchors, n 8, counts max_out and 1", n=8, counts=(5, 1), max_out=5)
def _topn_kept(ctx, n, counts, max_out, n_anchor=40):
    from wedetect_amd import topn as TN
    g = np.random.default_rng(9)
    b = len(counts)
    sc = g.random((b * n_anchor, 50), dtype=np.float32)
    ks, kl = R.top_n(sc, n)
    kl[5, n - 1] = -1
    ks[5, n - 1] = 0                                          # an empty slot among the keys
    key_np = TN.pack(ks, kl)
    anc = np.full((b, max_out), -1, np.int32)
    for i, c in enumerate(counts):
        anc[i, :c] = g.permutation(n_anchor)[:c]
    if counts[0] > 2:
        anc[0, 0], anc[0, 1], anc[0, 2] = 5, n_anchor, -3    # the row with the empty slot; two anchors out of range
    key = ctx.inp("key", torch.from_numpy(key_np.view(np.int64)), mis=8)
    a_d = ctx.inp("out_anchors", torch.from_numpy(anc), mis=4)
    c_d = ctx.inp("out_count", torch.tensor(counts, dtype=i32), mis=4)
    ts = ctx.out("top_scores", (b, max_out, n), mis=4)
    tl = ctx.out("top_labels", (b, max_out, n), i32, mis=4, fillers=(-1,))

    def launch():
        TN.topn_kept(key, n, n_anchor, a_d, c_d, max_out, b, ts, tl)

    def value(o):
        s, lab = o["top_scores"].cpu().numpy(), o["top_labels"].cpu().numpy()
        for i in range(b):
            for r in range(max_out):
                a = int(anc[i, r])
                if r < counts[i] and 0 <= a < n_anchor:
                    assert np.array_equal(s[i, r], ks[i * n_anchor + a]) and np.array_equal(lab[i, r], kl[i * n_anchor + a])
                else:
                    assert not s[i, r].any() and bool((lab[i, r] == -1).all())
    return X.Run(launch, lambda: {"top_scores": ts, "top_labels": tl}, value, f"n {n} counts {counts} max_out {max_out}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_topn_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    assert not any(f0) and not any(f1), f"range flags raised: surroundings 0x00 {f0}, 0xFF {f1}"
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite elements"
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, flags 0")
