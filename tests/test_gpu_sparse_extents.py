"""Guard-band tests (GPU) of include/wedetect_hip_sparse.h, run as tests/test_gpu_best_extents.py runs the entry points of
the single-label header (the harness of tests/test_gpu_extents.py: its Ctx / Run / Case / execute): every operand is carved
from a tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical, inputs
unchanged, no range flag) and its values are checked once.  The candidate list needs no initialisation: it is carved as a
workspace (0xFF, then dirty from the first launch, then zero-filled); the counters are zeroed by every launch, as the header
asks of the caller.

tests/test_cpu_sparse.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

import math
from typing import List

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.sparse_hazards  # noqa: F401
import tests.test_gpu_extents as X
from tests import sparse_ref as R

pytestmark = pytest.mark.gpu

f32, i32, i64 = torch.float32, torch.int32, torch.int64

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


def _list(ctx, b, list_cap):
    ctx.has_ws = True
    return ctx.ar.take("list", (b, list_cap), i64, misalign=8, role="workspace", fill=ctx.ws_fill)


def _select_outputs(ctx, b, nms_pre):
    cap = ctx.L.topk_capacity(nms_pre)
    return (ctx.out("out_idx", (b, cap), i32, mis=4, fillers=(-1,)), ctx.out("out_score", (b, cap), mis=4),
            ctx.out("out_count", (b,), i32, mis=4, fillers=(-1,)), ctx.out("status", (b,), i32, mis=4, fillers=(-1,)))


def _check_select(o, blocks, thr, list_cap, nms_pre, **kw):
    for b, sc in enumerate(blocks):
        keys = R.image_list(sc, thr, **kw)
        idx, s, n, status = R.select(keys, keys.shape[0], False, list_cap, nms_pre)
        assert int(o["state"][b, 0]) == keys.shape[0] and int(o["state"][b, 1]) == 0
        assert int(o["status"][b]) == status and int(o["out_count"][b]) == n
        assert np.array_equal(o["out_idx"][b].cpu().numpy(), idx)
        assert np.array_equal(o["out_score"][b].cpu().numpy().view(np.uint32), s.view(np.uint32))


@case("wd_sparse_similarity_split", "2 x 85 rows (buffer padded to 176), 7 of 20 classes at offset 5", b=2, ntot=85, ends=(64, 80), k=7, off=5, k_total=20)
@case("wd_sparse_similarity_split", "1 x 525 rows, 264 classes (two column tiles)", b=1, ntot=525, ends=(400, 500), k=264, off=0, k_total=264)
def _sparse_sim(ctx, b, ntot, ends, k, off, k_total, dim=768, es_scale=4.0, list_cap=2048, nms_pre=1000):
    """As the wd_best_similarity_split case: the rows of e_split behind the last one keep the surroundings' pattern.  -> select."""
    from wedetect_amd import sparse as SP
    L = ctx.L
    rows = b * ntot
    rows8 = (rows + 7) // 8 * 8
    e, t = X._rand(91, rows, dim, scale=0.8), F.normalize(X._rand(92, k, dim), dim=-1)
    es_val = X.split_cpu(e * es_scale)
    es = ctx.ar.take("e_split", (rows8, dim), f32, misalign=16, role="input")
    es[:rows].copy_(es_val.cuda())
    tsc = 2.0 ** (13 - math.floor(math.log2(float(t.abs().max()))))
    ts = X._padded_split(ctx, "t_split", t, tsc)
    seg = (ntot, ends[0], ends[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))
    dense = torch.empty(rows, k, device="cuda")                   # the materialising launch on the same operands: the scores' bits
    L.similarity_split(es, rows, ts, (1.0 / tsc) / es_scale, dense, k, dim, k, seg=seg, sigmoid=True)
    torch.cuda.synchronize()
    blocks = dense.cpu().numpy().reshape(b, ntot, k)
    flat = np.sort(blocks.reshape(-1))
    thr = float(flat[-min(flat.shape[0], 900 * b)])               # at most 900 candidates per image on average, fewer than the cap each
    assert all(0 < int((blk > np.float32(thr)).sum()) < list_cap for blk in blocks)
    lst = _list(ctx, b, list_cap)
    state = ctx.inout("state", torch.zeros(b, 2, dtype=i32), mis=4)
    oi, os_, oc, st = _select_outputs(ctx, b, nms_pre)
    flag = ctx.flag()

    def launch():
        state.zero_()
        SP.sparse_similarity_split(es, rows, ts, (1.0 / tsc) / es_scale, k, dim, ntot, k_total, thr, lst, list_cap, state, cls_offset=off,
                                   seg=seg, range_flag=flag)
        SP.sparse_select(lst, list_cap, state, b, nms_pre, oi, os_, oc, st)

    def value(o):
        _check_select(o, blocks, thr, list_cap, nms_pre, n_cls_total=k_total, cls_offset=off)
    return X.Run(launch, lambda: dict(state=state, out_idx=oi, out_score=os_, out_count=oc, status=st), value,
                 f"rows {rows} classes {k} offset {off} thr {thr:.4g}", [flag])


@case("wd_sparse_rows", "3 x 37 rows, 70 of 83 columns, counts 0 / 1 / 70", n_img=3, rpi=37, k=70, ld=83, counts=(0, 1, 70))
@case("wd_sparse_rows", "2 x 5 rows, one column, count NULL", n_img=2, rpi=5, k=1, ld=1, counts=None)
def _sparse_rows(ctx, n_img, rpi, k, ld, counts, list_cap=2048, nms_pre=1500, off=11, k_total=100, thr=0.25):
    """-> wd_sparse_select: the counters, the candidate buffers and the status are written whole, nothing else."""
    from wedetect_amd import sparse as SP
    rows = n_img * rpi
    g = np.random.default_rng(3)
    sc = (np.round(g.random((rows, k), dtype=np.float32) * 32) / 32).astype(np.float32)
    s_d = ctx.inp("scores", torch.from_numpy(sc), ld=ld, mis=4)
    c_d = None if counts is None else ctx.inp("count", torch.tensor(counts, dtype=i32), mis=4)
    lst = _list(ctx, n_img, list_cap)
    state = ctx.inout("state", torch.zeros(n_img, 2, dtype=i32), mis=4)
    oi, os_, oc, st = _select_outputs(ctx, n_img, nms_pre)

    def launch():
        state.zero_()
        SP.sparse_rows(s_d, n_img, rpi, k, ld, k_total, thr, lst, list_cap, state, cls_offset=off, count=c_d)
        SP.sparse_select(lst, list_cap, state, n_img, nms_pre, oi, os_, oc, st)

    def value(o):
        blocks = [sc[b * rpi:(b + 1) * rpi, :(k if counts is None else counts[b])] for b in range(n_img)]
        _check_select(o, blocks, thr, list_cap, nms_pre, n_cls_total=k_total, cls_offset=off)
    return X.Run(launch, lambda: dict(state=state, out_idx=oi, out_score=os_, out_count=oc, status=st), value,
                 f"{n_img} x {rpi} rows, {k} columns, ld {ld}")


CASES.append(X.Case("wd_sparse_select", "with wd_sparse_rows above: 3 x 37 rows", CASES[-1].fn))


@case("wd_sparse_select", "lists of 0 / 5 / 20000 / 40000 (overflow) keys and a non-finite image, cap 32768, nms_pre 30000")
def _select_only(ctx, list_cap=32768, nms_pre=30000):
    """Global strides (two 8192-key chunks and more), an empty, an overflowed and a non-finite image."""
    from wedetect_amd import sparse as SP
    seen = [0, 5, 20000, 40000, 300]
    b = len(seen)
    g = np.random.default_rng(8)
    keys = np.zeros((b, list_cap), np.uint64)
    for i, n in enumerate(seen):
        m = min(n, list_cap)
        sc = (np.round(g.random(m, dtype=np.float32) * 4096) / 4096).astype(np.float32)              # equal scores
        keys[i, :m] = R.pack_key(sc, g.permutation(1 << 22)[:m])
    src = torch.from_numpy(keys.view(np.int64)).cuda()
    st_host = torch.tensor([[n, int(i == 4)] for i, n in enumerate(seen)], dtype=i32)
    lst = _list(ctx, b, list_cap)
    state = ctx.inp("state", st_host, mis=4)
    oi, os_, oc, st = _select_outputs(ctx, b, nms_pre)

    def launch():
        for i, n in enumerate(seen):                              # slots past the counter keep what the surroundings gave them
            lst[i, :min(n, list_cap)].copy_(src[i, :min(n, list_cap)])
        SP.sparse_select(lst, list_cap, state, b, nms_pre, oi, os_, oc, st)

    def value(o):
        for i, n in enumerate(seen):
            idx, s, cnt, status = R.select(keys[i, :min(n, list_cap)], n, i == 4, list_cap, nms_pre)
            assert int(o["status"][i]) == status and int(o["out_count"][i]) == cnt
            assert np.array_equal(o["out_idx"][i].cpu().numpy(), idx) and np.array_equal(o["out_score"][i].cpu().numpy(), s)
        assert o["status"].tolist() == [0, 0, 0, 1, 2] and o["out_count"].tolist() == [0, 5, 20000, 0, -1]
    return X.Run(launch, lambda: dict(out_idx=oi, out_score=os_, out_count=oc, status=st), value, f"seen {seen}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_sparse_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    assert not any(f0) and not any(f1), f"range flags raised: surroundings 0x00 {f0}, 0xFF {f1}"
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite elements"
    assert run0.has_ws
    _, o2, f2 = X.execute(c, 0x00, 0x00)
    assert not any(f2)
    X._same(o0, o2, "list 0xFF vs zero-filled")
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, flags 0")
