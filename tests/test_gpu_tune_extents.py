"""Guard-band tests (GPU) of include/wedetect_hip_tune.h, run as tests/test_gpu_exemplar_extents.py runs the entry points of the
exemplar header (the harness of tests/test_gpu_extents.py: its Ctx / Run / Case / execute): every operand is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical — so every output
element is written: slabs and loss rows start as the surroundings' bytes — inputs unchanged) and its values are checked once
against tests/tune_ref.py.

tests/test_cpu_tune.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

from typing import List

import numpy as np
import pytest
import torch

import tests.test_gpu_extents as X
import tests.tune_hazards  # noqa: F401
from tests import tune_ref as R

pytestmark = pytest.mark.gpu

f32, i32, u8 = torch.float32, torch.int32, torch.uint8
SCALE, BIAS = (1.75, 2.5, 0.75), (-3.0, -4.5, -2.0)

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


@case("wd_tune_targets", "3 images x 85 anchors, 5 slots x 8, one image without a box", batch=3, n=85, max_ex=5, m=8)
@case("wd_tune_targets", "1 image x 1029 anchors, 64 slots x 8", batch=1, n=1029, max_ex=64, m=8)
def _targets(ctx, batch, n, max_ex, m):
    """ex_cls of an example none of whose slots holds an anchor is never read: it keeps the surroundings' pattern."""
    from wedetect_amd import tune as TN
    g = np.random.default_rng(n)
    S = max_ex * m
    sel_a = g.integers(0, min(n, 40), (batch, S)).astype(np.int32)
    sel_i = (np.round(g.random((batch, S), dtype=np.float32) * 8) / 8 + np.float32(0.0625)).astype(np.float32)
    sel_a[:, -m:] = -1                                                       # the last example: no anchor at all
    sel_a[0, 0], sel_i[0, 0] = n - 1, 0.5
    if batch > 1:
        sel_a[1] = -1
    sel_i[sel_a < 0] = 0
    ex_cls = g.integers(0, 1203, (batch, max_ex)).astype(np.int32)
    a_d, i_d = ctx.inp("sel_anchors", torch.from_numpy(sel_a), mis=4), ctx.inp("sel_iou", torch.from_numpy(sel_i), mis=4)
    c_d = ctx.ar.take("ex_cls", (batch, max_ex), i32, misalign=4, role="input")
    used = (sel_a.reshape(batch, max_ex, m) >= 0).any(axis=2)
    for b in range(batch):
        for e in range(max_ex):
            if used[b, e]:
                c_d[b, e] = int(ex_cls[b, e])
    pc = ctx.out("pos_cls", (batch, n), i32, mis=4, fillers=(-1,))
    py = ctx.out("pos_y", (batch, n), mis=4)

    def launch():
        TN.tune_targets(a_d, i_d, c_d, max_ex, m, batch, n, pc, py)

    def value(o):
        rc, ry = R.targets(sel_a, sel_i, ex_cls, m, n)
        assert np.array_equal(o["pos_cls"].cpu().numpy(), rc) and np.array_equal(o["pos_y"].cpu().numpy().view(np.uint32), ry.view(np.uint32))
        assert rc[0, n - 1] == ex_cls[0, 0]
    return X.Run(launch, lambda: {"pos_cls": pc, "pos_y": py}, value, f"{batch} x {n} anchors, {max_ex} x {m} slots")


def _chunk(rows, K, seed):
    g = np.random.default_rng(seed)
    E = g.standard_normal((rows, R.DIM)).astype(np.float32)
    pos_cls, pos_y = np.full(rows, -1, np.int32), np.zeros(rows, np.float32)
    for j, r in enumerate(sorted({0, rows - 1, rows // 2, min(rows - 1, 127), min(rows - 1, 128)})):
        pos_cls[r], pos_y[r] = (K - 1 - j) % K, 1.0 if j == 0 else 0.5
    W = g.standard_normal((K, R.DIM))
    T = (W / np.sqrt((W * W).sum(axis=1, keepdims=True))).astype(np.float32)
    return dict(E=E, pos_cls=pos_cls, pos_y=pos_y, n_anchor=84, off1=64, off2=80, scale=SCALE, bias=BIAS, rows=rows), T


@case("wd_tune_grad", "257 rows, 33 classes, 3 splits", rows=257, K=33, n_split=3)
@case("wd_tune_grad", "1 row, 1 class, 2 splits (one empty)", rows=1, K=1, n_split=2)
@case("wd_tune_grad", "300 rows, 97 classes, 1 split", rows=300, K=97, n_split=1)
def _grad(ctx, rows, K, n_split):
    """E, the targets and the bank are read up to their last element and not beyond (0xFF surroundings are NaN); the slabs and
    the loss rows are written whole, padded class rows included."""
    from wedetect_amd import tune as TN
    c, T = _chunk(rows, K, rows + K)
    inv = 1.0 / R.norm_of([c])
    kp = TN.k_pad(K)
    e_d = ctx.inp("embed", torch.from_numpy(c["E"]), mis=16)
    pc_d, py_d = ctx.inp("pos_cls", torch.from_numpy(c["pos_cls"]), mis=4), ctx.inp("pos_y", torch.from_numpy(c["pos_y"]), mis=4)
    t_d = ctx.inp("bank", torch.from_numpy(T), mis=16)
    slabs = ctx.out("slabs", (n_split, kp, R.DIM), mis=16)
    parts = ctx.out("loss_parts", (n_split, kp // 32), mis=4)

    def launch():
        TN.tune_grad(e_d, rows, 84, 64, 80, SCALE, BIAS, pc_d, py_d, t_d, K, inv, n_split, slabs, parts)

    def value(o):
        l64, d64 = R.chunk_dt(c, T.astype(np.float64), inv)
        _, d32 = R.chunk_dt(c, T, inv, dtype=np.float32)
        s = o["slabs"].cpu().numpy()
        assert not s[:, K:].any()
        got = np.zeros((kp, R.DIM), np.float32)
        for i in range(n_split):
            got = got + s[i]
        assert bool((R.grad_rel_err(got[:K], d64) <= 8 * float(R.grad_rel_err(d32, d64).max())).all())
        assert abs(float(o["loss_parts"].cpu().numpy().astype(np.float64).sum()) - float(l64)) <= 1e-4 * float(l64)
    return X.Run(launch, lambda: {"slabs": slabs, "loss_parts": parts}, value, f"{rows} rows, {K} classes, {n_split} splits")


@case("wd_tune_update", "4 slabs, 37 classes, rows 1 and 35 frozen, row 4 of zero norm", K=37, n_slab=4)
@case("wd_tune_update", "1 slab, 1 class", K=1, n_slab=1)
def _update(ctx, K, n_slab):
    """The padded class rows of the slabs are not read (they keep the surroundings' pattern); frozen rows and the zero-norm row
    keep their bits; loss_out[step] alone is written of loss_out."""
    from wedetect_amd import tune as TN
    kp = TN.k_pad(K)
    g = np.random.default_rng(K)
    slabs = g.standard_normal((n_slab, kp, R.DIM)).astype(np.float32)
    parts = g.random((n_slab, kp // 32)).astype(np.float32)
    W0 = (g.standard_normal((K, R.DIM)) * 2).astype(np.float32)
    tr = np.ones(K, np.uint8)
    if K > 35:
        W0[4] = 0
        tr[[1, 35]] = 0
    T0 = (W0 / np.maximum(np.sqrt((W0.astype(np.float64) ** 2).sum(axis=1, keepdims=True)), 1e-30)).astype(np.float32)
    s_d = ctx.ar.take("slabs", (n_slab, kp, R.DIM), f32, misalign=16, role="input")
    s_d[:, :K].copy_(torch.from_numpy(slabs[:, :K]))
    p_d = ctx.inp("loss_parts", torch.from_numpy(parts), mis=4)
    w = ctx.inout("w", torch.from_numpy(W0), mis=4)
    m = ctx.inout("m", torch.zeros(K, R.DIM), mis=4)
    v = ctx.inout("v", torch.zeros(K, R.DIM), mis=4)
    bank = ctx.inout("bank", torch.from_numpy(T0), mis=4)
    t_d = ctx.inp("trainable", torch.from_numpy(tr), mis=1)
    loss = ctx.inout("loss_out", torch.full((3,), -1.0), mis=4)
    status = ctx.flag("status")

    def launch():
        for x, x0 in ((w, W0), (bank, T0)):                                  # execute() may launch twice: from the same state
            x.copy_(torch.from_numpy(x0))
        m.zero_()
        v.zero_()
        TN.tune_update(s_d, n_slab, p_d, K, w, m, v, bank, t_d, 1e-2, 0.9, 0.999, 1e-8, 1, loss, status)

    def value(o):
        dt = slabs.astype(np.float64).sum(axis=0)[:K]
        T64, nrm = T0.astype(np.float64), np.sqrt((W0.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            dW = (dt - (dt * T64).sum(axis=1, keepdims=True) * T64) / nrm
        ok = tr.copy()
        if K > 35:
            dW[4], ok[4] = 0, 0
        Wr, mr, vr, Tr = R.adam_step(W0, np.zeros_like(dW), np.zeros_like(dW), dW, 2, 1e-2, (0.9, 0.999), 1e-8, ok)
        live = np.nonzero(ok)[0]
        gw, gb = o["w"].cpu().numpy(), o["bank"].cpu().numpy()
        assert bool((np.abs(gw[live] - Wr[live]) <= 2 * 2.0 ** -24 * np.abs(Wr[live]) + 1e-6).all())
        assert float(np.abs(gb[live] - Tr[live]).max()) <= 1e-6
        for k in np.nonzero(ok == 0)[0]:
            assert np.array_equal(gw[k].view(np.uint32), W0[k].view(np.uint32)) and np.array_equal(gb[k].view(np.uint32), T0[k].view(np.uint32))
            assert not o["m"][k].any() and not o["v"][k].any()
        lo = o["loss_out"].cpu().numpy()
        assert lo[0] == -1 and lo[2] == -1 and abs(float(lo[1]) - float(parts.astype(np.float64).sum())) <= 1e-5 * float(parts.sum())
        assert int(o["status"].item()) == (1 if K > 35 else 0)
    return X.Run(launch, lambda: {"w": w, "m": m, "v": v, "bank": bank, "loss_out": loss, "status": status}, value, f"{n_slab} slabs, {K} classes")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_tune_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite elements"
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF")


def test_refusals_happen_before_any_launch():
    """Bad arguments with device pointers that would fault if a kernel ran on them: the status is WD_ERR_BAD_ARG and the device
    stays usable."""
    from wedetect_amd import tune as TN
    one = 256
    assert TN.LIB.wd_tune_grad(one, 33, 512, 84, 64, 80, 1, 1, 1, 0, 0, 0, one, one, one, 3, 1.0, 1, one, one, None) == -1
    assert TN.LIB.wd_tune_update(one, 1, one, 3, 512, one, one, one, one, one, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.001, one, 0, one, None) == -1
    assert TN.LIB.wd_tune_targets(one, one, one, 65, 4, 1, 84, one, one, None) == -1
    torch.cuda.synchronize()
    assert int(torch.ones(4, device="cuda").sum().item()) == 4
