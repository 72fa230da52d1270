"""Bank-tuning kernels on the GPU against tests/tune_ref.py (include/wedetect_hip_tune.h): the target resolution bit for bit; the
fused forwards-and-backwards launch and the slab sum against float64 at the shapes where the tiling can go wrong, with the
rounding error of a plain numpy fp32 evaluation of the same formulas as the yardstick; sparse-E cases in which a dropped or
doubled row is an error of order one; the bitwise properties (repeatable, independent of a class's position and neighbours,
frozen rows, the status word); the update against the reference for two steps."""
import numpy as np
import pytest
import torch

import tests.tune_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/tune.py to tests/hazards.py)
from tests import tune_ref as R

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
N_ANCHOR, OFF1, OFF2 = 84, 64, 80                                   # a 64 x 64 image: level boundaries inside a tile
SCALE, BIAS = (f32(1.75), f32(2.5), f32(0.75)), (f32(-3.0), f32(-4.5), f32(-2.0))
ROWS = (1, 31, 32, 33, 84, 168, 257, 8400)
KS = (1, 31, 32, 33, 80, 97)
SPLITS = (1, 2, 3, 7)
_REF = {}                                                            # (rows, K, sparse, seed) -> the chunk and its references


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def edge_rows(rows):
    """First and last row, both sides of every tile boundary and of every boundary of every split count used here."""
    s = {0, rows - 1}
    for t in range(R.ROW_TILE, rows, R.ROW_TILE):
        s |= {t - 1, t}
    for n in SPLITS:
        for i in range(n):
            lo, hi = R.split_rows(rows, n, i)
            s |= {lo - 1, lo, hi - 1, hi}
    return sorted(r for r in s if 0 <= r < rows)


def make_chunk(rows, K, seed=0, sparse=False, e_scale=1.0):
    """A chunk with positives on the edge rows (and a few more), classes cycling downwards from K - 1 — the last, ragged class
    block first — with class ``K - 2`` left without a positive where K >= 3, and y == 1.0 on every third positive."""
    g = np.random.default_rng(1000 * rows + 10 * K + seed)
    E = (g.standard_normal((rows, R.DIM)) * e_scale).astype(f32)
    edges = edge_rows(rows)
    if sparse:
        keep = np.zeros(rows, bool)
        keep[edges] = True
        E[~keep] = 0
    pos = sorted(set(edges) | set(g.integers(0, rows, max(1, rows // 16)).tolist()))
    with_pos = [k for k in range(K - 1, -1, -1) if K < 3 or k != K - 2]
    pos_cls, pos_y = np.full(rows, -1, np.int32), np.zeros(rows, f32)
    for i, r in enumerate(pos):
        pos_cls[r] = with_pos[i % len(with_pos)]
        pos_y[r] = f32(1.0) if i % 3 == 0 else f32(0.1 + 0.8 * g.random())
    return dict(E=E, pos_cls=pos_cls, pos_y=pos_y, n_anchor=N_ANCHOR, off1=OFF1, off2=OFF2, scale=SCALE, bias=BIAS, rows=rows)


def make_bank(K, seed=0):
    W = np.random.default_rng(77 + K + seed).standard_normal((K, R.DIM)).astype(f32)
    T = (W / np.sqrt((W.astype(f64) ** 2).sum(axis=1, keepdims=True))).astype(f32)
    return T


def reference(rows, K, sparse=False):
    """The chunk, the bank and dt / loss in float64 and in plain numpy fp32 — computed once per shape, shared, left unchanged."""
    key = (rows, K, sparse)
    if key not in _REF:
        c, T = make_chunk(rows, K, sparse=sparse), make_bank(K)
        inv = 1.0 / R.norm_of([c])
        l64, d64 = R.chunk_dt(c, T.astype(f64), inv)
        _, d32 = R.chunk_dt(c, T, inv, dtype=f32)
        _REF[key] = dict(c=c, T=T, inv=inv, loss=float(l64), dt=d64, err32=R.grad_rel_err(d32, d64))
    return _REF[key]


def run_grad(chunks, T, inv, splits):
    """wd_tune_grad per chunk into consecutive slabs, then the slab sum in slab order (fp32, as wd_tune_update adds them) ->
    dt [K, 768] (numpy fp32), the raw slabs and partial losses (device)."""
    from wedetect_amd import tune as TN
    K, kp = T.shape[0], TN.k_pad(T.shape[0])
    slabs = torch.full((sum(splits), kp, R.DIM), float("nan"), device="cuda")
    parts = torch.full((sum(splits), kp // 32), float("nan"), device="cuda")
    bank, o = dev(T), 0
    for c, s in zip(chunks, splits):
        TN.tune_grad(dev(c["E"]), c["rows"], c["n_anchor"], c["off1"], c["off2"], c["scale"], c["bias"], dev(c["pos_cls"]), dev(c["pos_y"]),
                     bank, K, inv, s, slabs[o:o + s], parts[o:o + s])
        o += s
    acc = torch.zeros(kp, R.DIM, device="cuda")
    for i in range(slabs.shape[0]):
        acc = acc + slabs[i]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(slabs).all()) and bool(torch.isfinite(parts).all()), "a slab or a partial loss was not written whole"
    assert not bool(slabs[:, K:].any()), "the padded class rows of a slab must be zero"
    return acc[:K].cpu().numpy(), slabs, parts


def device_loss(slabs, parts, K):
    """The loss as wd_tune_update sums it (every row frozen: nothing else is touched)."""
    from wedetect_amd import tune as TN
    z = torch.zeros(K, R.DIM, device="cuda")
    out, status = torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    TN.tune_update(slabs, slabs.shape[0], parts, K, z, z.clone(), z.clone(), z.clone(), torch.zeros(K, dtype=torch.uint8, device="cuda"),
                   1e-3, 0.9, 0.999, 1e-8, 0, out, status)
    return float(out.item())


def z_err(c):
    """max_r a_r * ||E_r|| * 101 * 2^-24 (tune_ref.loss_bound)."""
    a, _ = R.row_consts(c["rows"], c["n_anchor"], c["off1"], c["off2"], c["scale"], c["bias"])
    return float((a * np.sqrt((c["E"].astype(f64) ** 2).sum(axis=1))).max()) * 101 * 2.0 ** -24


def check_grad(tag, got, ref):
    """Every class's ||G - G64|| / ||G64|| against 8 x the figure of the numpy fp32 evaluation of the same case — its largest
    class: one class's own fp32 figure can sit at the storage rounding of the result (2.6e-8 was seen at one row), which no fp32
    evaluation of a logit is held to."""
    err = R.grad_rel_err(got, ref["dt"])
    lim = 8 * float(ref["err32"].max())
    print(f"{tag}: kernel {err.min():.2e} .. {err.max():.2e}, numpy fp32 {ref['err32'].min():.2e} .. {ref['err32'].max():.2e}")
    bad = np.nonzero(~(err <= lim))[0]
    assert bad.size == 0, f"{tag}: classes {bad.tolist()[:8]}: kernel {err[bad][:8]} vs 8 x fp32 {lim}"


# --------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("batch,n,max_ex,m", [(1, 84, 1, 1), (3, 85, 5, 8), (2, 8400, 64, 8), (2, 300, 7, 4)])
def test_targets_bit_exact(batch, n, max_ex, m):
    from wedetect_amd import tune as TN
    g = np.random.default_rng(n + m)
    S = max_ex * m
    sel_a = g.integers(0, min(n, max(4, S // 2)), (batch, S)).astype(np.int32)      # few distinct anchors: many shared claims
    sel_i = (np.round(g.random((batch, S), dtype=f32) * 8) / 8 + f32(0.0625)).astype(f32)  # few distinct IoUs: ties occur
    sel_a[g.random((batch, S)) < 0.2] = -1
    sel_i[sel_a < 0] = 0
    sel_a[0, 0], sel_i[0, 0] = n - 1, 0.5                                            # the last anchor is claimed
    if batch > 1:
        sel_a[1], sel_i[1] = -1, 0                                                   # an image without a box
    ex_cls = g.integers(0, 1203, (batch, max_ex)).astype(np.int32)
    pc, py = torch.full((batch, n), 7, dtype=torch.int32, device="cuda"), torch.full((batch, n), float("nan"), device="cuda")
    TN.tune_targets(dev(sel_a), dev(sel_i), dev(ex_cls), max_ex, m, batch, n, pc, py)
    rc, ry = R.targets(sel_a, sel_i, ex_cls, m, n)
    assert np.array_equal(pc.cpu().numpy(), rc) and np.array_equal(py.cpu().numpy().view(np.uint32), ry.view(np.uint32))
    assert S < 8 or (rc >= 0).sum() < (sel_a >= 0).sum()                             # shared claims were resolved


# ------------------------------------------------------------------------------------------------------ grad: float64 parity
@pytest.mark.parametrize("rows", ROWS)
def test_grad_against_float64(rows):
    for K in KS:
        ref = reference(rows, K)
        for s in SPLITS:
            got, slabs, parts = run_grad([ref["c"]], ref["T"], ref["inv"], [s])
            check_grad(f"rows {rows} K {K} splits {s}", got, ref)
            loss = device_loss(slabs, parts, K)
            bound = R.loss_bound(ref["loss"], rows, K, s, parts.numel(), z_err(ref["c"]), ref["inv"])
            print(f"    loss {loss:.6f} vs {ref['loss']:.6f}, bound {bound:.2e}")
            assert abs(loss - ref["loss"]) <= bound


@pytest.mark.parametrize("rows,K", [(257, 33), (8400, 80), (168, 97)])
def test_grad_sparse_embeddings_expose_a_dropped_row(rows, K):
    ref = reference(rows, K, sparse=True)
    assert float(np.abs(ref["dt"]).max()) > 0
    for s in SPLITS:
        got, _, _ = run_grad([ref["c"]], ref["T"], ref["inv"], [s])
        check_grad(f"sparse rows {rows} K {K} splits {s}", got, ref)


def test_two_chunks_of_unequal_size():
    K = 33
    T = make_bank(K)
    for sparse in (False, True):
        ca, cb = make_chunk(257, K, seed=1, sparse=sparse), make_chunk(84, K, seed=2, sparse=sparse)
        inv = 1.0 / R.norm_of([ca, cb])
        l64, d64, _, _ = R.loss_grad([ca, cb], T.astype(f64))
        _, d32, _, _ = R.loss_grad([ca, cb], T, dtype=f32)
        ref = dict(dt=d64, err32=R.grad_rel_err(d32, d64))
        got, slabs, parts = run_grad([ca, cb], T, inv, [3, 2])
        check_grad(f"chunks 257 + 84 sparse {sparse}", got, ref)
        bound = R.loss_bound(float(l64), 257 + 84, K, 1, parts.numel(), max(z_err(ca), z_err(cb)), inv)
        assert abs(device_loss(slabs, parts, K) - float(l64)) <= bound


def test_one_row_equals_a_g_e():
    """dt_k = a * g_k * E_0, evaluated directly.  Bound per element: the logit is off by at most z_err (tune_ref.loss_bound), the
    sigmoid moves by at most a quarter of that plus 4 ulp of its own evaluation, and (p - y) / norm * a and the one product with
    E_d cost 4 more roundings."""
    K = 5
    c, T = make_chunk(1, K), make_bank(K)
    inv = 1.0 / R.norm_of([c])
    got, _, _ = run_grad([c], T, inv, [1])
    a, b = float(SCALE[0]), float(BIAS[0])
    z = a * (T.astype(f64) @ c["E"][0].astype(f64)) + b
    p = 1 / (1 + np.exp(-z))
    y = np.zeros(K)
    y[c["pos_cls"][0]] = c["pos_y"][0]
    want = (a * (p - y) * inv)[:, None] * c["E"][0].astype(f64)[None, :]
    dp = 0.25 * z_err(c) + 4 * 2.0 ** -24
    bound = np.abs(c["E"][0].astype(f64))[None, :] * a * inv * (dp + 4 * 2.0 ** -24 * np.abs(p - y))[:, None]
    assert c["pos_cls"][0] == K - 1 and c["pos_y"][0] == 1.0
    assert bool((np.abs(got - want) <= bound).all()), float((np.abs(got - want) / bound).max())


def test_logits_of_plus_minus_80_stay_finite():
    K, rows = 33, 257
    c, T = make_chunk(rows, K), make_bank(K)
    c["E"] = np.zeros_like(c["E"])
    for r in range(rows):                                                            # E_r = +-80 / a_r * t_k: z = +-80 + b for that class
        a = float(R.row_consts(rows, N_ANCHOR, OFF1, OFF2, SCALE, BIAS)[0][r])
        c["E"][r] = (80.0 / a) * T[r % K] * (1 if r % 2 else -1)
    inv = 1.0 / R.norm_of([c])
    got, slabs, parts = run_grad([c], T, inv, [2])
    loss = device_loss(slabs, parts, K)
    l64, d64 = R.chunk_dt(c, T.astype(f64), inv)
    assert np.isfinite(got).all() and np.isfinite(loss) and loss > 0
    assert abs(loss - float(l64)) <= R.loss_bound(float(l64), rows, K, 2, parts.numel(), z_err(c), inv)
    assert float(np.abs(got.astype(f64) - d64).max()) <= 1e-4 * float(np.abs(d64).max())


# ------------------------------------------------------------------------------------------------------------- bitwise
def test_two_runs_are_identical_and_a_class_ignores_its_neighbours():
    rows, K = 8400, 33
    ref = reference(rows, K)
    c, T = ref["c"], ref["T"]
    for s in (1, 7):
        a, sa, pa = run_grad([c], T, ref["inv"], [s])
        b, sb, pb = run_grad([c], T, ref["inv"], [s])
        assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)) and torch.equal(pa.view(torch.int32), pb.view(torch.int32))
        # the bank permuted (classes change block and lane), the targets renamed with it
        perm = np.random.default_rng(3).permutation(K)                              # new row j holds old class perm[j]
        inv_perm = np.argsort(perm)
        cp = dict(c, pos_cls=np.where(c["pos_cls"] >= 0, inv_perm[np.maximum(c["pos_cls"], 0)], -1).astype(np.int32))
        p, _, _ = run_grad([cp], T[perm], ref["inv"], [s])
        assert np.array_equal(p.view(np.uint32), a[perm].view(np.uint32))
        # 40 more classes appended (a further class block)
        T2 = np.concatenate([T, make_bank(40, seed=9)])
        e, _, _ = run_grad([c], T2, ref["inv"], [s])
        assert np.array_equal(e[:K].view(np.uint32), a.view(np.uint32))


# -------------------------------------------------------------------------------------------------------------- update
def test_update_two_steps_frozen_rows_and_the_status_word():
    """Tolerances.  dW is a sum of n_slab + 768-term trees in fp32: relative to max|dt| a few 2^-24 per level, 64 * 2^-24 taken;
    m and v are one fused step further (same bound relative to their own maxima).  The step lr * m^ / (sqrt(v^) + eps) has
    magnitude <= lr * 4 for these moments and is insensitive to dW where |dW| >> eps (all but a vanishing share of elements at
    these magnitudes): W within 2 * 2^-24 |W| + lr * 1e-4; T likewise."""
    from wedetect_amd import tune as TN
    K, n_slab, lr, betas, eps = 37, 5, 1e-2, (0.9, 0.999), 1e-8
    kp = TN.k_pad(K)
    g = np.random.default_rng(5)
    W0 = g.standard_normal((K, R.DIM)).astype(f32) * f32(3)
    W0[4] = 0                                                                        # a zero-norm row
    frozen = [1, 35]
    tr = np.ones(K, np.uint8)
    tr[frozen] = 0
    T0 = W0 / np.maximum(np.sqrt((W0.astype(f64) ** 2).sum(axis=1, keepdims=True)), 1e-30)
    T0 = T0.astype(f32)
    T0[4] = f32(0.125)                                                               # whatever the row held: it must stay
    w, m, v, bank = dev(W0), torch.zeros(K, R.DIM, device="cuda"), torch.zeros(K, R.DIM, device="cuda"), dev(T0)
    loss, status = torch.full((2,), float("nan"), device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    live = np.array([k for k in range(K) if tr[k] and k != 4])
    for step in range(2):
        slabs = g.standard_normal((n_slab, kp, R.DIM)).astype(f32)
        parts = g.random((n_slab, kp // 32)).astype(f32)
        before = [x.clone() for x in (w, m, v, bank)]
        TN.tune_update(dev(slabs), n_slab, dev(parts), K, w, m, v, bank, dev(tr), lr, betas[0], betas[1], eps, step, loss, status)
        dt = slabs.astype(f64).sum(axis=0)[:K]
        T64 = before[3].cpu().numpy().astype(f64)
        nrm = np.sqrt((before[0].cpu().numpy().astype(f64) ** 2).sum(axis=1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            dW = (dt - (dt * T64).sum(axis=1, keepdims=True) * T64) / nrm
        dW[4] = 0
        ok = tr.copy()
        ok[4] = 0
        fbetas = tuple(float(f32(x)) for x in betas)                                # the kernel receives the betas as fp32
        Wr, mr, vr, Tr2 = R.adam_step(before[0].cpu().numpy(), before[1].cpu().numpy(), before[2].cpu().numpy(), dW, step + 1, lr, fbetas, eps, ok)
        got = [x.cpu().numpy() for x in (w, m, v, bank)]
        for k in frozen + [4]:                                                       # W, m, v, T bit for bit
            for x, x0 in zip(got, before):
                assert np.array_equal(x[k].view(np.uint32), x0[k].cpu().numpy().view(np.uint32)), k
        assert int(status.item()) == 1                                               # the zero-norm row, and nothing else of it changed
        u = 2.0 ** -24
        assert float(np.abs(got[1][live] - mr[live]).max()) <= 64 * u * float(np.abs(mr[live]).max())
        assert float(np.abs(got[2][live] - vr[live]).max()) <= 64 * u * float(np.abs(vr[live]).max())
        assert bool((np.abs(got[0][live] - Wr[live]) <= 2 * u * np.abs(Wr[live]) + lr * 1e-4).all())
        assert float(np.abs(got[3][live] - Tr2[live]).max()) <= 2 * u + lr * 1e-4
        assert abs(float(loss[step]) - float(parts.astype(f64).sum())) <= 32 * u * float(parts.sum())
    assert float(np.abs(got[0][live] - W0[live]).max()) > lr / 2                     # the rows did step


def test_plan_fills_the_chip_and_grad_refuses_before_any_launch():
    from wedetect_amd import lib as L
    from wedetect_amd import tune as TN
    assert TN.plan(32 * 8400, 80) == 85 and TN.plan(32 * 8400, 1203) == 6 and TN.plan(84, 80) == 1
    ref = reference(33, 31)
    c = ref["c"]
    with pytest.raises(L.WedetectHipError):
        TN.tune_grad(dev(c["E"]), 33, N_ANCHOR, OFF1, OFF2, SCALE, BIAS, dev(c["pos_cls"]), dev(c["pos_y"]), dev(ref["T"]), 31, ref["inv"], 1,
                     torch.empty(1, 32, R.DIM, device="cuda"), torch.empty(1, 1, device="cuda"), dim=512)
