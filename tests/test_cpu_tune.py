"""Bank tuning on the CPU: the numpy restatement (tests/tune_ref.py) against finite differences of its own float64 loss and
hand-made vectors, the plan function, the header against the binding and the build lists, the argument refusals, the detector's
and the script's host side."""
import ctypes
import hashlib
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import tests.tune_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/tune.py to tests/hazards.py)
from tests import tune_ref as R
from tests.abi_decl import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wedetect_hip_tune.h")
f32, f64 = np.float32, np.float64
NAMES = ["wd_tune_abi_version", "wd_tune_grad", "wd_tune_plan", "wd_tune_targets", "wd_tune_update"]


def _chunks(K, dim=R.DIM):
    g = np.random.default_rng(2)
    out = []
    for rows in (100, 37):                                                    # two chunks of unequal size, 84 anchors per image
        E = g.standard_normal((rows, dim)) * 0.3
        pos_cls, pos_y = np.full(rows, -1, np.int32), np.zeros(rows, f32)
        for r in g.choice(rows, 9, replace=False):
            pos_cls[r], pos_y[r] = g.integers(0, K - 1), g.random() * 0.9 + 0.1       # class K - 1 has no positive
        out.append(dict(E=E, pos_cls=pos_cls, pos_y=pos_y, n_anchor=84, off1=64, off2=80, scale=(1.5, 2.0, 0.7), bias=(-1.0, -2.0, 0.5)))
    return out


# ------------------------------------------------------------------------------------------------------------ reference
def test_analytic_gradient_equals_central_differences_through_the_normalisation():
    K = 4
    chunks = _chunks(K)
    W = np.random.default_rng(3).standard_normal((K, R.DIM)) * 2.5             # raw rows, norms far from 1
    loss, dt, dW, T = R.loss_grad(chunks, W)
    assert abs(np.sqrt((T * T).sum(axis=1)) - 1).max() < 1e-12 and abs((dW * W).sum(axis=1)).max() < 1e-9 * abs(dW).max() * 100
    g = np.random.default_rng(4)
    h = 1e-5
    noise = 8 * 2.0 ** -53 * float(loss) / h                                   # a central difference of a float64 loss: its cancellation
    for _ in range(24):                                                        # single elements ...
        k, d = int(g.integers(0, K)), int(g.integers(0, R.DIM))
        Wp, Wm = W.copy(), W.copy()
        Wp[k, d] += h
        Wm[k, d] -= h
        fd = (R.loss_of(chunks, Wp) - R.loss_of(chunks, Wm)) / (2 * h)
        assert abs(fd - dW[k, d]) <= 1e-6 * abs(dW[k, d]) + noise, (k, d, fd, dW[k, d])
    for _ in range(4):                                                         # ... and whole directions
        V = g.standard_normal(W.shape)
        fd = (R.loss_of(chunks, W + h * V) - R.loss_of(chunks, W - h * V)) / (2 * h)
        assert abs(fd - (dW * V).sum()) <= 1e-6 * abs((dW * V).sum()) + noise
    # the unprojected dt is the gradient with respect to the unit rows: it has a radial part, dW has none
    assert abs((dt * T).sum(axis=1)).max() > 1e-3 * abs(dt).max()
    # norm: max(sum pos_y, 1)
    assert R.norm_of(chunks) == pytest.approx(sum(float(c["pos_y"].astype(f64).sum()) for c in chunks)) and R.norm_of(chunks) > 1
    assert R.norm_of([dict(pos_y=np.array([0.25], f32))]) == 1.0


def test_frozen_row_and_one_adam_step_by_hand():
    K = 3
    chunks = _chunks(K)
    W = np.random.default_rng(6).standard_normal((K, R.DIM))
    _, _, dW, _ = R.loss_grad(chunks, W)
    m0, v0 = np.zeros_like(W), np.zeros_like(W)
    lr, (b1, b2), eps = 0.01, (0.9, 0.999), 1e-8
    W1, m1, v1, T1 = R.adam_step(W, m0, v0, dW, 1, lr, (b1, b2), eps, trainable=[1, 0, 1])
    assert np.array_equal(W1[1], W[1]) and not m1[1].any() and not v1[1].any()         # the frozen row: bit for bit
    k, d = 2, 5
    m = (1 - b1) * dW[k, d]
    v = (1 - b2) * dW[k, d] ** 2
    want = W[k, d] - lr * (m / (1 - b1)) / (np.sqrt(v / (1 - b2)) + eps)
    assert W1[k, d] == pytest.approx(want, rel=1e-14) and m1[k, d] == m and v1[k, d] == v
    assert abs(abs(W1[k, d] - W[k, d]) - lr * abs(dW[k, d]) / (abs(dW[k, d]) + eps)) < 1e-12   # the first step: lr |g| / (|g| + eps)
    assert abs(np.sqrt((T1 * T1).sum(axis=1)) - 1).max() < 1e-12
    # the second step uses t = 2 in both corrections
    W2, m2, v2, _ = R.adam_step(W1, m1, v1, dW, 2, lr, (b1, b2), eps, trainable=[1, 0, 1])
    mm = b1 * m + (1 - b1) * dW[k, d]
    vv = b2 * v + (1 - b2) * dW[k, d] ** 2
    assert W2[k, d] == pytest.approx(W1[k, d] - lr * (mm / (1 - b1 ** 2)) / (np.sqrt(vv / (1 - b2 ** 2)) + eps), rel=1e-14)
    # a step against the gradient lowers the loss
    assert R.loss_of(chunks, W1) < R.loss_of(chunks, W)


def test_target_resolution_by_hand():
    m, n = 2, 10
    #            box 0          box 1          box 2 (empty)  box 3
    sel_a = [[3, 5,           3, 7,           -1, -1,        5, 9]]
    sel_i = [[0.5, 0.25,      0.75, 0.25,     0.0, 0.0,      0.25, 0.125]]
    ex_cls = [[11, 22, 33, 44]]
    pc, py = R.targets(np.array(sel_a, np.int32), np.array(sel_i, f32), np.array(ex_cls, np.int32), m, n)
    assert pc.dtype == np.int32 and py.dtype == f32
    assert (pc[0, 3], py[0, 3]) == (22, 0.75)                                 # two boxes claim anchor 3: the larger IoU wins
    assert (pc[0, 5], py[0, 5]) == (11, 0.25)                                 # an IoU tie: the lower example keeps anchor 5
    assert (pc[0, 7], py[0, 7]) == (22, 0.25) and (pc[0, 9], py[0, 9]) == (44, 0.125)
    rest = [a for a in range(n) if a not in (3, 5, 7, 9)]
    assert (pc[0, rest] == -1).all() and not py[0, rest].any()                # unclaimed anchors
    # an empty image, an anchor out of range
    pc, py = R.targets(np.full((2, 4), -1, np.int32), np.zeros((2, 4), f32), np.zeros((2, 2), np.int32), 2, 5)
    assert (pc == -1).all() and not py.any()
    pc, _ = R.targets(np.array([[5, 2]], np.int32), np.array([[0.5, 0.5]], f32), np.array([[1]], np.int32), 2, 5)
    assert pc.tolist() == [[-1, -1, 1, -1, -1]]


def test_plan_covers_every_row_once_and_matches_the_library():
    from wedetect_amd import tune as TN
    for rows in (1, 31, 127, 128, 129, 257, 8400, 84 * 7, 32 * 8400):
        for K in (1, 32, 33, 80, 1203, 20000):
            s = R.plan(rows, K)
            assert s == TN.plan(rows, K) and 1 <= s <= R.MAX_SPLIT and s * -(-K // 32) <= max(R.MAX_SPLIT, -(-K // 32))
            for n in {s, 1, 2, 3, 7}:
                cover = np.zeros(rows, np.int32)
                hi_prev = 0
                for i in range(n):
                    lo, hi = R.split_rows(rows, n, i)
                    assert lo == hi_prev and lo <= hi and (lo % R.ROW_TILE == 0 or lo == rows)
                    cover[lo:hi] += 1
                    hi_prev = hi
                assert hi_prev == rows and (cover == 1).all()
    assert R.plan(32 * 8400, 80) == 85 and R.plan(32 * 8400, 1203) == 6        # small banks still fill the 256 CUs
    assert R.plan(0, 5) == 0 and TN.LIB.wd_tune_plan(0, 5) == 0 and TN.LIB.wd_tune_plan(5, 0) == 0
    with pytest.raises(ValueError):
        TN.plan(0, 1)


# ------------------------------------------------------------------------------------------------- header, library, build
def test_library_exports_the_header_and_the_frozen_abi_is_untouched():
    from tests.test_cpu_abi import check_header
    from tests.test_cpu_tile import MAIN_HEADER_SHA256
    from wedetect_amd import lib as L
    from wedetect_amd import tune as TN
    decl = declared("wedetect_hip_tune.h")
    assert sorted(decl) == sorted(TN.EXPORTS) == NAMES
    for name in decl:
        assert hasattr(L.LIB, name)
    assert TN.LIB.wd_tune_abi_version() == TN.TUNE_ABI_VERSION == 1
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15
    assert hashlib.sha256(open(os.path.join(ROOT, "include", "wedetect_hip.h"), "rb").read()).hexdigest() == MAIN_HEADER_SHA256
    hdr = open(HEADER).read()
    for macro, val, py in (("WD_TUNE_DIM", 768, TN.DIM), ("WD_TUNE_CLASS_BLOCK", 32, TN.CLASS_BLOCK), ("WD_TUNE_ROW_TILE", 128, TN.ROW_TILE),
                           ("WD_TUNE_MAX_SPLIT", 256, TN.MAX_SPLIT)):
        assert re.search(rf"#define\s+{macro}\s+{val}\b", hdr) and py == val, macro
    assert (R.DIM, R.CLASS_BLOCK, R.ROW_TILE, R.MAX_SPLIT) == (TN.DIM, TN.CLASS_BLOCK, TN.ROW_TILE, TN.MAX_SPLIT)
    check_header("wedetect_hip_tune.h")                                        # argtypes / restype against the prototypes
    assert decl["wd_tune_plan"][0] == "int32_t" and TN.LIB.wd_tune_plan.restype is ctypes.c_int32
    for name in decl:
        if name in ("wd_tune_abi_version", "wd_tune_plan"):
            continue
        doc = hdr[: hdr.index(f"int {name}(")].rsplit("/* ----", 1)[1]
        assert "Extents:" in doc and "WD_ERR_BAD_ARG:" in doc, name
    assert "static" in hdr and "task-aligned" in hdr                           # why the targets do not follow the bank


def test_build_lists_are_as_registered_and_the_source_has_no_atomics():
    from wedetect_amd import build as WB
    assert "tune.hip" in WB.SOURCES and "wedetect_hip_tune.h" in WB.PUBLIC_HEADERS
    assert WB.NO_SCRATCH["tune.hip"] == ["tune_targets_kernel", "tune_grad_kernel", "tune_update_kernel"]
    assert WB.ASM_VMEM_SOURCES["tune.hip"] == []
    src = open(os.path.join(WB.CSRC, "tune.hip")).read()
    for k in WB.NO_SCRATCH["tune.hip"]:
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k
    assert "atomic" not in src.lower()
    assert "mfma_f32_32x32x2f32" in src                                         # the hot path is fp32-input MFMA
    # the older add-on is byte for byte what its own tests pin
    assert WB.NO_SCRATCH["exemplar.hip"] == ["exemplar_assign_kernel", "exemplar_pool_kernel"]


def test_argument_refusals_before_any_launch():
    from wedetect_amd import tune as TN
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)                      # non-null, never dereferenced: refused first
    nan, inf = float("nan"), float("inf")

    def targets(sel_a=one, sel_i=one, ex_cls=one, max_ex=4, m=4, batch=2, n_anchor=84, pos_cls=one, pos_y=one):
        return TN.LIB.wd_tune_targets(sel_a, sel_i, ex_cls, max_ex, m, batch, n_anchor, pos_cls, pos_y, None)

    for kw in (dict(sel_a=None), dict(sel_i=None), dict(ex_cls=None), dict(pos_cls=None), dict(pos_y=None), dict(max_ex=0), dict(max_ex=65),
               dict(m=0), dict(m=9), dict(batch=0), dict(n_anchor=0), dict(batch=65536), dict(batch=40000, n_anchor=60000),
               dict(pos_y=ctypes.c_void_p(258))):
        assert targets(**kw) == -1, kw

    def grad(embed=one, rows=168, dim=768, n_anchor=84, off1=64, off2=80, s=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0), pos_cls=one, pos_y=one,
             bank=one, n_cls=3, inv_norm=0.5, n_split=2, slabs=one, parts=one):
        return TN.LIB.wd_tune_grad(embed, rows, dim, n_anchor, off1, off2, *s, *b, pos_cls, pos_y, bank, n_cls, inv_norm, n_split, slabs, parts, None)

    for kw in (dict(embed=None), dict(pos_cls=None), dict(pos_y=None), dict(bank=None), dict(slabs=None), dict(parts=None), dict(dim=512),
               dict(dim=1024), dict(dim=0), dict(rows=0), dict(n_anchor=0), dict(n_cls=0), dict(off1=0), dict(off1=80), dict(off2=85),
               dict(s=(1.0, nan, 1.0)), dict(b=(0.0, 0.0, inf)), dict(inv_norm=0.0), dict(inv_norm=-1.0), dict(inv_norm=nan), dict(inv_norm=inf),
               dict(n_split=0), dict(n_split=257), dict(embed=odd), dict(bank=odd), dict(slabs=odd), dict(parts=ctypes.c_void_p(258)),
               dict(rows=3_000_000), dict(n_cls=65535 * 32 + 1)):
        assert grad(**kw) == -1, kw

    def update(slabs=one, n_slab=2, parts=one, n_cls=3, dim=768, w=one, m=one, v=one, bank=one, tr=one, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8,
               bc1=0.1, bc2=0.001, loss=one, step=0, status=one):
        return TN.LIB.wd_tune_update(slabs, n_slab, parts, n_cls, dim, w, m, v, bank, tr, lr, b1, b2, eps, bc1, bc2, loss, step, status, None)

    for kw in (dict(slabs=None), dict(parts=None), dict(w=None), dict(m=None), dict(v=None), dict(bank=None), dict(tr=None), dict(loss=None),
               dict(status=None), dict(dim=512), dict(n_slab=0), dict(n_cls=0), dict(step=-1), dict(lr=-1.0), dict(lr=nan), dict(b1=1.0),
               dict(b2=-0.1), dict(eps=0.0), dict(bc1=0.0), dict(bc2=1.5), dict(bc1=nan), dict(slabs=odd), dict(w=ctypes.c_void_p(258))):
        assert update(**kw) == -1, kw


def test_every_tune_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_cpu_arena import _takes_memory
    from tests.test_gpu_tune_extents import CASES
    decl = declared("wedetect_hip_tune.h")
    covered = {c.entry for c in CASES}
    for name, params in sorted(decl.items()):
        if name in ("wd_tune_abi_version", "wd_tune_plan"):
            assert not _takes_memory(params) and name not in covered
            continue
        assert _takes_memory(params) and name in covered, f"{name}: tune entry without a case in tests/test_gpu_tune_extents.py"
    assert not covered - set(decl)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_wrappers_are_declared_to_the_happens_before_checker():
    from tests import hazards as H
    assert {"tune.tune_targets", "tune.tune_grad", "tune.tune_update"} <= set(H.ACCESS)
    assert not any(w.startswith("tune.") for w, _, _ in H.BENIGN)              # plain reads and writes only


# ------------------------------------------------------------------------------------------------- detector and script
def test_host_refusals_need_no_device():
    import torch
    from wedetect_amd import tune as TN
    from wedetect_amd.detector import YOLOWorldDetector, plan_tune_boxes
    box = (1.0, 2.0, 30.0, 40.0)
    p = plan_tune_boxes([[(box, 5), ((0, 0, 5, 5), 0)], [], [((2, 2, 9, 9), 5)]], 6, 2, 0.2)
    assert p["ex_boxes"].shape == (3, 2, 4) and p["ex_count"].tolist() == [2, 0, 1] and p["gt_cls"].tolist() == [[5, 0], [0, 0], [5, 0]]
    assert p["m"] == 2 and p["max_ex"] == 2 and plan_tune_boxes([[]])["ex_count"].tolist() == [0]
    bank = torch.zeros(3, 768)
    d = YOLOWorldDetector("nano")                                              # never moved to a device: the checks come first
    for bad, what in (([[((5, 5, 5, 9), 0)]], "positive width"), ([[(box, 3)]], "outside the 3 rows"), ([[(box, -1)]], "non-negative"),
                      ([[(box, 0)] * 65], "at most 64")):
        with pytest.raises(ValueError, match=what):
            d.tune_bank([None] * len(bad), None, bad, init=bank)
    for bad in ("pooled", None, 3, [[1.0] * 768]):                             # bad init
        with pytest.raises(ValueError, match="init"):
            d.tune_bank([None], None, [[(box, 0)]], init=bad)
    with pytest.raises(ValueError, match="a \\[K, 768\\] tensor"):
        d.tune_bank([None], None, [[(box, 0)]], init=torch.zeros(3, 512))
    with pytest.raises(ValueError, match="no text bank"):
        d.tune_bank([None], None, [[(box, 0)]], init="text")
    with pytest.raises(NotImplementedError, match="per-image banks"):
        d.tune_bank([None], None, [[(box, 0)]], init=torch.zeros(2, 3, 768))
    with pytest.raises(ValueError, match="2 names for a bank of 3 rows"):
        d.tune_bank([None], None, [[(box, 0)]], ["a", "b"], init=bank)
    with pytest.raises(ValueError, match="set_tuned_bank fits"):
        d.set_tuned_bank([None], None, [[(box, 0)]], init=bank, fit=False)
    g = YOLOWorldDetector("nano", prompt_groups=True)
    with pytest.raises(NotImplementedError, match="prompt_groups"):
        g.tune_bank([None], None, [[(box, 0)]], init=bank)
    with pytest.raises(RuntimeError, match="not on a HIP device"):            # a valid request reaches the device check
        d.tune_bank([None], None, [[(box, 0)]], init=bank)
    # the cache limit: 640 x 640 images of 8400 anchors, 25.8 MB each
    tw = SimpleNamespace(B=4, ntot=8400)
    t = TN.BankTuner(tw, max_cache_bytes=250_000_000)
    assert t.chunk_bytes() == 4 * 8400 * (768 * 4 + 8)
    t.check_room()
    t.cache_bytes = 2 * t.chunk_bytes()
    with pytest.raises(ValueError, match="25.8 MB per 640 x 640 image"):
        t.check_room()
    with pytest.raises(ValueError, match="no labelled batch"):
        TN.BankTuner(tw).fit(bank, 5)
    with pytest.raises(NotImplementedError, match="per-image banks"):
        TN.check_bank(torch.zeros(2, 3, 768))


def test_script_flags_parse_and_are_off_by_default(capsys):
    import infer_wedetect as I
    a = I.parse_args(["--config", "c"])
    assert a.tune_steps == 0 and a.tune_lr == 1e-2
    a = I.parse_args(["--config", "c", "--text", "x", "--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,30,40:cup", "--tune-steps", "25",
                      "--tune-lr", "0.005", "--save-bank", "o.pt"])
    assert a.tune_steps == 25 and a.tune_lr == 0.005 and a.exemplars == (["cup"], [((1.0, 2.0, 30.0, 40.0), 0)])
    for argv, why in ((["--tune-steps", "5"], "needs --exemplar-boxes"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,3,4:a", "--tune-steps", "-1"], "count >= 0"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,3,4:a", "--tune-steps", "5", "--tune-lr", "0"], "positive rate"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,3,4:a", "--tune-steps", "5", "--prompt-groups"], "--prompt-groups")):
        with pytest.raises(SystemExit) as ei:
            I.parse_args(["--config", "c"] + argv)
        assert ei.value.code == 2 and why in capsys.readouterr().err
