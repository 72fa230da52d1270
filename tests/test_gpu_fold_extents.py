"""Guard-band tests (GPU) of include/wedetect_hip_fold.h, run as tests/test_gpu_extents.py runs the entry points of the main
header (same harness: its Ctx / Run / Case / execute): every operand is carved from a tests/arena.py Arena with guard bands,
the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical, inputs unchanged, no range flag) and its values are
checked once.  Shapes: a bank of 81 rows (ragged 8-column pieces, rows at odd addresses), 3 x 300 kept rows (no multiple of
the 256-row tile), images with no kept row.

tests/test_cpu_fold.py asserts on the CPU that every function of the fold header that takes device memory has a case here.
"""
from __future__ import annotations

import math
from typing import List

import pytest
import torch

import tests.test_gpu_extents as X
from tests.util import assert_close

pytestmark = pytest.mark.gpu

f32, i32, u8 = torch.float32, torch.int32, torch.uint8

CASES: List[X.Case] = []

EXEMPT = {"wd_fold_abi_version": "no memory"}

# the fp16x3 budget of a contraction checked against float64 (tests/test_gpu_extents.py TOL of the split GEMM cases: 2^-22 per
# operand on O(1) products of a 256-term sum, far inside 1e-5 on a sigmoid)
TOL_SCORE = (1e-5, 0.0)


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


def _split_dev(ctx, name, w, scale):
    """wd_split_weights_padded of ``w * scale`` into an arena blob of exactly wd_split_weights_bytes(n, k)."""
    L = ctx.L
    n, k = w.shape
    nbytes = int(L.LIB.wd_split_weights_bytes(n, k))
    buf = ctx.ar.take(name, (nbytes,), u8, misalign=16, role="input", row_pitch=(k + 15) // 16 * 64)
    w_dev = (w * scale).cuda()
    L.check(L.LIB.wd_split_weights_padded(w_dev.data_ptr(), n, k, 1.0, buf.data_ptr(), L.stream_ptr()), "wd_split_weights_padded")
    torch.cuda.synchronize()
    return buf


@case("wd_fold_similarity", "K 81 (ragged pieces, odd row addresses), 3 x 37 rows, images 5 rows apart", b=3, rows=37, n=81, cbs_x=5, c_mis=4)
@case("wd_fold_similarity", "K 80 (16-byte stores), 2 x 300 rows (three row tiles)", b=2, rows=300, n=80, cbs_x=0, c_mis=16)
@case("wd_fold_similarity", "K 1, 2 x 9 rows", b=2, rows=9, n=1, cbs_x=3, c_mis=4)
@case("wd_fold_similarity", "K 300 (three column tiles, last one ragged), 2 x 130 rows", b=2, rows=130, n=300, cbs_x=0, c_mis=16)
def _fold_sim(ctx, b, rows, n, cbs_x, c_mis, cin=256):
    from wedetect_amd import fold as FD
    x = X._rand(11, b * rows, cin)
    wt = X._rand(12, n, cin, scale=cin ** -0.5)
    n8 = (n + 7) // 8 * 8
    bias = torch.zeros(n8)
    bias[:n] = X._rand(13, n, scale=0.3)
    ex = math.frexp(float(wt.abs().max()))[1]
    scale = 2.0 ** (14 - ex)                                # max |w| * scale in [2^13, 2^14): what the engine computes on the device
    a = ctx.inp("a", X.split_cpu(x), ld=cin)
    a_val = X.unsplit(X.split_cpu(x))
    wsp = _split_dev(ctx, "w_split", wt, scale)
    bias_t = ctx.inp("bias", bias)
    u_dev = ctx.inp("w_unscale_dev", torch.tensor([1.0 / (4.0 * scale)], dtype=f32), mis=4)
    c = ctx.out("c", (b, rows, n), ld=n, mis=c_mis, bs=rows + cbs_x)
    flag = ctx.flag()
    oscale, obias = 1.75, -0.4

    def launch():                                           # w_unscale 4 x w_unscale_dev: the product is what counts
        FD.fold_similarity(a, wsp, 4.0, u_dev, bias_t, c, batch=b, rows=rows, cin=cin, n=n, c_batch_stride=rows + cbs_x,
                           out_scale=oscale, out_bias=obias, sigmoid=True, range_flag=flag)

    def value(o):
        y = torch.sigmoid((a_val @ wt.double().T + bias[:n].double()) * oscale + obias)
        assert_close(f"folded similarity m {b * rows} n {n}", o["c"].cpu().reshape(y.shape).double(), y, *TOL_SCORE)
    return X.Run(launch, lambda: {"c": c}, value, f"m {b * rows} n {n} k {cin}, image stride {rows + cbs_x}", [flag])


def _kept_inputs(b, max_out, nl, counts, seed=5):
    g = torch.Generator().manual_seed(seed)
    ntot = sum(nl)
    anchors = torch.full((b, max_out), -1, dtype=i32)
    for i, n in enumerate(counts):
        anchors[i, :n] = torch.randint(0, ntot, (n,), generator=g, dtype=i32)
        if n >= 5:                                          # the level boundaries themselves
            anchors[i, :5] = torch.tensor([nl[0] - 1, nl[0], nl[0] + nl[1] - 1, nl[0] + nl[1], ntot - 1], dtype=i32)
    return anchors, torch.tensor(counts, dtype=i32)


@case("wd_kept_rows_gather", "3 x 300 slots, counts 0 / 300 / 17, gather -> embedding GEMMs -> select", b=3, max_out=300, counts=(0, 300, 17))
@case("wd_kept_rows_gather", "2 x 7 slots, nothing kept", b=2, max_out=7, counts=(0, 0))
def _kept_pipeline(ctx, b, max_out, counts, nl=(64, 16, 4), cin=256, dim=72):
    """The embedding launches of ImageTower._kept_rows: the kept c2 rows by level, one batch-stride GEMM per level on the
    implicit-GEMM kernel (b * max_out rows: 900 is no multiple of its 256-row tile), the rows picked back."""
    from wedetect_amd import fold as FD
    L = ctx.L
    anchors, cnt = _kept_inputs(b, max_out, nl, counts)
    xs = [X._rand(20 + l, b * nl[l], cin) for l in range(3)]
    ws = [X._rand(30 + l, dim, cin, scale=cin ** -0.5) for l in range(3)]
    c2 = [ctx.inp(f"c2_{l}", X.split_cpu(xs[l]), ld=cin) for l in range(3)]
    scales = [2.0 ** (14 - math.frexp(float(w.abs().max()))[1]) for w in ws]
    wsp = [_split_dev(ctx, f"w_split{l}", ws[l], scales[l]) for l in range(3)]
    a_d, c_d = ctx.inp("out_anchors", anchors, mis=4), ctx.inp("out_count", cnt, mis=4)
    rows = b * max_out
    gathered = ctx.out("gathered", (3 * rows, cin), ld=cin)
    level = ctx.out("level_embed", (3 * rows, dim), ld=dim)
    out = ctx.out("out_embed", (rows, dim), ld=dim)
    flag = ctx.flag()

    def launch():
        FD.kept_rows_gather(c2, nl, cin, a_d, c_d, max_out, b, gathered)
        for l in range(3):
            L.conv_gemm(gathered[l * rows:], None, None, level[l * rows:], batch=b, hin=1, win=max_out, cin=cin, lda=cin, n=dim,
                        ldc=dim, c_batch_stride=max_out, w_split=(wsp[l], 1.0 / scales[l]), split_flags=L.SPLIT_A, range_flag=flag)
        FD.kept_rows_select(level, dim, nl[0], nl[0] + nl[1], a_d, c_d, max_out, b, out)

    def value(o):
        off = (0, nl[0], nl[0] + nl[1])
        g_want = torch.zeros(3, rows, cin)
        e_want = torch.zeros(rows, dim, dtype=torch.float64)
        for i in range(b):
            for s in range(counts[i]):
                a = int(anchors[i, s])
                l = (a >= off[1]) + (a >= off[2])
                src = i * nl[l] + a - off[l]
                g_want[l, i * max_out + s] = X.split_cpu(xs[l])[src]
                e_want[i * max_out + s] = X.unsplit(X.split_cpu(xs[l]))[src] @ ws[l].double().T
        assert torch.equal(X._bits(o["gathered"].cpu()), X._bits(g_want.view(3 * rows, cin))), "gathered c2 rows (bytes)"
        got = o["out_embed"].cpu()
        assert_close("kept embeddings", got.double(), e_want, 1e-5, 1e-5)
        keep = torch.zeros(rows, dtype=torch.bool)
        for i in range(b):
            keep[i * max_out: i * max_out + counts[i]] = True
        assert bool((got[~keep] == 0).all()) and not bool(torch.signbit(got[~keep]).any()), "rows past the count must be +0"
        lv = o["level_embed"].cpu().view(3, rows, dim)
        lvl_of = torch.tensor([[(int(a) >= off[1]) + (int(a) >= off[2]) for a in anchors[i]] for i in range(b)]).view(-1)
        assert torch.equal(got[keep], lv[lvl_of[keep], torch.arange(rows)[keep]]), "a kept row is its level's GEMM row, bit for bit"
    return X.Run(launch, lambda: {"gathered": gathered, "level_embed": level, "out_embed": out}, value,
                 f"{b} x {max_out} slots, counts {list(counts)}", [flag])


@case("wd_kept_rows_select", "2 x 300 slots of 768 floats, counts 300 / 0", b=2, max_out=300, counts=(300, 0), dim=768)
@case("wd_kept_rows_select", "3 x 5 slots of 8 floats, counts 5 / 2 / 0", b=3, max_out=5, counts=(5, 2, 0), dim=8)
def _kept_select(ctx, b, max_out, counts, dim, nl=(64, 16, 4)):
    from wedetect_amd import fold as FD
    anchors, cnt = _kept_inputs(b, max_out, nl, counts, seed=9)
    rows = b * max_out
    lv = X._rand(41, 3 * rows, dim)
    lv_d = ctx.inp("level_embed", lv, ld=dim)
    a_d, c_d = ctx.inp("out_anchors", anchors, mis=4), ctx.inp("out_count", cnt, mis=4)
    out = ctx.out("out_embed", (rows, dim), ld=dim)

    def launch():
        FD.kept_rows_select(lv_d, dim, nl[0], nl[0] + nl[1], a_d, c_d, max_out, b, out)

    def value(o):
        want = torch.zeros(rows, dim)
        for i in range(b):
            for s in range(counts[i]):
                a = int(anchors[i, s])
                want[i * max_out + s] = lv.view(3, rows, dim)[(a >= nl[0]) + (a >= nl[0] + nl[1]), i * max_out + s]
        assert torch.equal(X._bits(o["out_embed"].cpu()), X._bits(want))
    return X.Run(launch, lambda: {"out_embed": out}, value, f"{b} x {max_out} slots, counts {list(counts)}, dim {dim}")


@case("wd_kept_rows_reorder", "3 x 300 slots, K 81, counts 300 / 0 / 17, reorder -> select", b=3, max_out=300, counts=(300, 0, 17), k=81)
@case("wd_kept_rows_reorder", "2 x 5 slots, K 1, nothing kept", b=2, max_out=5, counts=(0, 0), k=1)
def _kept_reorder(ctx, b, max_out, counts, k, nl=(64, 16, 4), dim=8):
    """The kept rows take level_scores[level of the anchor][slot][label] and the order (score descending, anchor * k + label
    ascending); boxes, labels, anchors and — through perm — the embeddings move with them; rows past the count stay."""
    from wedetect_amd import fold as FD
    anchors, cnt = _kept_inputs(b, max_out, nl, counts, seed=17)
    g = torch.Generator().manual_seed(18)
    rows, ntot = b * max_out, sum(nl)
    labels = torch.randint(0, k, (b, max_out), generator=g, dtype=i32)
    # a few distinct values only: ties that the index has to break
    ls = torch.randint(1, 8, (3, rows, k), generator=g).float() / 8
    if counts[0] >= 4:                                      # the same (anchor, score) under two labels; the same score on two anchors
        anchors[0, 1] = anchors[0, 0]
        labels[0, 0], labels[0, 1] = k - 1, 0
    boxes0 = X._rand(19, rows, 4)
    scores0 = torch.full((b, max_out), -3.0)
    lv = X._rand(42, 3 * rows, dim)
    ls_d = ctx.inp("level_scores", ls.view(3 * rows, k), ld=k, mis=4)
    lv_d = ctx.inp("level_embed", lv, ld=dim)
    c_d = ctx.inp("out_count", cnt, mis=4)
    init = dict(out_boxes=boxes0, out_scores=scores0, out_labels=labels, out_anchors=anchors)
    io = {n: ctx.inout(n, v, mis=16 if n == "out_boxes" else 4) for n, v in init.items()}
    src = {n: v.cuda() for n, v in init.items()}
    perm = ctx.out("perm", (b, max_out), i32, mis=4)
    out = ctx.out("out_embed", (rows, dim), ld=dim)

    def launch():
        for n in io:
            io[n].copy_(src[n])
        FD.kept_rows_reorder(ls_d, k, ntot, nl[0], nl[0] + nl[1], io["out_boxes"], io["out_scores"], io["out_labels"],
                             io["out_anchors"], c_d, max_out, b, perm)
        FD.kept_rows_select(lv_d, dim, nl[0], nl[0] + nl[1], io["out_anchors"], c_d, max_out, b, out, perm)

    def value(o):
        o = {n: v.cpu() for n, v in o.items()}
        lvl = lambda a: (a >= nl[0]) + (a >= nl[0] + nl[1])
        for i in range(b):
            n = counts[i]
            sl = slice(i * max_out, (i + 1) * max_out)
            key = []
            for s_ in range(n):
                a, c = int(anchors[i, s_]), int(labels[i, s_])
                key.append((-float(ls[lvl(a), i * max_out + s_, c]), a * k + c, s_))
            order = [t[2] for t in sorted(key)]
            want_perm = torch.tensor(order + list(range(n, max_out)), dtype=i32)
            assert torch.equal(o["perm"][i], want_perm), f"image {i}: perm"
            assert torch.equal(o["out_anchors"][i, :n], anchors[i][order]) and torch.equal(o["out_labels"][i, :n], labels[i][order])
            assert torch.equal(o["out_scores"][i, :n], torch.tensor([-t[0] for t in sorted(key)]))
            assert torch.equal(o["out_boxes"].view(b, max_out, 4)[i, :n], boxes0.view(b, max_out, 4)[i][order])
            # rows past the count: untouched
            assert torch.equal(o["out_scores"][i, n:], scores0[i, n:]) and torch.equal(o["out_anchors"][i, n:], anchors[i, n:])
            assert torch.equal(o["out_labels"][i, n:], labels[i, n:])
            assert torch.equal(o["out_boxes"].view(b, max_out, 4)[i, n:], boxes0.view(b, max_out, 4)[i, n:])
            e = o["out_embed"][sl]
            for j, s_ in enumerate(order):
                assert torch.equal(e[j], lv.view(3, rows, dim)[lvl(int(anchors[i, s_])), i * max_out + s_]), f"image {i} row {j}"
            assert bool((e[n:] == 0).all())
    return X.Run(launch, lambda: {**io, "perm": perm, "out_embed": out}, value, f"{b} x {max_out} slots, K {k}, counts {list(counts)}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_fold_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    assert not any(f0) and not any(f1), f"range flags raised: surroundings 0x00 {f0}, 0xFF {f1}"
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite elements"
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, flags 0")


def test_fold_entries_refuse_what_their_kernels_do_not_cover():
    """Argument checks: nothing is launched, WD_ERR_BAD_ARG / WD_ERR_UNSUPPORTED."""
    from wedetect_amd import fold as FD
    from wedetect_amd import lib as L
    dev = torch.device("cuda")
    a = torch.zeros(4, 64, device=dev)
    cnt, anc = torch.zeros(2, dtype=i32, device=dev), torch.zeros(2, 3, dtype=i32, device=dev)
    out = torch.full((3 * 6, 64), 7.0, device=dev)
    p = lambda t: t.data_ptr()
    rc = [FD.LIB.wd_kept_rows_gather(p(a), p(a), p(a), 2, 2, 0, 64, p(anc), p(cnt), 3, 2, p(out), L.stream_ptr()),     # an empty level
          FD.LIB.wd_kept_rows_gather(p(a), p(a), p(a), 2, 2, 2, 66, p(anc), p(cnt), 3, 2, p(out), L.stream_ptr()),    # row_floats % 4
          FD.LIB.wd_kept_rows_gather(p(a), p(a) + 4, p(a), 2, 2, 2, 64, p(anc), p(cnt), 3, 2, p(out), L.stream_ptr()),  # alignment
          FD.LIB.wd_kept_rows_select(p(out), 6, 2, 4, p(anc), p(cnt), None, 3, 2, p(out), L.stream_ptr()),           # dim % 4
          FD.LIB.wd_kept_rows_select(p(out), 64, 4, 2, p(anc), p(cnt), None, 3, 2, p(out), L.stream_ptr()),          # off2 < off1
          FD.LIB.wd_kept_rows_reorder(p(out), 8, 6, 2, 4, p(out), p(out), p(anc), p(anc), p(cnt), 1025, 2, p(anc), L.stream_ptr()),  # max_out
          FD.LIB.wd_kept_rows_reorder(p(out), 8, 6, 2, 7, p(out), p(out), p(anc), p(anc), p(cnt), 3, 2, p(anc), L.stream_ptr())]     # off2 > anchors
    torch.cuda.synchronize()
    assert rc == [-1] * 7, rc
    assert bool((out == 7.0).all())
    with pytest.raises(L.WedetectHipError):                 # no device scale: that is wd_conv_gemm_split's job
        FD.fold_similarity(a, a, 1.0, None, None, out, batch=1, rows=4, cin=64, n=8, c_batch_stride=4, out_scale=1.0, out_bias=0.0)
