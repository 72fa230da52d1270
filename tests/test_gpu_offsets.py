"""Large-offset tests (GPU): one operand of a launch spans more than 2^31 and 2^32 bytes — or elements, or classes — while every
other operand stays compact.  The table is tests/offsets_cases.py; the refusals in it run without a device in
tests/test_cpu_offsets.py.

A giant operand is sparse: a row stride of 64 KiB under rows of a few hundred bytes, so 65 792 rows span 4.3 GB and the launch
takes microseconds.  It is carved from a tests/arena.py Arena filled with 0xFF (NaN as fp32 / fp16, -1 as int32), with 2 GiB of
guard in front and behind: an offset wrapped modulo 2^32 lands inside the operand, a sign-wrapped one at most 2 GiB away — in
memory the test owns, where it changes a value or a guard byte instead of faulting.  Per case:

  1. the COMPACT launch (same entry, same m / n / k, same forced cfg, ld = row width) against float64 on the host, on sampled rows:
     the first and last 256, the 256 on either side of the rows where the giant operand passes byte 2^31 and 2^32, and the tile-edge
     rows next to each block — at the tolerance the existing test of that entry asserts;
  2. the WIDE launch bit-identical to the compact one in EVERY row (torch.equal on the device): a row's result does not depend on
     its stride;
  3. guards, spare columns and the rows between c_batch_stride images still 0xFF, inputs still their bits
     (Arena.check_blocked: row blocks on the device, no host copy).

Each case holds at most 16 GiB and frees it before it returns; it may skip only when the device has less free memory than that.
"""
from __future__ import annotations

import gc
import math

import pytest
import torch
import torch.nn.functional as F

from tests import offsets_cases as O
from tests.arena import Arena
from tests.test_gpu_extents import split_cpu, unsplit
from tests.util import assert_close

pytestmark = pytest.mark.gpu

f32, f64, i32, i64, u8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
CORRECT = [c for c in O.CASES if c.expect == "correct"]

# tolerances of the existing tests of each entry, reused unchanged (atol, rtol)
TOL_GEMM_F32 = (2e-5, 2e-5)         # tests/test_gpu_kernels.py  test_gemm_plain
TOL_SIM_F32 = (2e-6, 1e-5)          # tests/test_gpu_kernels.py  similarity epilogue (sigmoid)
TOL_SPLIT = (6e-6, 2e-6)            # tests/test_gpu_split.py  fp16x3 GEMM / conv vs float64
TOL_SIM_SPLIT = (2e-6, 1e-6)        # tests/test_gpu_split.py  wd_similarity_split (sigmoid)
REL_CONV3 = 2e-5                    # tests/test_gpu_split.py  row-sharing 3 x 3 kernels: |d| < 2e-5 * max|ref|
TOL_LN = (5e-6, 5e-6)               # tests/test_gpu_kernels.py  LayerNorm rows
TOL_RETR_SPLIT = (3e-6, 0.0)        # tests/test_gpu_split.py  wd_retrieval_max_split
TOL_DW = (1e-5, 1e-5)               # tests/test_gpu_kernels.py  depthwise 7 x 7
TOL_STATS_MEAN = (1e-6, 2e-6)       # tests/test_gpu_split.py  wd_ln_stats_finalize: row mean
TOL_STATS_RSTD = (0.0, 3e-6)        # tests/test_gpu_split.py  wd_ln_stats_finalize: row rstd


def _L():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wedetect_amd import lib
    return lib


def _need(nbytes: int) -> None:
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"needs {nbytes / 2 ** 30:.1f} GiB of free device memory, the device has {free / 2 ** 30:.1f} GiB free")


def _release() -> None:
    gc.collect()
    torch.cuda.empty_cache()


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, device="cuda", generator=g) * scale


def sample_rows(m: int, marks, tile: int = 256) -> torch.Tensor:
    """Row indices [0, m): 256 rows on either side of every mark (0 and m always among them), each block widened to the next
    multiple of ``tile`` and one row beyond it: the tile-edge rows next to the block."""
    rows = set()
    for r in {0, m, *[int(x) for x in marks]}:
        lo = max(0, (r - 256) // tile * tile - 1)
        hi = min(m, -(-(r + 256) // tile) * tile + 1)
        rows.update(range(max(lo, 0), max(hi, 0)))
    return torch.tensor(sorted(rows), dtype=i64)


def byte_marks(pitch_bytes: int):
    """Rows of an operand of that pitch in which byte offsets 2^31 and 2^32 fall."""
    return [(1 << 31) // pitch_bytes, (1 << 32) // pitch_bytes]


def giant(name, shape, dtype, *, ld, role, data=None, batch_stride=None, extra=0, min_span=1 << 32):
    """An Arena that holds ONE operand: ``shape`` with rows ``ld`` elements apart, 2 GiB of 0xFF on each side.  ``min_span``: what
    the operand must at least span (2^32 bytes unless the case stops short of it on purpose)."""
    esz = torch.empty((), dtype=dtype).element_size()
    rows = math.prod(shape[:-1])
    span = ((batch_stride * (shape[0] - 1) + shape[1]) if batch_stride else rows) * ld * esz
    cap = span + 2 * O.GUARD + (2 << 20) + extra
    _need(cap + (1 << 30))
    ar = Arena(cap, "cuda", 0xFF)
    view = ar.take(name, shape, dtype, ld=ld, role=role, data=data, batch_stride=batch_stride, guard_bytes=O.GUARD)
    buf = ar.buffers[name]
    assert buf.guard >= O.GUARD and buf.end - buf.start > min_span, f"{name}: the operand spans {buf.end - buf.start} bytes, not {min_span}"
    return ar, view


# ================================================================================================ GEMM family
def run_gemm(c, L):
    k = c.kw
    kind, wide, m, n, cin = k["kind"], k["wide"], k["m"], k["n"], k["cin"]
    flags, cfg = k.get("flags", 0), k.get("cfg")
    SA, SC = bool(flags & 1), bool(flags & 2)
    g = _gen(len(c.id) * 7919 + m + n)
    b, h, w = (k["b"], k["h"], k["w"]) if "b" in k else ((m // k["hw"], 1, k["hw"]) if wide == "cbs" else (1, 1, m))
    deconv = wide == "deconv"
    co = n // 4 if deconv else n
    out_rows = 4 * m if deconv else m
    x = _randn(g, m, cin)
    wt = _randn(g, n, cin, scale=cin ** -0.5)
    bias = _randn(g, n, scale=0.3)
    a_c = split_cpu(x) if SA else x                                     # compact activations, float32-typed
    res_mode = "inplace" if wide == "inplace" else ("sep" if wide == "res" or k.get("res") == "sep" else None)
    r = _randn(g, m, n) if res_mode else None
    res_alpha = 1.0 if res_mode == "inplace" else 0.625
    seg = (k["seg_rows"], k["seg_ends"][0], k["seg_ends"][1], (0.7, 0.58, 0.82), (-2.6, -2.2, -1.9)) if wide == "seg" else None
    base = dict(batch=b, hin=h, win=w, cin=cin, n=n, seg=seg, sigmoid=seg is not None, res_alpha=res_alpha)
    if kind == "f32":
        wd = wt
    else:
        wd = None
        base.update(w_split=L.split_weights(wt), split_cfg=cfg, split_flags=flags)
    if deconv:
        base.update(out_mode=L.OUT_DECONV2X2)
    ws = None
    if k.get("splits"):
        ws = torch.full((k["splits"] * m * n,), float("nan"), device="cuda")
        base.update(workspace=ws, k_splits=k["splits"])
    elif cfg == 65:
        ws = torch.zeros(L.p8_workspace_bytes() // 4, device="cuda")
        base.update(workspace=ws, k_splits=0)
    flag = torch.zeros(1, dtype=i32, device="cuda") if kind == "split" else None
    if flag is not None:
        base.update(range_flag=flag)
    ld_w = k.get("ldc", O.WIDE_LD)                                      # the wide stride of this case

    def launch(a, lda, cc, ldc, res=None, ldres=0, c2=None, ldc2=0, cbs=0, cfg_=None):
        kw = dict(base, lda=lda, ldc=ldc, res=res, ldres=ldres, c2=c2, ldc2=ldc2, c_batch_stride=cbs)
        if cfg_ is not None:
            kw.update(split_cfg=cfg_)
        L.conv_gemm(a, wd, bias, cc, **kw)

    # ---- compact launch: ld = row width everywhere
    hw = h * w
    cbs_c = hw if wide == "cbs" else 0
    c_c = r.clone() if res_mode == "inplace" else torch.full((out_rows, co), float("nan"), device="cuda")
    c2_c = torch.full((m, n), float("nan"), device="cuda") if k.get("c2") else None
    res_c = c_c if res_mode == "inplace" else r
    launch(a_c, cin, c_c, co, res=res_c, ldres=n if res_mode else 0, c2=c2_c, ldc2=n if c2_c is not None else 0, cbs=cbs_c)
    if "same_as_cfg" in k:                                              # production against the forced tile it must equal
        c_f = torch.full_like(c_c, float("nan"))
        launch(a_c, cin, c_f, co, cfg_=k["same_as_cfg"])
        assert torch.equal(c_c, c_f), f"production dispatch differs from forced cfg {k['same_as_cfg']} on the compact operands"
    torch.cuda.synchronize()

    # ---- float64 on the host, sampled rows of the GEMM's [m, n] space
    pitch = ld_w * 4
    if wide == "cbs":
        marks = [(bb // (k["cbs"] * co * 4)) * hw for bb in (1 << 31, 1 << 32)]
    elif deconv:                                                        # output pixel row R -> its source pixel
        marks = []
        for R in byte_marks(pitch):
            bi, y, xx = R // (4 * hw), R // (2 * w) % (2 * h), R % (2 * w)
            marks.append((bi * h + y // 2) * w + xx // 2)
    else:
        marks = byte_marks(pitch)
    marks += [seg[1], seg[2], seg[0], seg[0] + seg[1]] if seg is not None else []
    S = sample_rows(m, marks)
    Sd = S.cuda()
    a_val = (unsplit(a_c[Sd]) if SA else x[Sd].double()).cpu()
    y = a_val @ wt.double().cpu().T + bias.double().cpu()
    if seg is not None:
        pos = S % seg[0]
        lvl = (pos >= seg[1]).long() + (pos >= seg[2]).long()
        y = torch.sigmoid(y * torch.tensor(seg[3], dtype=f64)[lvl][:, None] + torch.tensor(seg[4], dtype=f64)[lvl][:, None])
    if r is not None:
        y = y + res_alpha * r[Sd].double().cpu()
    got = c_c.view(b, h, 2, w, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(m, n) if deconv else c_c
    got = got[Sd]
    g64 = (unsplit(got) if SC else got.double()).cpu()
    tol = TOL_SIM_F32 if seg is not None else (TOL_GEMM_F32 if kind == "f32" else TOL_SPLIT)
    err = assert_close(f"{c.id}: compact launch vs float64 on {S.numel()} sampled rows", g64, y, *tol)
    if c2_c is not None:
        assert_close(f"{c.id}: compact c2 vs float64", c2_c[Sd].double().cpu(), y, *tol)

    # ---- wide launch: one operand from the arena
    if kind == "f32":
        picked = L.gemm_config(m, n, cin)
    elif SA and (wide in ("cbs", "seg", "deconv") or k.get("c2") or (SC and res_mode)):
        picked = L.gemm_config(m, n, cin, split=True, dma=True)
    elif SA:
        picked = L.gemm_config(m, n, cin, split=True, presplit=True, park=cfg == 65)
    else:
        picked = L.gemm_config(m, n, cin, split=True)
    print(f"{c.id}: m {m} n {n} k {cin} flags {flags} cfg {cfg}: the shape-only production choice for both launches is {picked!r}"
          f"{'' if cfg in (None, -1) else ' (the forced cfg overrides it on both)'}; compact vs float64 max |d| {err:.3g}")
    a_w, c_w, res_w, c2_w = a_c, None, r, None
    lda, ldc, ldres, ldc2, cbs_w = cin, co, (n if res_mode else 0), (n if c2_c is not None else 0), cbs_c
    if wide == "a":
        # (the rows one group inside the 2^32 limit of cfg 64 / 65 / 66 end within 512 KiB of it)
        ar, a_w = giant("a", (m, cin), f32, ld=ld_w, role="input", data=a_c, min_span=(1 << 32) - (2 << 20) if m < 65536 else 1 << 32)
        lda = ld_w
    elif wide in ("c", "seg", "deconv"):
        ar, c_w = giant("c", (out_rows, co), f32, ld=ld_w, role="output")
        ldc = ld_w
    elif wide == "cbs":
        ar, c_w = giant("c", (b, hw, co), f32, ld=co, role="output", batch_stride=k["cbs"])
        cbs_w = k["cbs"]
    elif wide == "res":
        ar, res_w = giant("res", (m, n), f32, ld=ld_w, role="input", data=r)
        ldres = ld_w
    elif wide == "inplace":
        ar, c_w = giant("c", (m, n), f32, ld=ld_w, role="inout", data=r)
        res_w, ldc, ldres = c_w, ld_w, ld_w
    elif wide == "c2":
        ar, c2_w = giant("c2", (m, n), f32, ld=ld_w, role="output")
        ldc2 = ld_w
    else:
        raise KeyError(wide)
    if c_w is None:
        c_w = torch.full((out_rows, co), float("nan"), device="cuda")
    if c2_c is not None and c2_w is None:
        c2_w = torch.full((m, n), float("nan"), device="cuda")
    if ws is not None and cfg != 65:
        ws.fill_(float("nan"))
    ar.arm()
    launch(a_w, lda, c_w, ldc, res=res_w, ldres=ldres, c2=c2_w, ldc2=ldc2, cbs=cbs_w)
    torch.cuda.synchronize()
    c_w2 = c_w.reshape(out_rows, co) if wide == "cbs" else c_w
    assert torch.equal(c_w2, c_c), f"{c.id}: the wide launch differs from the compact one: {_first_diff(c_w2, c_c)}"
    if c2_c is not None:
        assert torch.equal(c2_w, c2_c), f"{c.id}: c2 of the wide launch differs from the compact one: {_first_diff(c2_w, c2_c)}"
    ar.check_blocked()
    if flag is not None:
        assert int(flag.item()) == 0, "range flag raised"
    del ar, a_w, c_w, res_w, c2_w, c_w2


def _first_diff(a, b) -> str:
    d = (a.reshape(b.shape).contiguous().view(i32) != b.contiguous().view(i32)).nonzero()
    return f"{d.shape[0]} element(s), first at {tuple(int(v) for v in d[0])}, last at {tuple(int(v) for v in d[-1])}" if d.shape[0] else "none"


# ================================================================================================ implicit-GEMM kernels
def run_conv(c, L):
    k = c.kw
    b, h, w, cin, n, lda, kh, stride, pad, cfg = k["b"], k["h"], k["w"], k["cin"], k["n"], k["lda"], k["kh"], k["stride"], k["pad"], k["cfg"]
    deconv = k.get("deconv", False)
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kh) // stride + 1
    m, kk, px = b * ho * wo, kh * kh * cin, b * h * w
    g = _gen(len(c.id) * 104729 + lda)
    x = _randn(g, px, cin)
    wt = _randn(g, n, kk, scale=kk ** -0.5)
    bias = _randn(g, n, scale=0.3)
    a_c = split_cpu(x)
    flag = torch.zeros(1, dtype=i32, device="cuda")
    co, out_rows = (n // 4, 4 * m) if deconv else (n, m)
    base = dict(batch=b, hin=h, win=w, cin=cin, kh=kh, kw=kh, stride=stride, pad=pad, n=n, ldc=co, w_split=L.split_weights(wt), split_cfg=cfg,
                split_flags=L.SPLIT_A, range_flag=flag, out_mode=L.OUT_DECONV2X2 if deconv else L.OUT_ROWS)
    c_c = torch.full((out_rows, co), float("nan"), device="cuda")
    L.conv_gemm(a_c, None, bias, c_c, lda=cin, **base)
    torch.cuda.synchronize()
    # float64 on the host: the whole (small) map, compared on the output rows whose taps read the sampled pixels
    xi = unsplit(a_c).cpu().view(b, h, w, cin).permute(0, 3, 1, 2)
    wi = wt.double().cpu().view(n, kh, kh, cin).permute(0, 3, 1, 2)
    y = F.conv2d(xi, wi, bias.double().cpu(), stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(m, n)
    got = (c_c.view(b, ho, 2, wo, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(m, n) if deconv else c_c).double().cpu()
    pix_marks = byte_marks(lda * 4)                                     # input pixels at byte 2^31 / 2^32 of a
    marks = []
    for pm in pix_marks:
        bi, yy, xx = pm // (h * w), pm // w % h, pm % w
        marks.append((min(bi, b - 1) * ho + min(yy // stride, ho - 1)) * wo + min(xx // stride, wo - 1))
    S = sample_rows(m, marks)
    three = kh == 3 and stride == 1 and cfg in (-1, 77, 78, 79)
    tol = (REL_CONV3 * float(y.abs().max()), 0.0) if three else TOL_SPLIT
    err = assert_close(f"{c.id}: compact launch vs float64 on {S.numel()} sampled rows", got[S], y[S], *tol)
    picked = L.gemm_config(m, n, kk, split=True, dma=True, conv3=kh == 3 and stride == 1)
    print(f"{c.id}: {b} x {h} x {w} x {cin} -> n {n}, {kh} x {kh} / {stride}, lda {lda}, cfg {cfg}: production choice for both launches "
          f"{picked!r}; compact vs float64 max |d| {err:.3g}")
    ar, a_w = giant("a", (px, cin), f32, ld=lda, role="input", data=a_c)
    c_w = torch.full((out_rows, co), float("nan"), device="cuda")
    ar.arm()
    L.conv_gemm(a_w, None, bias, c_w, lda=lda, **base)
    torch.cuda.synchronize()
    assert torch.equal(c_w, c_c), f"{c.id}: the wide launch differs from the compact one: {_first_diff(c_w, c_c)}"
    ar.check_blocked()
    assert int(flag.item()) == 0, "range flag raised"
    del ar, a_w


# ================================================================================================ LayerNorm rows
def _ln_ref(xs: torch.Tensor, gamma, beta, eps=1e-6):
    x64 = xs.double().cpu()
    mu = x64.mean(dim=1, keepdim=True)
    var = x64.var(dim=1, unbiased=False, keepdim=True)
    return (x64 - mu) / torch.sqrt(var + eps) * gamma.double().cpu() + beta.double().cpu()


def run_layernorm(c, L):
    k = c.kw
    rows, cc, wide, split = k["rows"], k["c"], k["wide"], k["split"]
    g = _gen(rows * 31 + cc + len(c.id))
    x = _randn(g, rows, cc) + 0.25
    gamma, beta = _randn(g, cc, scale=0.5) + 1.0, _randn(g, cc, scale=0.3)
    y_c = torch.full((rows, cc), float("nan"), device="cuda")
    L.layernorm_rows(x, y_c, gamma, beta, rows, cc, split=split)
    torch.cuda.synchronize()
    ld = O.WIDE_LD_LN
    assert rows * ld * 4 > 1 << 32
    S = sample_rows(rows, byte_marks(ld * 4), tile=64)
    Sd = S.cuda()
    got = (unsplit(y_c[Sd]) if split else y_c[Sd].double()).cpu()
    err = assert_close(f"{c.id}: compact launch vs float64 on {S.numel()} sampled rows", got, _ln_ref(x[Sd], gamma, beta), *TOL_LN)
    print(f"{c.id}: rows {rows} c {cc} {'hi/lo' if split else 'fp32'} output, {'four rows' if rows >= 65536 and cc <= 256 else 'one row'} per "
          f"lane group; compact vs float64 max |d| {err:.3g}")
    if wide == "x":
        ar, x_w = giant("x", (rows, cc), f32, ld=ld, role="input", data=x)
        y_w = torch.full((rows, cc), float("nan"), device="cuda")
        ar.arm()
        L.layernorm_rows(x_w, y_w, gamma, beta, rows, cc, ldx=ld, split=split)
    else:
        ar, y_w = giant("y", (rows, cc), f32, ld=ld, role="output")
        ar.arm()
        L.layernorm_rows(x, y_w, gamma, beta, rows, cc, ldy=ld, split=split)
    torch.cuda.synchronize()
    assert torch.equal(y_w, y_c), f"{c.id}: the wide launch differs from the compact one: {_first_diff(y_w, y_c)}"
    ar.check_blocked()
    del ar, y_w


def run_layernorm_s2d(c, L):
    """Dense by the entry's own contract (ldy = 4 c): x and y are real 4.3 GB tensors.  Every image is compared bit for bit with
    the entry run on that image alone; float64 on sampled pixels."""
    k = c.kw
    b, h, w, cc = k["b"], k["h"], k["w"], k["c"]
    px = b * h * w
    assert px * cc * 4 > 1 << 32
    _need(2 * px * cc * 4 + 2 * O.GUARD + px // b * cc * 4 + (2 << 30))
    g = _gen(b * h + w)
    gamma, beta = _randn(g, cc, scale=0.5) + 1.0, _randn(g, cc, scale=0.3)
    x = torch.empty(px, cc, device="cuda")
    for i in range(b):                                                  # filled on the device, an image at a time
        x[i * h * w:(i + 1) * h * w].normal_(generator=g)
    ar, y = giant("y", (px // 4, 4 * cc), f32, ld=4 * cc, role="output")
    ar.arm()
    L.layernorm_rows_split_s2d(x, y, gamma, beta, b, h, w, cc)
    torch.cuda.synchronize()
    ar.check_blocked()
    one = torch.empty(h * w // 4, 4 * cc, device="cuda")
    for i in range(b):
        one.fill_(float("nan"))
        L.layernorm_rows_split_s2d(x[i * h * w:(i + 1) * h * w], one, gamma, beta, 1, h, w, cc)
        torch.cuda.synchronize()
        assert torch.equal(y[i * h * w // 4:(i + 1) * h * w // 4], one), f"{c.id}: image {i} differs from the entry run on it alone"
    # sampled source pixels -> their place in the space-to-depth rows
    S = sample_rows(px, byte_marks(cc * 4) + [bm * 4 for bm in byte_marks(4 * cc * 4)], tile=64)
    Sd = S.cuda()
    ref = _ln_ref(x[Sd], gamma, beta)
    pxx, q = S % w, S // w
    py, bi = q % h, q // h
    drow = ((bi * (h // 2) + py // 2) * (w // 2) + pxx // 2).cuda()
    slot = ((py & 1) * 2 + (pxx & 1)).cuda()
    got = unsplit(y.view(px // 4, 4, cc)[drow, slot]).cpu()
    err = assert_close(f"{c.id}: vs float64 on {S.numel()} sampled pixels", got, ref, *TOL_LN)
    print(f"{c.id}: {b} x {h} x {w} x {cc}: x {px * cc * 4 / 2 ** 30:.2f} GiB, y the same; max |d| {err:.3g}")
    del ar, y, x, one


# ================================================================================================ depthwise family (dense NHWC)
def _dw_ref(x, w7, bias, b, h, w, c):
    """float64 depthwise 7 x 7 + bias on the host: x [b * h * w, c] -> the same shape."""
    r = F.conv2d(x.double().cpu().view(b, h, w, c).permute(0, 3, 1, 2), w7.double().cpu().T.reshape(c, 1, 7, 7), bias.double().cpu(),
                 padding=3, groups=c)
    return r.permute(0, 2, 3, 1).reshape(b * h * w, c)


def _fill_normal(x, g, rows_per_block):
    for r in range(0, x.shape[0], rows_per_block):                       # on the device, block by block
        x[r:r + rows_per_block].normal_(generator=g)


def run_dwconv_batch(c, L):
    """(a) the batch index carries x and y past byte 2^31 and 2^32.  float64 on the first and last image and on the images on
    either side of both boundaries; every image bit-identical to the same entry run on four batch slices of 1.09 GB."""
    k = c.kw
    mode, b, h, w, cc = k["mode"], k["b"], k["h"], k["w"], k["c"]
    px = h * w
    img_bytes = px * cc * 4
    assert b * img_bytes > 1 << 32 and (1 << 31) % img_bytes == 0
    _need(15 << 30)
    g = _gen(b + len(mode))
    w7, bias = _randn(g, 49, cc, scale=1 / 7), _randn(g, cc, scale=0.3)
    gamma, beta = _randn(g, cc, scale=0.2) + 1.0, _randn(g, cc, scale=0.3)
    x = torch.empty(b * px, cc, device="cuda")
    _fill_normal(x, g, 130 * px)
    ar, y = giant("y", (b * px, cc), f32, ld=cc, role="output")
    variant = {"variant1": 1, "variant2": 2, "variant4": 4}.get(mode, 0)
    scale = 4.0

    def run(xs, ys, nb, part=None, stats=None):
        if mode == "ln":
            L.dwconv7_ln(xs, w7, bias, ys, gamma, beta, nb, h, w, cc, split=False)
        elif mode == "stats":
            L.dwconv7_stats(xs, w7, bias, ys, part, nb, h, w, cc, scale=scale)
            L.ln_stats_finalize(part, stats, nb * px, cc)
        else:
            L.dwconv7(xs, w7, bias, ys, nb, h, w, cc, variant=variant)

    part = torch.full((cc // 32, b * px, 2), float("nan"), device="cuda") if mode == "stats" else None
    stats = torch.full((b * px, 2), float("nan"), device="cuda") if mode == "stats" else None
    ar.arm()
    run(x, y, b, part, stats)
    torch.cuda.synchronize()
    ar.check_blocked()
    # ---- every image: four batch slices
    nb = b // 4
    ys = torch.empty(nb * px, cc, device="cuda")
    ps = torch.empty(cc // 32, nb * px, 2, device="cuda") if mode == "stats" else None
    ss = torch.empty(nb * px, 2, device="cuda") if mode == "stats" else None
    for s in range(4):
        r0, r1 = s * nb * px, (s + 1) * nb * px
        ys.fill_(float("nan"))
        run(x[r0:r1], ys, nb, ps, ss)
        torch.cuda.synchronize()
        assert torch.equal(y[r0:r1], ys), f"{c.id}: images [{s * nb}, {(s + 1) * nb}) differ from a batch slice of their own: {_first_diff(y[r0:r1], ys)}"
        if mode == "stats":
            assert torch.equal(part[:, r0:r1], ps), f"{c.id}: partial sums of slice {s} differ"
            assert torch.equal(stats[r0:r1], ss), f"{c.id}: row statistics of slice {s} differ"
    del ys, ps, ss
    # ---- float64 on the host: first, last, and the images on either side of byte 2^31 and 2^32
    imgs = [0, (1 << 31) // img_bytes - 1, (1 << 31) // img_bytes, (1 << 32) // img_bytes - 1, (1 << 32) // img_bytes, b - 1]
    rows = torch.cat([torch.arange(i * px, (i + 1) * px) for i in imgs]).cuda()
    xs = x[rows]
    d64 = _dw_ref(xs, w7, bias, len(imgs), h, w, cc)
    got = y[rows]
    if mode == "ln":
        # the fused kernel against LayerNorm(float64 conv): the conv's 1e-5 passes through the normalisation multiplied by
        # rstd * |gamma| (its largest value over the sampled rows), plus the LayerNorm's own 5e-6
        mu, var = d64.mean(dim=1, keepdim=True), d64.var(dim=1, unbiased=False, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + 1e-6)
        ref = (d64 - mu) * rstd * gamma.double().cpu() + beta.double().cpu()
        amp = float(rstd.max()) * float(gamma.abs().max())
        err = assert_close(f"{c.id}: vs float64 on images {imgs}", got.double().cpu(), ref, TOL_DW[0] * amp + TOL_LN[0], TOL_DW[1] * amp + TOL_LN[1])
        # and, as the existing test of the entry asserts, the bits of wd_dwconv7 followed by wd_layernorm_rows
        pair = torch.empty(len(imgs) * px, cc, device="cuda")
        L.dwconv7(xs, w7, bias, pair, len(imgs), h, w, cc)
        L.layernorm_rows(pair, pair, gamma, beta, len(imgs) * px, cc)
        torch.cuda.synchronize()
        assert torch.equal(got, pair), f"{c.id}: differs from wd_dwconv7 + wd_layernorm_rows on the sampled images"
    elif mode == "stats":
        err = assert_close(f"{c.id}: y_split vs float64 on images {imgs}", unsplit(got).cpu() / scale, d64, *TOL_DW)
        d = torch.empty(len(imgs) * px, cc, device="cuda")               # the fp32 pre-norm tensor whose rows the statistics describe
        L.dwconv7(xs, w7, bias, d, len(imgs), h, w, cc)
        torch.cuda.synchronize()
        dd = d.double().cpu()
        st = stats[rows].cpu()
        assert_close(f"{c.id}: row mean", st[:, 0], dd.mean(dim=1), *TOL_STATS_MEAN)
        assert_close(f"{c.id}: row rstd", st[:, 1], 1.0 / torch.sqrt(dd.var(dim=1, unbiased=False) + 1e-6), *TOL_STATS_RSTD)
    else:
        err = assert_close(f"{c.id}: vs float64 on images {imgs}", got.double().cpu(), d64, *TOL_DW)
    print(f"{c.id}: {b} x {h} x {w} x {cc}, x and y {b * img_bytes / 2 ** 30:.2f} GiB each; max |d| {err:.3g}")
    del ar, y, x, part, stats


def run_dwconv_image(c, L):
    """(b) one image whose (h + 8) * w * c * 4 passes 2^32: the LDS-DMA form does not apply (forcing it is refused) and h % 16 != 0,
    so production runs the 1 x 4-strip LDS tile kernel (variant 2's form; elementwise.hip, launch_dwconv7).  Bit for bit against
    the generic form (variant 1) run on four horizontal strips with their three halo rows — interior rows of a strip see exactly
    the pixels they see in the whole image —, float64 at the four corners and around the rows at byte 2^31 and 2^32."""
    k = c.kw
    h, w, cc = k["h"], k["w"], k["c"]
    row_bytes = w * cc * 4
    assert (h + 8) * row_bytes >= 1 << 32 and h * row_bytes > 1 << 32 and h % 16
    _need(15 << 30)
    g = _gen(h + w)
    w7, bias = _randn(g, 49, cc, scale=1 / 7), _randn(g, cc, scale=0.3)
    x = torch.empty(h * w, cc, device="cuda")
    _fill_normal(x, g, 128 * w)
    ar, y = giant("y", (h * w, cc), f32, ld=cc, role="output")
    assert L.LIB.wd_dwconv7_variant(x.data_ptr(), w7.data_ptr(), bias.data_ptr(), y.data_ptr(), 1, h, w, cc, 4, L.stream_ptr()) == O.UNSUPPORTED
    ar.arm()
    L.dwconv7(x, w7, bias, y, 1, h, w, cc)
    torch.cuda.synchronize()
    ar.check_blocked()
    n_strip = 4
    sh = h // n_strip
    assert sh * n_strip == h
    out = torch.empty((sh + 6) * w, cc, device="cuda")
    for s in range(n_strip):
        r0, r1 = s * sh, (s + 1) * sh
        a0, a1 = max(0, r0 - 3), min(h, r1 + 3)
        o = out[:(a1 - a0) * w]
        o.fill_(float("nan"))
        L.dwconv7(x[a0 * w:a1 * w], w7, bias, o, 1, a1 - a0, w, cc, variant=1)
        torch.cuda.synchronize()
        mine = o[(r0 - a0) * w:(r1 - a0) * w]
        assert torch.equal(y[r0 * w:r1 * w], mine), f"{c.id}: rows [{r0}, {r1}) differ from the generic form: {_first_diff(y[r0 * w:r1 * w], mine)}"
    # float64 on crops: rows at the top, around byte 2^31 and 2^32, at the bottom; columns at the left and right edge
    x3, y3 = x.view(h, w, cc), y.view(h, w, cc)
    worst = 0.0
    for rr in ((0, 8), ((1 << 31) // row_bytes - 4, (1 << 31) // row_bytes + 4), ((1 << 32) // row_bytes - 4, (1 << 32) // row_bytes + 4), (h - 8, h)):
        for cl in ((0, 8), (w - 8, w)):
            pad = torch.zeros(rr[1] - rr[0] + 6, cl[1] - cl[0] + 6, cc, dtype=f64)
            s0, s1, t0, t1 = max(0, rr[0] - 3), min(h, rr[1] + 3), max(0, cl[0] - 3), min(w, cl[1] + 3)
            pad[s0 - (rr[0] - 3):s1 - (rr[0] - 3), t0 - (cl[0] - 3):t1 - (cl[0] - 3)] = x3[s0:s1, t0:t1].double().cpu()
            ref = F.conv2d(pad.permute(2, 0, 1)[None], w7.double().cpu().T.reshape(cc, 1, 7, 7), bias.double().cpu(), groups=cc)[0].permute(1, 2, 0)
            worst = max(worst, assert_close(f"{c.id}: rows {rr} columns {cl} vs float64", y3[rr[0]:rr[1], cl[0]:cl[1]].double().cpu(), ref, *TOL_DW))
    print(f"{c.id}: 1 x {h} x {w} x {cc}: production = the 1 x 4-strip LDS tile kernel; forced variant 4 refused; max |d| {worst:.3g}")
    del ar, y, x, out, x3, y3


# ================================================================================================ score entries on the 256 x 256 kernel
def _sim_operands(g, rows, n_cls, dim, L):
    e = F.normalize(_randn(g, rows, dim), dim=1)
    t = F.normalize(_randn(g, n_cls, dim), dim=1)
    es = torch.empty(L.LIB.wd_split_weights_bytes(rows, dim), dtype=u8, device="cuda")
    L.split_weights_scaled(e, es)
    ts, unscale = L.split_weights(t)
    return e, t, es, ts, unscale


SEG_AFFINE = ((0.7, 0.58, 0.82), (-2.6, -2.2, -1.9))


def run_similarity(c, L):
    k = c.kw
    rows, n_cls, dim = k["rows"], k["n_cls"], k["dim"]
    g = _gen(rows + n_cls + k["seg_ends"][0])
    e, t, es, ts, unscale = _sim_operands(g, rows, n_cls, dim, L)
    seg = (k["seg_rows"], k["seg_ends"][0], k["seg_ends"][1], tuple(10.0 * s for s in SEG_AFFINE[0]), SEG_AFFINE[1])
    flag = torch.zeros(1, dtype=i32, device="cuda")
    o_c = torch.full((rows, n_cls), float("nan"), device="cuda")
    L.similarity_split(es, rows, ts, unscale, o_c, n_cls, dim, n_cls, seg=seg, range_flag=flag)
    torch.cuda.synchronize()
    S = sample_rows(rows, byte_marks(O.WIDE_LD * 4) + [seg[1], seg[2], seg[0]])
    Sd = S.cuda()
    ev = unsplit(es.view(f32).view(-1, dim)[Sd]).cpu()                  # the halves the kernel multiplies
    pos = S % seg[0]
    lvl = (pos >= seg[1]).long() + (pos >= seg[2]).long()
    tv = unsplit(ts.view(f32).view(-1, dim)[:n_cls]).cpu() * unscale
    y = torch.sigmoid(ev @ tv.T * torch.tensor(seg[3], dtype=f64)[lvl][:, None] + torch.tensor(seg[4], dtype=f64)[lvl][:, None])
    err = assert_close(f"{c.id}: compact launch vs float64 on {S.numel()} sampled rows", o_c[Sd].double().cpu(), y, *TOL_SIM_SPLIT)
    print(f"{c.id}: rows {rows} K {n_cls} dim {dim} seg {seg[:3]}; compact vs float64 max |d| {err:.3g}")
    ar, o_w = giant("out", (rows, n_cls), f32, ld=O.WIDE_LD, role="output")
    ar.arm()
    L.similarity_split(es, rows, ts, unscale, o_w, n_cls, dim, O.WIDE_LD, seg=seg, range_flag=flag)
    torch.cuda.synchronize()
    assert torch.equal(o_w, o_c), f"{c.id}: the wide launch differs from the compact one: {_first_diff(o_w, o_c)}"
    ar.check_blocked()
    assert int(flag.item()) == 0
    del ar, o_w


def run_fused(c, L):
    """The fused entries at a class offset (or a flat index) whose largest value is just below 2^31: the result of the same launch
    at offset 0, shifted — scores bit for bit, every class / index exactly.  The materialised scores of wd_similarity_split (held
    to float64 above and in tests/test_gpu_split.py) give the expected maxima."""
    import numpy as np
    from wedetect_amd import best as BS, groups as PG, sparse as SP, topn as TN
    k = c.kw
    rows, n_cls, dim = k["rows"], k["n_cls"], k["dim"]
    g = _gen(rows * 13 + n_cls)
    e, t, es, ts, unscale = _sim_operands(g, rows, n_cls, dim, L)
    seg = (rows, rows // 2, rows - 8, tuple(10.0 * s for s in SEG_AFFINE[0]), SEG_AFFINE[1])
    flag = torch.zeros(1, dtype=i32, device="cuda")
    scores = torch.full((rows, n_cls), float("nan"), device="cuda")
    L.similarity_split(es, rows, ts, unscale, scores, n_cls, dim, n_cls, seg=seg, range_flag=flag)
    off = k.get("cls_offset", 0)
    if c.entry == "wd_best_similarity_split":
        assert off + n_cls <= (1 << 31) - 1 < off + n_cls + 32
        key0, key1 = (torch.zeros(rows, dtype=i64, device="cuda") for _ in range(2))
        BS.best_similarity_split(es, rows, ts, unscale, n_cls, dim, key0, 0, seg=seg, range_flag=flag)
        BS.best_similarity_split(es, rows, ts, unscale, n_cls, dim, key1, off, seg=seg, range_flag=flag)
        torch.cuda.synchronize()
        s0, l0 = BS.unpack_key(key0.cpu().numpy().view(np.uint64))
        s1, l1 = BS.unpack_key(key1.cpu().numpy().view(np.uint64))
        want_s, want_l = scores.max(dim=1)
        single = ((scores == want_s[:, None]).sum(dim=1) == 1).cpu().numpy()                  # rows whose maximum is not tied
        assert np.array_equal(s0.view(np.uint32), want_s.cpu().numpy().view(np.uint32))
        assert single.sum() > rows // 2 and np.array_equal(l0[single], want_l.cpu().numpy()[single])
        assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32)) and np.array_equal(l1.astype(np.int64), l0.astype(np.int64) + off)
        assert int(l1.max()) > (1 << 31) - 1 - 2 * n_cls
    elif c.entry == "wd_topn_similarity_split":
        n_top = 4
        key0, key1 = (torch.zeros(rows, n_top, dtype=i64, device="cuda") for _ in range(2))
        TN.topn_similarity_split(es, rows, ts, unscale, n_cls, dim, n_top, key0, 0, seg=seg, range_flag=flag)
        TN.topn_similarity_split(es, rows, ts, unscale, n_cls, dim, n_top, key1, off, seg=seg, range_flag=flag)
        torch.cuda.synchronize()
        s0, l0 = TN.unpack(key0.cpu().numpy().view(np.uint64))
        s1, l1 = TN.unpack(key1.cpu().numpy().view(np.uint64))
        want_s, want_l = torch.sort(scores, dim=1, descending=True, stable=True)
        assert np.array_equal(s0.view(np.uint32), want_s[:, :n_top].cpu().numpy().view(np.uint32))
        distinct = (want_s[:, :n_top] != want_s[:, 1:n_top + 1]).all(dim=1).cpu().numpy()      # rows without a tie among the first n + 1
        assert distinct.sum() > rows // 2 and np.array_equal(l0[distinct], want_l[:, :n_top].cpu().numpy()[distinct])
        assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32)) and np.array_equal(l1.astype(np.int64), l0.astype(np.int64) + off)
    elif c.entry == "wd_group_similarity_split":
        plan = PG.PromptGroups.from_sizes([2] * (n_cls // 2))                                  # 16 classes per bin of 32 rows
        assert plan.K_pad == n_cls
        G = plan.G
        go, bf = plan.group_of.cuda(), plan.bin_first.cuda()
        o0 = torch.full((rows, G), float("nan"), device="cuda")
        PG.group_similarity_split(es, rows, ts, unscale, n_cls, dim, go, bf, 0, o0, G, G, seg=seg, range_flag=flag)
        torch.cuda.synchronize()
        assert torch.equal(o0, plan.class_max(scores)), "class maxima at offset 0 differ from the maxima of the materialised scores"
        if "ldo" in k:                                                                          # [rows][G] with a wide row stride
            ar, o1 = giant("out", (rows, G), f32, ld=k["ldo"], role="output")
            ar.arm()
            PG.group_similarity_split(es, rows, ts, unscale, n_cls, dim, go, bf, 0, o1, k["ldo"], G, seg=seg, range_flag=flag)
            torch.cuda.synchronize()
            assert torch.equal(o1, o0), f"{c.id}: the wide launch differs from the compact one: {_first_diff(o1, o0)}"
            ar.check_blocked()
            del ar, o1
        else:                                                                                   # the plan's rows placed at bank row `off`
            assert off % 32 == 0 and off + n_cls <= (1 << 31) - 1 < off + n_cls + 32
            _need(((off + n_cls) * 4) + (3 << 30))
            G_all = 1000 + G                                                                    # classes before this chunk: 1000
            go_big = torch.zeros(off + n_cls, dtype=i32, device="cuda")
            go_big[off:] = go + 1000
            bf_big = torch.zeros((off + n_cls) // 32 + 1, dtype=i32, device="cuda")
            bf_big[off // 32:] = bf + 1000
            o1 = torch.full((rows, G_all), float("nan"), device="cuda")
            PG.group_similarity_split(es, rows, ts, unscale, n_cls, dim, go_big, bf_big, off, o1, G_all, G_all, seg=seg, range_flag=flag)
            torch.cuda.synchronize()
            assert torch.equal(o1[:, 1000:], o0) and bool(torch.isnan(o1[:, :1000]).all())
            del go_big, bf_big
    elif c.entry == "wd_sparse_similarity_split":
        rpi, total = k["rows_per_img"], k["n_cls_total"]
        assert rows == rpi and rpi * total < 1 << 31 <= rpi * (total + 1)
        off, cap, thr = total - n_cls, 1 << 18, 0.05
        lists, states = [], []
        for o_, tot in ((0, n_cls), (off, total)):
            lst = torch.full((1, cap), -1, dtype=i64, device="cuda")
            st = torch.zeros(1, 2, dtype=i32, device="cuda")
            SP.sparse_similarity_split(es, rows, ts, unscale, n_cls, dim, rpi, tot, thr, lst, cap, st, o_, seg=seg, range_flag=flag)
            torch.cuda.synchronize()
            lists.append(lst.cpu().numpy().view(np.uint64)[0])
            states.append(st.cpu().numpy()[0])
        n_cand = int((scores > thr).sum())
        assert 0 < n_cand < cap and int(states[0][0]) == int(states[1][0]) == n_cand and not states[0][1] and not states[1][1]
        k0, k1 = np.sort(lists[0][:n_cand]), np.sort(lists[1][:n_cand])
        bits0, flat0 = (k0 >> np.uint64(32)).astype(np.uint32), (k0 & np.uint64(0xFFFFFFFF)).astype(np.int64)
        want = (flat0 // n_cls) * total + off + flat0 % n_cls
        exp = np.sort((bits0.astype(np.uint64) << np.uint64(32)) | want.astype(np.uint64))
        assert np.array_equal(k1, exp), "candidates at the large flat index differ from the ones at offset 0, shifted"
        sc = scores.cpu().numpy()
        assert np.array_equal(~bits0, sc[flat0 // n_cls, flat0 % n_cls].view(np.uint32)), "list scores differ from the materialised ones"
        assert int(want.max()) > (1 << 31) - 1 - 2 * total and int(want.max()) < 1 << 31
    else:
        raise KeyError(c.entry)
    assert int(flag.item()) == 0
    print(f"{c.id}: rows {rows} K {n_cls} dim {dim} offset {off}: shifted result exact")


# ================================================================================================ retrieval: the chunk seams
def run_retrieval(c, L):
    k = c.kw
    dim, n_cls = k["dim"], k["n_cls"]
    chunk = O.retrieval_chunk(dim)
    seams = list(range(chunk, n_cls, chunk))
    assert seams, "the case has no seam"
    n_img, rows, counts = 3, 20, (20, 0, 1)
    bank_bytes = n_cls * dim * 4
    _need(2 * bank_bytes + 2 * O.GUARD + (2 << 30))
    g = _gen(dim + n_cls)
    e = F.normalize(_randn(g, n_img, rows, dim), dim=2)
    scale = _randn(g, n_img, rows, scale=0.1) + 2.0
    bias = _randn(g, n_img, rows, scale=0.2) - 2.0
    count = torch.tensor(counts, dtype=i32, device="cuda")
    bank = torch.empty(n_cls, dim, device="cuda")
    amax = 0.0
    for c0 in range(0, n_cls, 1 << 16):                                  # filled on the device, rows normalised in blocks
        blk = bank[c0:c0 + (1 << 16)]
        blk.normal_(generator=g)
        blk.div_(blk.norm(dim=1, keepdim=True))
        amax = max(amax, float(blk.abs().max()))
    del blk
    w_scale = 2.0 ** (13 - math.floor(math.log2(amax)))                  # lib.split_weights, without its whole-bank temporary
    ts = torch.empty(L.LIB.wd_split_weights_bytes(n_cls, dim), dtype=u8, device="cuda")
    L.check(L.LIB.wd_split_weights_padded(bank.data_ptr(), n_cls, dim, w_scale, ts.data_ptr(), L.stream_ptr()), "wd_split_weights_padded")
    torch.cuda.synchronize()
    unscale = 1.0 / w_scale
    del bank
    bits = _checksum(ts)
    flag = torch.zeros(1, dtype=i32, device="cuda")
    ar, out = giant_small("out", (n_img, n_cls), f32)
    ar.arm()
    L.retrieval_max_split(e, (ts, unscale), scale, bias, count, out, n_img, rows, n_cls, dim, range_flag=flag)
    torch.cuda.synchronize()
    ar.check_blocked()
    assert _checksum(ts) == bits, "the split bank changed"
    assert int(flag.item()) == 0
    assert bool((out[1] == 0).all()), "an image without regions must score exactly 0 everywhere"
    # float64 on sampled classes
    row_b = dim * 4
    S = sample_rows(n_cls, [*seams, (1 << 31) // row_b] + ([(1 << 32) // row_b] if (1 << 32) // row_b < n_cls else []), tile=64)
    Sd = S.cuda()
    tv = unsplit(ts.view(f32).view(-1, dim)[Sd]).cpu() * unscale          # the halves the kernel multiplies
    es = torch.empty(L.LIB.wd_split_weights_bytes(n_img * rows, dim), dtype=u8, device="cuda")
    L.split_weights_scaled(e.view(-1, dim), es)
    ev = unsplit(es.view(f32).view(-1, dim)[:n_img * rows]).cpu().view(n_img, rows, dim)
    ref = torch.zeros(n_img, S.numel(), dtype=f64)
    for i, cnt in enumerate(counts):
        if cnt:
            logit = ev[i, :cnt] @ tv.T * torch.exp(scale[i, :cnt].double().cpu())[:, None] + bias[i, :cnt].double().cpu()[:, None]
            ref[i] = torch.sigmoid(logit).max(dim=0).values
    err = assert_close(f"{c.id}: vs float64 on {S.numel()} sampled classes", out[:, Sd].double().cpu(), ref, *TOL_RETR_SPLIT)
    # every class: the bank cut at the seams into separate calls (exact: the shard test of tests/test_gpu_split.py)
    cuts = [0, *seams, n_cls]
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        part = torch.full((n_img, c1 - c0), float("nan"), device="cuda")
        t_ptr = ts[c0 * dim * 4:]
        L.retrieval_max_split(e, (t_ptr, unscale), scale, bias, count, part, n_img, rows, c1 - c0, dim, range_flag=flag)
        torch.cuda.synchronize()
        assert torch.equal(out[:, c0:c1], part), f"{c.id}: classes [{c0}, {c1}) differ from a call of their own: {_first_diff(out[:, c0:c1], part)}"
    print(f"{c.id}: dim {dim} n_cls {n_cls} chunk {chunk} seams {seams} bank {bank_bytes / 2 ** 30:.2f} GiB; max |d| {err:.3g}")
    del ar, out, ts


def _checksum(t: torch.Tensor) -> int:
    """Sum of the 32-bit words of a large buffer, in blocks (no temporary of the buffer's size)."""
    w = t.view(i32)
    return sum(int(w[a:a + (1 << 26)].sum()) for a in range(0, w.numel(), 1 << 26))


def giant_small(name, shape, dtype):
    """An Arena around a compact output with 2 GiB of guard on each side (the output itself is small)."""
    esz = torch.empty((), dtype=dtype).element_size()
    cap = math.prod(shape) * esz + 2 * O.GUARD + (2 << 20)
    _need(cap + (1 << 30))
    ar = Arena(cap, "cuda", 0xFF)
    return ar, ar.take(name, shape, dtype, role="output", guard_bytes=O.GUARD)


# ================================================================================================ top-k past 2^31 elements
def run_topk(c, L):
    import numpy as np
    k = c.kw
    batch, n, nms_pre, thr = k["batch"], k["n"], k["nms_pre"], k["thr"]
    # element offsets 2^30 and 2^31 (bytes 2^32 and 2^33) and 2^31 + 2^29, next to the tensor's end: 2^31 + 2^30 lies beyond the
    # 5 * (2^29 + 256) = 2.68e9 elements of this shape
    CROSSINGS = (1 << 30, 1 << 31, (1 << 31) + (1 << 29))
    assert batch * n > CROSSINGS[-1] + 3 > 1 << 31
    _need(batch * n * 4 + (3 << 30))
    scores = torch.zeros(batch, n, device="cuda")
    rng = np.random.default_rng(5)
    planted = []
    for bi in range(batch):
        if bi == 2:                                                      # an empty image (no crossing falls into it)
            planted.append((np.zeros(0, np.int64), np.zeros(0, np.float32)))
            continue
        want = 700 if bi == 1 else 1500                                  # one image with fewer than nms_pre
        idx = {0, n - 1}
        near = set()
        for cross in CROSSINGS:                                          # element offsets of the whole tensor
            loc = cross - bi * n
            near.update(i for i in range(loc - 3, loc + 3) if 0 <= i < n)
        idx |= near
        while len(idx) < want:
            idx.update(int(v) for v in rng.integers(0, n, want - len(idx)))
        idx = np.array(sorted(idx), np.int64)
        val = rng.uniform(0.01, 0.99, idx.size).astype(np.float32)
        val[::7] = np.float32(0.5)                                       # ties: index ascending decides
        val[:2] = np.float32(0.999)                                      # the first element among the best
        val[-1] = np.float32(0.9995) if bi != 1 else np.float32(0.0005)  # the last element: the best / below the threshold
        val[np.isin(idx, sorted(near))] = np.float32(0.95)               # the crossing elements are kept, tied among themselves
        planted.append((idx, val))
        scores[bi, torch.from_numpy(idx).cuda()] = torch.from_numpy(val).cuda()
    cap = L.topk_capacity(nms_pre)
    ws = torch.empty(L.topk_workspace_bytes(batch, n, nms_pre), dtype=u8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    out_idx = torch.full((batch, cap), -7, dtype=i32, device="cuda")
    out_score = torch.full((batch, cap), float("nan"), device="cuda")
    out_count = torch.full((batch,), -7, dtype=i32, device="cuda")
    L.topk_candidates(scores, batch, n, thr, nms_pre, out_idx, out_score, out_count, ws)
    torch.cuda.synchronize()
    gi, gs, gc_ = out_idx.cpu().numpy(), out_score.cpu().numpy(), out_count.cpu().numpy()
    crossing = 0
    for bi, (idx, val) in enumerate(planted):
        keep = val > np.float32(thr)
        idx, val = idx[keep], val[keep]
        order = np.lexsort((idx, -val.astype(np.float64)))[:nms_pre]     # score descending, index ascending
        cnt = order.size
        assert int(gc_[bi]) == cnt, f"image {bi}: count {int(gc_[bi])} vs {cnt}"
        assert np.array_equal(gi[bi, :cnt], idx[order].astype(np.int32)), f"image {bi}: indices differ"
        assert np.array_equal(gs[bi, :cnt].view(np.uint32), val[order].view(np.uint32)), f"image {bi}: scores differ"
        assert bool((gi[bi, cnt:] == -1).all()) and bool((gs[bi, cnt:] == 0).all())
        crossing += int(np.isin(idx[order] + bi * n, [x + d for x in CROSSINGS for d in range(-3, 3)]).sum())
    assert int(gc_[2]) == 0 and 0 < int(gc_[1]) < nms_pre and crossing == 6 * len(CROSSINGS)
    print(f"{c.id}: counts {gc_.tolist()}, {crossing} kept candidates next to the element offsets 2^30 / 2^31 / 2^31 + 2^29")
    del scores, ws


RUNNERS = {"dwconv_batch": run_dwconv_batch, "dwconv_image": run_dwconv_image, "gemm": run_gemm, "conv": run_conv, "layernorm": run_layernorm, "layernorm_s2d": run_layernorm_s2d, "similarity": run_similarity,
           "fused": run_fused, "retrieval": run_retrieval, "topk": run_topk}


@pytest.mark.parametrize("c", CORRECT, ids=[c.id for c in CORRECT])
def test_offsets(c):
    L = _L()
    _release()
    held = torch.cuda.memory_allocated()                                # what earlier tests of the process still hold is not this case's
    torch.cuda.reset_peak_memory_stats()
    try:
        RUNNERS[c.family](c, L)
    finally:
        _release()
    peak = torch.cuda.max_memory_allocated() - held
    print(f"{c.id}: peak device memory {peak / 2 ** 30:.2f} GiB (the process held {held / 2 ** 30:.2f} GiB before it)")
    assert peak <= 16 << 30, f"the case held {peak / 2 ** 30:.2f} GiB, more than 16 GiB"
