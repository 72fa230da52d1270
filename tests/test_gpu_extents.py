"""Guard-band tests (GPU): every entry point of include/wedetect_hip.h runs with its operands carved from a tests/arena.py
Arena, at the shapes where tail / halo / staging code goes wrong.  Per case:

  1. no stray store, inputs unchanged            — Arena.check() after the launch;
  2. independence of the surroundings            — the case runs with every guard / spare column / row between the documented
     extent and the allocation filled with 0x00 and again with 0xFF (NaN as fp32 and fp16, -1 as int32, 255 as uint8; 0x7F
     around integer outputs whose contract names a -1 filler): outputs bit-identical, finite, every range flag 0.  Outputs
     start out holding the pattern, so an element the kernel should have written and did not is a NaN in the second run;
  3. workspace hygiene                            — workspaces start as 0xFF bytes except what the header says must be zero;
     bit-identical to a zero-filled workspace; the flag page of the park workspace all-zero again; a second launch on the
     dirty workspace gives the same bits;
  4. value                                        — one comparison with an fp64 / oracle reference at the tolerance the
     existing test of that entry point asserts (each constant names its source line).

The extent of a buffer is what the header documents.  READS outside an extent that influence no result cannot be observed
without a fault and are out of scope; so are stores farther away than the guard (tests/arena.py).

tests/test_cpu_arena.py asserts on the CPU that every wd_* function taking device memory has a case here.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.arena import Arena, GuardViolation
from tests.util import assert_close

pytestmark = pytest.mark.gpu

f32, i32, u8, f64, i64 = torch.float32, torch.int32, torch.uint8, torch.float64, torch.int64

# tolerances of the existing tests, reused unchanged (atol, rtol)
TOL_GEMM_F32 = (2e-5, 2e-5)         # tests/test_gpu_kernels.py:39  test_gemm_plain
TOL_GEMM_F32_EPI = (3e-5, 3e-5)     # tests/test_gpu_kernels.py:54, 112, 126  activation / residual / conv / deconv
TOL_SIM_F32 = (2e-6, 1e-5)          # tests/test_gpu_kernels.py:78  similarity epilogue (sigmoid)
TOL_SPLIT = (6e-6, 2e-6)            # tests/test_gpu_split.py:64, 110  fp16x3 GEMM / conv vs float64
REL_CONV3 = 2e-5                    # tests/test_gpu_split.py:673  |d| < 2e-5 * max|ref| (row-sharing 3 x 3 kernels)
REL_MLP = 2e-5                      # tests/test_gpu_split.py:791, 832, 1010  fused MLPs: |d| < 2e-5 * max|ref|
TOL_DW = (1e-5, 1e-5)               # tests/test_gpu_kernels.py:192  depthwise 7 x 7
TOL_LN = (5e-6, 5e-6)               # tests/test_gpu_kernels.py:229  LayerNorm rows
TOL_STEM = (2e-5, 2e-5)             # tests/test_gpu_kernels.py:171  fused stem
TOL_L2 = (1e-6, 1e-6)               # tests/test_gpu_kernels.py:238
TOL_DFL = (2e-4, 1e-6)              # tests/test_gpu_kernels.py:257
TOL_RETR = (2e-6, 1e-5)             # tests/test_gpu_kernels.py:524
TOL_RETR_SPLIT = (3e-6, 0.0)        # tests/test_gpu_split.py:330
TOL_SIM_SPLIT = (2e-6, 1e-6)        # tests/test_gpu_split.py:442-443 (sigmoid)
TOL_STATS_MEAN = (1e-6, 2e-6)       # tests/test_gpu_split.py:903
TOL_STATS_RSTD = (0.0, 3e-6)        # tests/test_gpu_split.py:904
TOL_ATTN = (2e-6, 1e-6)             # tests/test_gpu_text.py:75
TOL_TEXT = (2e-5, 0.0)              # tests/test_gpu_text.py:55 (the tower whose first kernel this is)
TOL_XATTN = (2e-6, 1e-5)            # tests/test_gpu_bricks.py:138
TOL_BRICK = (1e-3, 0.0)             # tests/test_gpu_bricks.py:90 (the block whose last kernel this is)
TOL_GROUPED = (2e-6, 1e-5)          # tests/test_gpu_per_image_bank.py (the fp32 similarity tolerance, test_gpu_kernels.py:78)


def _L():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wedetect_amd import lib
    return lib


def _rand(seed, *shape, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def split_cpu(x: torch.Tensor) -> torch.Tensor:
    """fp32 rows [r, k] (k % 8 == 0) -> the fp16 hi/lo group format ([8 x hi | 8 x lo] per 8 elements) in a float32-typed
    tensor of the same shape (include/wedetect_hip.h, WD_SPLIT_A)."""
    r, k = x.shape
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return torch.stack([hi.view(r, k // 8, 8), lo.view(r, k // 8, 8)], dim=2).reshape(r, 2 * k).contiguous().view(f32)


def unsplit(buf: torch.Tensor) -> torch.Tensor:
    """hi + lo of a split-format tensor [r, k] (float32-typed) as float64."""
    r, k = buf.shape
    h = buf.contiguous().view(torch.float16).view(r, k // 8, 2, 8)
    return (h[:, :, 0].double() + h[:, :, 1].double()).reshape(r, k)


def _act64(y, act, L):
    return {L.ACT_NONE: lambda v: v, L.ACT_RELU: torch.relu, L.ACT_SILU: F.silu, L.ACT_GELU: F.gelu}[act](y)


# ------------------------------------------------------------------------------------------------ harness
@dataclass
class Run:
    launch: Callable[[], None]
    outs: Callable[[], Dict[str, torch.Tensor]]          # after a launch: name -> the defined part of an output
    value: Callable[[Dict[str, torch.Tensor]], None]     # the one comparison with the reference
    info: str = ""
    flags: List[torch.Tensor] = field(default_factory=list)
    zero_page: Optional[torch.Tensor] = None             # bytes that must be zero again after every launch
    finite: bool = True
    has_ws: bool = False


class Ctx:
    """What a case uses to carve its operands."""

    def __init__(self, ar: Arena, ws_fill: int, L):
        self.ar, self.ws_fill, self.L = ar, ws_fill, L
        self.has_ws = False
        self.shrinks: List[tuple] = []

    def inp(self, name, data, *, ld=None, mis=16, bs=None):
        return self.ar.take(name, data.shape, data.dtype, ld=ld, misalign=mis, role="input", data=data, batch_stride=bs)

    def out(self, name, shape, dtype=f32, *, ld=None, mis=16, fillers=(), bs=None):
        return self.ar.take(name, shape, dtype, ld=ld, misalign=mis, role="output", fillers=fillers, batch_stride=bs)

    def inout(self, name, data, *, ld=None, mis=16):
        return self.ar.take(name, data.shape, data.dtype, ld=ld, misalign=mis, role="inout", data=data)

    def ws(self, name, nbytes, *, zero_prefix=0, mis=16, row_pitch=None):
        """A workspace of ``nbytes``: 0xFF (or what the run asks for) except the first ``zero_prefix`` bytes."""
        self.has_ws = True
        t = self.ar.take(name, (int(nbytes),), u8, misalign=mis, role="workspace", fill=self.ws_fill, row_pitch=row_pitch)
        if zero_prefix:
            t[:zero_prefix] = 0
        return t

    def flag(self, name="range_flag"):
        return self.ar.take(name, (1,), i32, misalign=4, role="inout", data=torch.zeros(1, dtype=i32))


@dataclass
class Case:
    entry: str
    name: str
    fn: Callable[[Ctx], Run]
    cap: int = 64 << 20                                   # grown by execute() when a case needs more

    @property
    def id(self) -> str:
        return f"{self.entry}[{self.name}]"


CASES: List[Case] = []

EXEMPT = {
    "wd_abi_version": "no memory",
    "wd_strerror": "no memory",
    "wd_sizeof_conv_gemm": "no memory",
    "wd_split_weights_bytes": "size query, no memory",
    "wd_topk_workspace_bytes": "size query, no memory",
    "wd_topk_capacity": "size query, no memory",
    "wd_nms_workspace_bytes": "size query, no memory",
    "wd_p8_workspace_bytes": "size query, no memory",
    "wd_det_match_workspace_bytes": "size query, no memory",
    "wd_det_match_lds_bytes": "size query, no memory",
    "wd_recall_scratch_floats": "size query, no memory",
    "wd_conv_gemm_config": "name query, no memory",
    "wd_conv_gemm_split_config": "name query, no memory",
    "wd_time_next_gemm": "takes two host event handles, no device memory",
    "wd_probe_lds_dma": "diagnostic micro-benchmark, not on the product path",
    "wd_probe_issue": "diagnostic micro-benchmark, not on the product path",
}


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


_CAPACITY: Dict[str, int] = {}


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(-1).view(u8)


def _snapshot(run: Run) -> Dict[str, torch.Tensor]:
    return {k: v.clone(memory_format=torch.contiguous_format) for k, v in run.outs().items()}


def _same(a: Dict[str, torch.Tensor], b: Dict[str, torch.Tensor], what: str) -> None:
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        if not torch.equal(_bits(a[k]), _bits(b[k])):
            d = (_bits(a[k]) != _bits(b[k])).nonzero().flatten()
            esz = a[k].element_size()
            raise AssertionError(f"{what}: output {k!r} differs in {d.numel()} byte(s); first element {int(d[0]) // esz}, last "
                                 f"{int(d[-1]) // esz} of {a[k].numel()} (shape {tuple(a[k].shape)})")


def execute(c: Case, pattern: int, ws_fill: int, shrink=None):
    """One run of a case in one surrounding: carve, arm, launch, check; relaunch on the dirty workspace."""
    L = _L()
    cap = _CAPACITY.get(c.id, c.cap)
    while True:
        try:
            ar = Arena(cap, "cuda", pattern)
            ctx = Ctx(ar, ws_fill, L)
            run = c.fn(ctx)
            break
        except MemoryError:                                # guards are 256 row pitches per side: a case with wide rows needs more
            if cap >= 4 << 30:
                raise
            ar = ctx = None
            cap *= 2
    _CAPACITY[c.id] = cap                                  # the later runs of the case start at the size that fitted
    run.has_ws = ctx.has_ws
    if shrink is not None:
        shrink(ar)
    ar.arm()
    run.launch()
    torch.cuda.synchronize()
    if shrink is not None:
        return run, ar.violations(), None
    ar.check()
    outs = _snapshot(run)
    flags = [int(f.item()) for f in run.flags]
    if run.zero_page is not None:
        assert int(run.zero_page.max()) == 0, "the zero page of the workspace must be zero again after a launch"
    if ctx.has_ws:
        run.launch()
        torch.cuda.synchronize()
        ar.check()
        _same(outs, _snapshot(run), "second launch on the dirty workspace")
        flags = [max(a, int(f.item())) for a, f in zip(flags, run.flags)]
        if run.zero_page is not None:
            assert int(run.zero_page.max()) == 0, "the zero page of the workspace must be zero again after the second launch"
    return run, outs, flags


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_extents(c):
    run0, o0, f0 = execute(c, 0x00, 0xFF)
    run1, o1, f1 = execute(c, 0xFF, 0xFF)
    assert not any(f0) and not any(f1), f"range / error flags raised: surroundings 0x00 {f0}, 0xFF {f1}"
    _same(o0, o1, "surroundings 0x00 vs 0xFF")
    if run0.finite:
        for k, v in o1.items():
            if v.dtype.is_floating_point:
                assert bool(torch.isfinite(v).all()), f"output {k!r}: {int((~torch.isfinite(v)).sum())} non-finite element(s)"
    if run0.has_ws:
        _, o2, f2 = execute(c, 0x00, 0x00)
        assert not any(f2)
        _same(o0, o2, "workspace 0xFF vs zero-filled")
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, flags 0" + (", workspace hygiene ok" if run0.has_ws else ""))


# ================================================================================================ GEMM family
def _gemm(ctx: Ctx, *, b=1, h=1, w=None, m=None, cin, n, kh=1, stride=1, pad=0, kind="f32", cfg=None, flags=0, lda_x=0, ldc_x=0,
          act=0, res=None, c2=False, deconv=False, cbs_x=None, splits=0, ws=None, c_mis=16, seg=None, sigmoid=False, ln=False,
          want_cfg=None, tol=None, rel=None, bias=True, padded_w=False, c_split_scale=1.0, a_scale=1.0, seed=1, res_x=4):
    """One wd_conv_gemm / _tuned / _split / _split_ws launch.  kind: "f32" (cfg = tuned tile or None) or "split"; flags as the
    ABI; lda_x / ldc_x: spare columns of a / c; res: None | "sep" | "inplace"; cbs_x: extra rows per image (c_batch_stride);
    ws: None | "splitk" | "park"; ln: the LayerNorm fold (ln_stats / ln_u)."""
    L = ctx.L
    if w is None:
        w = m
    rows_in = b * h * w
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kh) // stride + 1
    M, k = b * ho * wo, kh * kh * cin
    SA, SC = bool(flags & L.SPLIT_A), bool(flags & L.SPLIT_C)
    x = _rand(seed, rows_in, cin, scale=1.0)
    wt = _rand(seed + 1, n, k, scale=k ** -0.5)
    bs_ = _rand(seed + 2, n, scale=0.3) if bias else None
    a_val = unsplit(split_cpu(x)) if SA else x.double()                  # what the kernel's operand really holds
    a = ctx.inp("a", split_cpu(x) if SA else x, ld=cin + lda_x)
    bias_t = ctx.inp("bias", bs_) if bias else None
    kw = dict(batch=b, hin=h, win=w, cin=cin, lda=cin + lda_x, kh=kh, kw=kh, stride=stride, pad=pad, n=n, act=act,
              sigmoid=sigmoid, seg=seg, a_scale=a_scale, c_split_scale=c_split_scale)
    if kind == "f32":
        wd = ctx.inp("w", wt)
        kw.update(tuned_cfg=cfg)
    else:
        # wd_split_weights writes exactly n rows; the rows up to wd_split_weights_bytes() keep the surroundings' pattern
        scale = 2.0 ** (13 - math.floor(math.log2(float(wt.abs().max()))))
        nbytes = int(L.LIB.wd_split_weights_bytes(n, k))
        wsp = ctx.ar.take("w_split", (nbytes,), u8, misalign=16, role="input", row_pitch=(k + 15) // 16 * 64)
        w_dev = wt.cuda()
        fn = L.LIB.wd_split_weights_padded if padded_w else L.LIB.wd_split_weights
        L.check(fn(w_dev.data_ptr(), n, k, scale, wsp.data_ptr(), L.stream_ptr()), "wd_split_weights")
        torch.cuda.synchronize()
        wd = None
        kw.update(w_split=(wsp, 1.0 / scale), split_cfg=-1 if cfg is None else cfg, split_flags=flags)
    # ---- output addressing
    ref_rows = M
    if deconv:
        co = n // 4
        ldc = co + ldc_x
        c = ctx.out("c", (b * 2 * ho * 2 * wo, co), ld=ldc, mis=c_mis)
        kw.update(out_mode=L.OUT_DECONV2X2)
    elif cbs_x is not None:
        ldc = n + ldc_x
        c = ctx.out("c", (b, ho * wo, n), ld=ldc, mis=c_mis, bs=ho * wo + cbs_x)
        kw.update(c_batch_stride=ho * wo + cbs_x)
    else:
        ldc = n + ldc_x
        c = ctx.out("c", (M, n), ld=ldc, mis=c_mis) if res != "inplace" else None
    r = None
    if res is not None:
        r = _rand(seed + 3, M, n)
        if res == "inplace":
            c = ctx.inout("c", r, ld=ldc, mis=c_mis)
            r_dev = r.cuda()
            kw.update(res=c, ldres=ldc, res_alpha=1.0)
        else:
            kw.update(res=ctx.inp("res", r, ld=n + res_x), ldres=n + res_x, res_alpha=0.625)
    kw.update(ldc=ldc)
    c2_t = None
    if c2:
        c2_t = ctx.out("c2", (b, ho * wo, n), ld=n + 4, bs=ho * wo + cbs_x) if cbs_x is not None else ctx.out("c2", (M, n), ld=n + 4)
        kw.update(c2=c2_t, ldc2=n + 4)
    flag = ctx.flag() if kind == "split" else None
    if flag is not None:
        kw.update(range_flag=flag)
    stats = u_vec = None
    if ln:
        mu = a_val.mean(dim=1)
        rstd = 1.0 / torch.sqrt(a_val.var(dim=1, unbiased=False) + 1e-6)
        stats = torch.stack([mu, rstd], dim=1).float().contiguous()
        u_vec = wt.double().sum(dim=1).float()
        kw.update(ln_stats=ctx.inp("ln_stats", stats, mis=8), ln_u=ctx.inp("ln_u", u_vec))
    zero_page = None
    if ws == "splitk":
        kw.update(workspace=ctx.ws("workspace", 4 * (splits or 8) * M * n, row_pitch=4 * n), k_splits=splits)
    elif ws == "park":
        wsb = ctx.ws("workspace", L.p8_workspace_bytes(), zero_prefix=4096)
        zero_page = wsb[:4096]
        kw.update(workspace=wsb, k_splits=0)

    def launch():
        if res == "inplace":
            c.copy_(r_dev)
        L.conv_gemm(a, wd, bias_t, c, **kw)

    def outs():
        o = {"c": c}
        if c2_t is not None:
            o["c2"] = c2_t
        return o

    def value(o):
        if kh == 1 and stride == 1:
            y = a_val @ wt.double().T
        else:
            xi = a_val.view(b, h, w, cin).permute(0, 3, 1, 2)
            wi = wt.double().view(n, kh, kh, cin).permute(0, 3, 1, 2)
            y = F.conv2d(xi, wi, None, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(M, n)
        if ln:
            y = stats[:, 1:2].double() * (y - stats[:, 0:1].double() * u_vec.double()[None, :])
        if bias:
            y = y + bs_.double()
        y = _act64(y, act, L)
        if seg is not None:
            pos = torch.arange(M) % seg[0]
            lvl = (pos >= seg[1]).long() + (pos >= seg[2]).long()
            y = y * torch.tensor(seg[3], dtype=f64)[lvl][:, None] + torch.tensor(seg[4], dtype=f64)[lvl][:, None]
        if sigmoid:
            y = torch.sigmoid(y)
        if r is not None:
            y = y + (1.0 if res == "inplace" else 0.625) * r.double()
        got = o["c"].cpu()
        if deconv:
            co_ = n // 4
            y = y.view(b, ho, wo, 2, 2, co_).permute(0, 1, 3, 2, 4, 5).reshape(b * 2 * ho * 2 * wo, co_)
        got = got.reshape(y.shape)
        g64 = unsplit(got) / c_split_scale if SC else got.double()
        at, rt = (rel * float(y.abs().max()), 0.0) if rel is not None else tol
        assert_close(f"{info} c", g64, y, at, rt)
        if c2_t is not None:
            assert_close(f"{info} c2", o["c2"].cpu().reshape(y.shape), y, at, rt)

    plain = kh == 1 and stride == 1 and pad == 0
    special = deconv or cbs_x is not None or seg is not None or sigmoid
    if kind == "f32":
        picked = L.gemm_config(M, n, k)
    elif SA and (not plain or special or c2 or (SC and res is not None)):
        picked = L.gemm_config(M, n, k, split=True, dma=True, conv3=(kh == 3 and stride == 1))
    elif SA:
        picked = L.gemm_config(M, n, k, split=True, presplit=True, park=(ws == "park"))
    else:
        picked = L.gemm_config(M, n, k, split=True, conv=not plain)
    info = f"{kind} m {M} n {n} k {k} flags {flags} cfg {cfg if cfg is not None else 'production: ' + picked}"
    if cfg is None:
        assert want_cfg is not None, "a production-dispatched case names the tile it was written for"
        assert want_cfg in picked, f"the dispatcher picks {picked!r} for this shape, the case was written for {want_cfg!r}"
    return Run(launch, outs, value, info, [flag] if flag is not None else [], zero_page)


def _g(entry, name, cap=64 << 20, **kw):
    CASES.append(Case(entry, name, (lambda ctx, _kw=kw: _gemm(ctx, **_kw)), cap))


SEG = (84, 64, 80, (0.7, 0.58, 0.82), (-2.6, -2.2, -1.9))
A, C_ = 1, 2          # WD_SPLIT_A, WD_SPLIT_C

# ---- fp32 MFMA kernel: rows {1, tile - 1, tile, tile + 1} of every production tile (conv_gemm.hip: pick_bn / use_small_tile), n ragged
#      inside the tile, a K tail in both K steps (16 / 32), c only 4-byte aligned (scalar stores); the tile is asserted
for _n, _tile, _bm in ((79, "64x80x32", 64), (127, "64x128x16", 64), (95, "128x96x16", 128), (63, "128x64x16", 128), (47, "128x48x16", 128)):
    for _m in (1, _bm - 1, _bm, _bm + 1):
        _g("wd_conv_gemm", f"{_tile} m{_m} n{_n} k100", m=_m, cin=100, n=_n, c_mis=4, ldc_x=3, lda_x=4, tol=TOL_GEMM_F32, want_cfg=_tile)
_g("wd_conv_gemm", "128x128x16 production (2064 tiles) m16385 n2048 k20", m=16385, cin=20, n=2048, tol=TOL_GEMM_F32,
   want_cfg="128x128x16")
_g("wd_conv_gemm", "gelu + residual into a channel slice, c 4-byte aligned", m=333, cin=128, n=64, ldc_x=136, c_mis=4, act=3, res="sep",
   tol=TOL_GEMM_F32_EPI, want_cfg="128x64x16")
_g("wd_conv_gemm", "residual in place", m=257, cin=512, n=128, res="inplace", tol=TOL_GEMM_F32_EPI, want_cfg="64x128x16")
_g("wd_conv_gemm", "similarity seg + sigmoid, n 81", m=3 * 84, cin=768, n=81, seg=SEG, sigmoid=True, bias=False, c_mis=4,
   tol=TOL_SIM_F32, want_cfg="128x96x16")
_g("wd_conv_gemm", "similarity seg + sigmoid, n 80", m=3 * 84, cin=768, n=80, seg=SEG, sigmoid=True, bias=False,
   tol=TOL_SIM_F32, want_cfg="64x80x32")
_g("wd_conv_gemm", "batch-stride rows", b=3, h=4, w=4, cin=64, n=96, cbs_x=5, tol=TOL_GEMM_F32, want_cfg="128x96x16")
_g("wd_conv_gemm", "3x3 s1 conv, lda > cin", b=2, h=9, w=7, cin=32, n=64, kh=3, pad=1, lda_x=8, tol=TOL_GEMM_F32_EPI, want_cfg="128x64x16")
_g("wd_conv_gemm", "3x3 s2 conv ragged map", b=2, h=7, w=9, cin=64, n=64, kh=3, stride=2, pad=1, tol=TOL_GEMM_F32_EPI, want_cfg="128x64x16")
_g("wd_conv_gemm", "2x2 s2 conv", b=2, h=8, w=8, cin=128, n=256, kh=2, stride=2, tol=TOL_GEMM_F32_EPI, want_cfg="64x128x16")
_g("wd_conv_gemm", "deconv 2x2 scatter into a third of the rows", b=2, h=5, w=6, cin=64, n=128, deconv=True, ldc_x=64,
   tol=TOL_GEMM_F32_EPI, want_cfg="64x128x16")
# the tiles scripts/gemm_bench.py runs through wd_conv_gemm_tuned that are (or were) production: 3 = 128x128, 9 = 128x64, 13 = 64x128, 25 = 64x80
for _cfg, _bm, _n in ((3, 128, 127), (9, 128, 63), (13, 64, 127), (25, 64, 79)):
    for _m in (1, _bm - 1, _bm, _bm + 1):
        _g("wd_conv_gemm_tuned", f"cfg{_cfg} m{_m} n{_n}", m=_m, cin=100, n=_n, cfg=_cfg, ldc_x=3, c_mis=4, tol=TOL_GEMM_F32)

# ---- fp16x3, fp32 activations split by the loader (flags 0): every tile, ragged everywhere (n = 331: ragged to 8 and to the tile:
#      the scalar store tail; w_split rows [331, 336) exist in the buffer and hold the surroundings' pattern)
for _cfg in (41, 50, 51, 52, 53, 55):
    _g("wd_conv_gemm_split", f"loader-split cfg{_cfg} m257 n331 k200 gelu", kind="split", cfg=_cfg, m=257, cin=200, n=331, act=3,
       ldc_x=3, lda_x=4, c_mis=4, tol=TOL_SPLIT)
for _cfg, _bm in ((41, 128), (50, 128), (51, 128), (52, 256), (53, 128), (55, 128)):
    for _m in (1, _bm - 1, _bm, _bm + 1):
        _g("wd_conv_gemm_split", f"loader-split cfg{_cfg} m{_m} n83 k40 residual", kind="split", cfg=_cfg, m=_m, cin=40, n=83,
           res="sep", ldc_x=1, c_mis=4, tol=TOL_SPLIT)
_g("wd_conv_gemm_split", "loader-split production m127 n75 k24 residual c 4-byte aligned", kind="split", m=127, cin=24, n=75,
   res="sep", c_mis=4, ldc_x=1, tol=TOL_SPLIT, want_cfg="128x128x32/4w")
_g("wd_conv_gemm_split", "loader-split 3x3 s2 silu", kind="split", b=2, h=18, w=22, cin=32, n=96, kh=3, stride=2, pad=1, act=2,
   lda_x=8, tol=TOL_SPLIT, want_cfg="128x128x32/4w")
_g("wd_conv_gemm_split", "loader-split deconv scatter", kind="split", b=2, h=5, w=7, cin=32, n=64, deconv=True, ldc_x=16,
   tol=TOL_SPLIT, want_cfg="128x64x16/2w")
_g("wd_conv_gemm_split", "loader-split seg + sigmoid batch-stride", kind="split", b=2, h=1, w=84, cin=768, n=80, seg=SEG,
   sigmoid=True, bias=False, cbs_x=3, tol=TOL_SIM_F32, want_cfg="128x128x32/4w")
_g("wd_conv_gemm_split", "C-only split (fp32 in, hi/lo out) into a channel slice", kind="split", flags=C_, m=1000, cin=512, n=128,
   ldc_x=256, act=1, tol=TOL_SPLIT, want_cfg="128x128x32/4w")

# ---- fp16x3, pre-split activations, plain layers: the register-staged tiles (50 / 51) and the direct-to-LDS families of
#      split_gemm_pre / p4 / p8, rows {1 (or one row group), tile - 1, tile, tile + 1} of every tile height
for _cfg, _bm in ((50, 128), (51, 128), (60, 128), (63, 256)):
    for _m in (1, _bm - 1, _bm, _bm + 1):
        _g("wd_conv_gemm_split", f"pre-split cfg{_cfg} m{_m} n136 k80 gelu -> hi/lo", kind="split", cfg=_cfg, flags=A | C_, m=_m,
           cin=80, n=136, act=3, lda_x=8, ldc_x=8, tol=TOL_SPLIT)
        _g("wd_conv_gemm_split", f"pre-split cfg{_cfg} m{_m} n136 k80 residual", kind="split", cfg=_cfg, flags=A, m=_m, cin=80,
           n=136, res="sep", lda_x=8, ldc_x=4, tol=TOL_SPLIT)
    for _n in (81, 83):                                           # n ragged to 8: the scalar store tail, w_split rows [n, n8) present
        _g("wd_conv_gemm_split", f"pre-split cfg{_cfg} m{_bm + 1} n{_n} k80 residual, c 4-byte aligned", kind="split", cfg=_cfg, flags=A,
           m=_bm + 1, cin=80, n=_n, res="sep", lda_x=8, ldc_x=1, c_mis=4, res_x=1, tol=TOL_SPLIT)
_g("wd_conv_gemm_split", "pre-split cfg55 long K residual in place", kind="split", cfg=55, flags=A, m=130, cin=1024, n=128,
   res="inplace", tol=TOL_SPLIT)
for _m, _n, _k in ((8, 8, 32), (248, 264, 64), (256, 256, 64), (264, 320, 96)):     # 256 x 256 tiles: rows / columns in groups of 8
    _g("wd_conv_gemm_split", f"p8 cfg64 m{_m} n{_n} k{_k} gelu -> hi/lo", kind="split", cfg=64, flags=A | C_, m=_m, cin=_k, n=_n,
       act=3, lda_x=8, ldc_x=8, tol=TOL_SPLIT)
    _g("wd_conv_gemm_split", f"p8 cfg64 m{_m} n{_n} k{_k} residual", kind="split", cfg=64, flags=A, m=_m, cin=_k, n=_n, res="sep",
       lda_x=8, ldc_x=4, tol=TOL_SPLIT)
for _m, _n, _k in ((16, 16, 96), (112, 272, 16), (128, 256, 32), (144, 272, 48)):   # 128 x 256 tiles: rows / columns in groups of 16
    _g("wd_conv_gemm_split", f"p4 cfg66 m{_m} n{_n} k{_k} gelu -> hi/lo", kind="split", cfg=66, flags=A | C_, m=_m, cin=_k, n=_n,
       act=3, lda_x=8, ldc_x=8, tol=TOL_SPLIT)
    _g("wd_conv_gemm_split", f"p4 cfg66 m{_m} n{_n} k{_k} residual in place", kind="split", cfg=66, flags=A, m=_m, cin=_k, n=_n,
       res="inplace", lda_x=8, tol=TOL_SPLIT)
_g("wd_conv_gemm_split", "pre-split production m1000 n128 k128 gelu -> hi/lo", kind="split", flags=A | C_, m=1000, cin=128, n=128, act=3,
   tol=TOL_SPLIT, want_cfg="128x128x16/4w/glds")
_g("wd_conv_gemm_split", "pre-split production m2048 n4096 k256 residual (p8 tile form)", kind="split", flags=A, m=2048, cin=256, n=4096,
   res="sep", tol=TOL_SPLIT, want_cfg="256x256x32/8w/p8")
_g("wd_conv_gemm_split", "LayerNorm fold cfg60 m129 n256 k64", kind="split", cfg=60, flags=A | C_, m=129, cin=64, n=256, act=3, ln=True,
   tol=TOL_SPLIT)
_g("wd_conv_gemm_split", "LayerNorm fold cfg64 m264 n256 k64", kind="split", cfg=64, flags=A | C_, m=264, cin=64, n=256, act=3, ln=True,
   tol=TOL_SPLIT)
# the persistent 256 x 256 kernel: one column tile, and the gang shapes of tests/test_gpu_split.py:511-513 (three / four column tiles:
# gangs of 1 and of 4; tiles cut between two CUs are parked in the workspace)
_g("wd_conv_gemm_split_ws", "persistent cfg65 m65544 n256 k96 residual", kind="split", cfg=65, flags=A, m=65536 + 8,
   cin=96, n=256, res="sep", res_x=0, ws="park", tol=TOL_SPLIT)
_g("wd_conv_gemm_split_ws", "persistent cfg65 m66000 n512 k32 gelu -> hi/lo", kind="split", cfg=65, flags=A | C_,
   m=66000, cin=32, n=512, act=3, ws="park", tol=TOL_SPLIT)
_g("wd_conv_gemm_split_ws", "persistent cfg65 gangs m40008 n1024 k64 gelu -> hi/lo", kind="split", cfg=65, flags=A | C_,
   m=40008, cin=64, n=1024, act=3, ws="park", tol=TOL_SPLIT)
_g("wd_conv_gemm_split_ws", "persistent cfg65 gangs m70000 n768 k96 residual", kind="split", cfg=65, flags=A,
   m=70000, cin=96, n=768, res="sep", res_x=0, ws="park", tol=TOL_SPLIT)
for _s in (2, 3, 7):
    _g("wd_conv_gemm_split_ws", f"forced split-K {_s} cfg51 m130 n72 k400", kind="split", cfg=51, m=130, cin=400, n=72, splits=_s,
       ws="splitk", ldc_x=4, lda_x=4, tol=TOL_SPLIT)
_g("wd_conv_gemm_split_ws", "forced split-K 3 pre-split cfg60 residual", kind="split", cfg=60, flags=A, m=130, cin=400, n=72, splits=3,
   ws="splitk", res="sep", lda_x=8, tol=TOL_SPLIT)
_g("wd_conv_gemm_split_ws", "library-chosen split-K, seg + sigmoid", kind="split", b=1, h=1, w=84, cin=768, n=80, seg=SEG,
   sigmoid=True, bias=False, ws="splitk", splits=0, tol=TOL_SIM_F32, want_cfg="128x128x32/4w")

# ---- fp16x3, pre-split activations through the implicit-GEMM LDS-DMA kernels (split_gemm_conv / conv3)
for _cfg in (70, 73, 74):
    _g("wd_conv_gemm_split", f"dma cfg{_cfg} 3x3 s2 relu -> hi/lo channel slice", kind="split", cfg=_cfg, flags=A | C_, b=2, h=13, w=17,
       cin=32, n=96, kh=3, stride=2, pad=1, act=1, lda_x=8, ldc_x=64, tol=TOL_SPLIT)
    _g("wd_conv_gemm_split", f"dma cfg{_cfg} 1x1 dual output + residual", kind="split", cfg=_cfg, flags=A | C_, b=2, h=12, w=20, cin=48,
       n=136, act=2, res="sep", c2=True, lda_x=8, tol=TOL_SPLIT)
_g("wd_conv_gemm_split", "dma production 2x2 s2 fp32 out", kind="split", flags=A, b=2, h=16, w=12, cin=64, n=128, kh=2, stride=2,
   lda_x=8, ldc_x=4, tol=TOL_SPLIT, want_cfg="256x128x16/8w/dma")
_g("wd_conv_gemm_split", "dma production 1x1 batch-stride rows, dual", kind="split", flags=A | C_, b=2, h=9, w=31, cin=256, n=40,
   cbs_x=7, c2=True, tol=TOL_SPLIT, want_cfg="256x64x16/8w/dma")
_g("wd_conv_gemm_split", "dma production deconv scatter -> hi/lo", kind="split", flags=A | C_, b=2, h=5, w=7, cin=64, n=128, deconv=True,
   ldc_x=64, tol=TOL_SPLIT, want_cfg="256x128x16/8w/dma")
for _cfg in (75, 77, 78, 79):
    _g("wd_conv_gemm_split", f"conv3 cfg{_cfg} ragged 13x17 silu + residual, dual", kind="split", cfg=_cfg, flags=A | C_, b=1, h=13, w=17,
       cin=32, n=96, kh=3, pad=1, act=2, res="sep", c2=True, lda_x=8, ldc_x=8, rel=REL_CONV3)
    _g("wd_conv_gemm_split", f"conv3 cfg{_cfg} 2x2 map", kind="split", cfg=_cfg, flags=A, b=1, h=2, w=2, cin=16, n=8, kh=3, pad=1,
       lda_x=8, ldc_x=4, rel=REL_CONV3)
_g("wd_conv_gemm_split", "conv3 production 19x23 c48 n136", kind="split", flags=A, b=2, h=19, w=23, cin=48, n=136, kh=3, pad=1,
   rel=REL_CONV3, want_cfg="256x64x16")
for _cfg in (77, 79):
    _g("wd_conv_gemm_split_ws", f"conv3 cfg{_cfg} forced split-K 2, dual", kind="split", cfg=_cfg, flags=A | C_, b=2, h=20, w=20, cin=256,
       n=64, kh=3, pad=1, act=2, res="sep", c2=True, splits=2, ws="splitk", rel=REL_CONV3)
_g("wd_conv_gemm_split_ws", "dma cfg70 forced split-K 2", kind="split", cfg=70, flags=A | C_, b=2, h=20, w=20, cin=64, n=64, kh=3, pad=1,
   act=2, c2=True, splits=2, ws="splitk", tol=TOL_SPLIT)


# ================================================================================================ fp16x3 weight split
@case("wd_split_weights", "n5 k48", n=5, k=48, padded=False)
@case("wd_split_weights", "n130 k24 (k padded to 32)", n=130, k=24, padded=False)
@case("wd_split_weights_padded", "n5 k48", n=5, k=48, padded=True)
@case("wd_split_weights_padded", "n130 k24", n=130, k=24, padded=True)
def _split_weights(ctx, n, k, padded):
    """wd_split_weights writes exactly n rows of k16 * 4 bytes; _padded writes all of wd_split_weights_bytes(n, k)."""
    L = ctx.L
    k16, n8 = (k + 15) // 16 * 16, (n + 7) // 8 * 8
    assert int(L.LIB.wd_split_weights_bytes(n, k)) == n8 * k16 * 4
    w = _rand(3, n, k, scale=0.05)
    wd = ctx.inp("w", w)
    out = ctx.out("out", (n8 if padded else n, k16))
    scale = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    fn = L.LIB.wd_split_weights_padded if padded else L.LIB.wd_split_weights

    def launch():
        L.check(fn(wd.data_ptr(), n, k, scale, out.data_ptr(), L.stream_ptr()), "wd_split_weights")

    def value(o):        # tests/test_gpu_split.py:19-38: the numpy restatement, bit for bit
        x = torch.zeros(out.shape[0], k16)
        x[:n, :k] = w * scale
        assert torch.equal(_bits(o["out"].cpu()), _bits(split_cpu(x)))
    return Run(launch, lambda: {"out": out}, value, f"n {n} k {k} padded {padded}", finite=False)


# ================================================================================================ fused block MLPs
def _mlp_ref(a_val, w1, b1, w2, b2, x0, ln=None):
    y = a_val @ w1.double().T
    if ln is not None:
        stats, u = ln
        y = stats[:, 1:2].double() * (y - stats[:, 0:1].double() * u.double()[None, :])
    return x0.double() + F.gelu(y + b1.double()) @ w2.double().T + b2.double()


def _dev_split_weights(L, w):
    ws, unscale = L.split_weights(w.cuda())
    return ws, unscale


@case("wd_mlp_fused_split", "rows 128", rows=128, c=128, kind="narrow")
@case("wd_mlp_fused_split", "rows 384 hid_scale 0.25", rows=384, c=128, kind="narrow", hid_scale=0.25)
@case("wd_mlp_fused_wide", "c256 rows 128", rows=128, c=256, kind="wide")
@case("wd_mlp_fused_wide", "c512 rows 384, workspace on offer", rows=384, c=512, kind="wide", park=True)
@case("wd_mlp_fused_wide", "c256 rows 128 x 257 persistent", rows=128 * 257, c=256, kind="wide", park=True, cap=256 << 20)
@case("wd_mlp_fused_wide_ln", "c256 rows 128", rows=128, c=256, kind="ln")
@case("wd_mlp_fused_wide_ln", "c256 rows 128 x 257 persistent", rows=128 * 257, c=256, kind="ln", park=True, cap=256 << 20)
def _mlp(ctx, rows, c, kind, hid_scale=1.0, park=False):
    L = ctx.L
    hdim = 4 * c
    d = _rand(11, rows, c, scale=2.0, shift=0.7 if kind == "ln" else 0.0)
    x0 = _rand(12, rows, c, scale=1.5)
    w1, b1 = _rand(13, hdim, c, scale=c ** -0.5), _rand(14, hdim, scale=0.1)
    w2, b2 = _rand(15, c, hdim, scale=hdim ** -0.5), _rand(16, c, scale=0.1)
    dsc = 4.0 if kind == "ln" else 1.0
    a_sp = split_cpu(d * dsc)
    a_val = unsplit(a_sp) / dsc
    ws1, ws2 = _dev_split_weights(L, w1), _dev_split_weights(L, w2)
    u1, u2 = ws1[1] / dsc, ws2[1] / hid_scale
    if kind == "narrow":
        p1, p2 = ws1[0], ws2[0]
    else:
        p1, p2 = L.mlp_wide_pack(ws1[0], hdim, c), L.mlp_wide_pack(ws2[0], c, hdim)
    a = ctx.inp("a_split", a_sp)
    w1d = ctx.ar.take("w1", p1.shape, u8, misalign=16, role="input", data=p1.cpu(), row_pitch=4 * c)
    w2d = ctx.ar.take("w2", p2.shape, u8, misalign=16, role="input", data=p2.cpu(), row_pitch=4 * hdim)
    b1d, b2d = ctx.inp("b1", b1), ctx.inp("b2", b2)
    x = ctx.inout("x", x0)
    x0d = x0.cuda()
    flag = ctx.flag()
    ln = None
    if kind == "ln":
        d64 = a_val
        stats = torch.stack([d64.mean(dim=1), 1.0 / torch.sqrt(d64.var(dim=1, unbiased=False) + 1e-6)], dim=1).float().contiguous()
        u = w1.double().sum(dim=1).float()
        ln = (stats, u)
        statsd, ud = ctx.inp("ln_stats", stats, mis=8), ctx.inp("u", u)
    wsb = zero_page = None
    if park:
        wsb = ctx.ws("workspace", L.p8_workspace_bytes(), zero_prefix=4096)
        zero_page = wsb[:4096]

    def launch():
        x.copy_(x0d)
        if kind == "narrow":
            L.mlp_fused(a, rows, c, hdim, (w1d, u1), b1d, (w2d, u2), b2d, x, hid_scale=hid_scale, range_flag=flag)
        elif kind == "wide":
            L.mlp_fused_wide(a, rows, c, hdim, (w1d, u1), b1d, (w2d, u2), b2d, x, hid_scale=hid_scale, range_flag=flag, workspace=wsb)
        else:
            L.mlp_fused_wide_ln(a, rows, c, hdim, (w1d, u1), b1d, ud, statsd, (w2d, u2), b2d, x, hid_scale=hid_scale, range_flag=flag,
                                workspace=wsb)

    def value(o):
        ref = _mlp_ref(a_val, w1, b1, w2, b2, x0, ln)
        assert_close(f"mlp {kind}", o["x"].cpu(), ref, REL_MLP * float(ref.abs().max()))
    return Run(launch, lambda: {"x": x}, value, f"{kind} rows {rows} c {c} park {park}", [flag], zero_page)


# ================================================================================================ elementwise.hip
def _dw_ref(x, w7, bias, b, h, w, c):
    r = F.conv2d(x.double().view(b, h, w, c).permute(0, 3, 1, 2), w7.double().T.reshape(c, 1, 7, 7), bias.double(), padding=3, groups=c)
    return r.permute(0, 2, 3, 1).reshape(b * h * w, c)


DW_MAPS = {0: [(36, 5, 3), (32, 17, 20), (64, 20, 33)], 1: [(36, 5, 3), (32, 17, 9)], 2: [(32, 5, 3), (32, 17, 20), (64, 20, 33)],
           3: [(32, 16, 17), (32, 32, 5)], 4: [(32, 5, 3), (32, 17, 20), (64, 20, 33), (96, 9, 11)]}
for _v, _maps in DW_MAPS.items():
    for _c, _h, _w in _maps:
        @case("wd_dwconv7" if _v == 0 else "wd_dwconv7_variant", f"form {_v} c{_c} {_h}x{_w}", variant=_v, c=_c, h=_h, w=_w)
        def _dwconv(ctx, variant, c, h, w, b=2):
            L = ctx.L
            x, w7, bias = _rand(21, b * h * w, c), _rand(22, 49, c, scale=1 / 7), _rand(23, c)
            xd, wd, bd = ctx.inp("x", x), ctx.inp("w7", w7), ctx.inp("bias", bias)
            y = ctx.out("y", (b * h * w, c))
            return Run(lambda: L.dwconv7(xd, wd, bd, y, b, h, w, c, variant=variant), lambda: {"y": y},
                       lambda o: assert_close("dwconv7", o["y"].cpu(), _dw_ref(x, w7, bias, b, h, w, c), *TOL_DW),
                       f"form {variant} c {c} map {h}x{w}")

for _c, _h, _w in ((64, 17, 5), (128, 9, 33), (192, 17, 9), (256, 9, 7), (256, 13, 21), (384, 11, 19), (512, 5, 17)):
    for _split in (False, True):
        @case("wd_dwconv7_ln", f"c{_c} {_h}x{_w} split {_split}", c=_c, h=_h, w=_w, split=_split)
        def _dwconv_ln(ctx, c, h, w, split, b=2):
            """Value: bit-identical to wd_dwconv7 followed by wd_layernorm_rows(_split) (tests/test_gpu_kernels.py:625)."""
            L = ctx.L
            rows = b * h * w
            x, w7, bias = _rand(24, rows, c, scale=2.0), _rand(25, 49, c, scale=0.15), _rand(26, c, scale=0.1)
            gam, bet = torch.rand(c, generator=torch.Generator().manual_seed(27)) + 0.5, _rand(28, c, scale=0.1)
            xd, wd, bd, gd, btd = ctx.inp("x", x), ctx.inp("w7", w7), ctx.inp("bias", bias), ctx.inp("gamma", gam), ctx.inp("beta", bet)
            y = ctx.out("y", (rows, c))

            def value(o):
                ref = torch.empty(rows, c, device="cuda")
                L.dwconv7(x.cuda(), w7.cuda(), bias.cuda(), ref, b, h, w, c)
                L.layernorm_rows(ref, ref, gam.cuda(), bet.cuda(), rows, c, split=split)
                torch.cuda.synchronize()
                assert torch.equal(_bits(o["y"]), _bits(ref)), "differs from dwconv7 + layernorm_rows"
            return Run(lambda: L.dwconv7_ln(xd, wd, bd, y, gd, btd, b, h, w, c, split=split), lambda: {"y": y}, value,
                       f"c {c} map {h}x{w} split {split}")

for _c, _h, _w in ((64, 9, 7), (256, 13, 21), (512, 5, 17)):
    @case("wd_dwconv7_stats", f"c{_c} {_h}x{_w}", c=_c, h=_h, w=_w)
    def _dw_stats(ctx, c, h, w, b=2, scale=4.0):
        L = ctx.L
        rows = b * h * w
        x, w7, bias = _rand(31, rows, c, scale=2.0, shift=0.7), _rand(32, 49, c, scale=0.15), _rand(33, c, scale=0.1)
        xd, wd, bd = ctx.inp("x", x), ctx.inp("w7", w7), ctx.inp("bias", bias)
        ys, part = ctx.out("y_split", (rows, c)), ctx.out("part", (c // 32, rows, 2))

        def value(o):
            ref = _dw_ref(x, w7, bias, b, h, w, c)
            assert_close("dwconv7_stats y", unsplit(o["y_split"].cpu()) / scale, ref, *TOL_DW)
        return Run(lambda: L.dwconv7_stats(xd, wd, bd, ys, part, b, h, w, c, scale=scale), lambda: {"y_split": ys, "part": part}, value,
                   f"c {c} map {h}x{w}")

    @case("wd_ln_stats_finalize", f"c{_c} rows {2 * _h * _w}", c=_c, h=_h, w=_w)
    def _ln_finalize(ctx, c, h, w, b=2):
        L = ctx.L
        rows = b * h * w
        x, w7, bias = _rand(31, rows, c, scale=2.0, shift=0.7), _rand(32, 49, c, scale=0.15), _rand(33, c, scale=0.1)
        d, ds = torch.empty(rows, c, device="cuda"), torch.empty(rows, c, device="cuda")
        part = torch.empty(c // 32, rows, 2, device="cuda")
        L.dwconv7(x.cuda(), w7.cuda(), bias.cuda(), d, b, h, w, c)
        L.dwconv7_stats(x.cuda(), w7.cuda(), bias.cuda(), ds, part, b, h, w, c)
        torch.cuda.synchronize()
        pd = ctx.inp("part", part.cpu())
        stats = ctx.out("stats", (rows, 2), mis=8)

        def value(o):
            d64 = d.double().cpu()
            assert_close("row mean", o["stats"][:, 0].cpu(), d64.mean(dim=1), *TOL_STATS_MEAN)
            assert_close("row rstd", o["stats"][:, 1].cpu(), 1.0 / torch.sqrt(d64.var(dim=1, unbiased=False) + 1e-6), *TOL_STATS_RSTD)
        return Run(lambda: L.ln_stats_finalize(pd, stats, rows, c), lambda: {"stats": stats}, value, f"c {c} rows {rows}")


def _stem_inputs(c0, b, h, w):
    g = torch.Generator().manual_seed(41)
    img = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.int64).to(u8)
    return img, _rand(42, c0, 48, scale=0.3), _rand(43, c0, scale=0.1), _rand(44, c0, scale=0.2, shift=1.0), _rand(45, c0, scale=0.1)


for _c0, _b, _h, _w in ((64, 1, 8, 12), (96, 1, 36, 44), (128, 2, 20, 28), (192, 3, 20, 28), (128, 1, 4, 4)):
    @case("wd_stem_fused", f"c0 {_c0} {_b}x{_h}x{_w}", c0=_c0, b=_b, h=_h, w=_w)
    def _stem_fused(ctx, c0, b, h, w):
        L = ctx.L
        img, wt, bias, g, bt = _stem_inputs(c0, b, h, w)
        m = b * (h // 4) * (w // 4)
        imgd = ctx.inp("img", img, mis=4)
        wd, bd, gd, btd = ctx.inp("wgt", wt), ctx.inp("bias", bias), ctx.inp("gamma", g), ctx.inp("beta", bt)
        out = ctx.out("out", (m, c0))

        def value(o):
            x = (img.double() / 255.0).view(b, h // 4, 4, w // 4, 4, 3).permute(0, 1, 3, 2, 4, 5).reshape(m, 48)
            ref = F.layer_norm(x @ wt.double().T + bias.double(), (c0,), g.double(), bt.double(), 1e-6)
            assert_close(f"stem c0={c0}", o["out"].cpu(), ref, *TOL_STEM)
        return Run(lambda: L.stem_fused(imgd, wd, bd, gd, btd, out), lambda: {"out": out}, value, f"c0 {c0} rows {m}")

for _b, _h, _w in ((1, 4, 4), (2, 32, 24), (1, 36, 44)):
    @case("wd_stem_patchify", f"{_b}x{_h}x{_w}", b=_b, h=_h, w=_w)
    def _stem_patchify(ctx, b, h, w):
        L = ctx.L
        img = _stem_inputs(64, b, h, w)[0]
        m = b * (h // 4) * (w // 4)
        imgd = ctx.inp("img", img, mis=4)
        out = ctx.out("out", (m, 48))

        def value(o):         # tests/test_gpu_kernels.py:143: bit-exact
            ref = (img.float() / 255.0).view(b, h // 4, 4, w // 4, 4, 3).permute(0, 1, 3, 2, 4, 5).reshape(m, 48)
            assert torch.equal(o["out"].cpu(), ref)
        return Run(lambda: L.stem_patchify(imgd, out), lambda: {"out": out}, value, f"rows {m}")


def _ln_inputs(rows, c):
    return _rand(51, rows, c, scale=2.0, shift=0.5), _rand(52, c, scale=0.2, shift=1.0), _rand(53, c, scale=0.1)


for _c in (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048):
    for _split in (False, True):
        @case("wd_layernorm_rows_split" if _split else "wd_layernorm_rows", f"c{_c} rows 77 ldx+4 ldy+8", c=_c, split=_split)
        def _layernorm(ctx, c, split, rows=77):
            L = ctx.L
            x, g, b = _ln_inputs(rows, c)
            xd, gd, bd = ctx.inp("x", x, ld=c + 4), ctx.inp("gamma", g), ctx.inp("beta", b)
            y = ctx.out("y", (rows, c), ld=c + 8)

            def value(o):
                ref = F.layer_norm(x.double(), (c,), g.double(), b.double(), 1e-6)
                got = unsplit(o["y"].cpu()) if split else o["y"].cpu().double()
                assert_close(f"layernorm c{c}", got, ref, *TOL_LN)
            return Run(lambda: L.layernorm_rows(xd, y, gd, bd, rows, c, ldx=c + 4, ldy=c + 8, split=split), lambda: {"y": y}, value,
                       f"c {c} split {split}")


@case("wd_layernorm_rows", "in place, one row, ld > c", c=96, split=False)
@case("wd_layernorm_rows_split", "in place, one row, ld > c", c=96, split=True)
def _layernorm_inplace(ctx, c, split, rows=1):
    L = ctx.L
    x, g, b = _ln_inputs(rows, c)
    xd, gd, bd = ctx.inout("x", x, ld=c + 8), ctx.inp("gamma", g), ctx.inp("beta", b)
    x0 = x.cuda()

    def launch():
        xd.copy_(x0)
        L.layernorm_rows(xd, xd, gd, bd, rows, c, ldx=c + 8, ldy=c + 8, split=split)

    def value(o):
        ref = F.layer_norm(x.double(), (c,), g.double(), b.double(), 1e-6)
        assert_close("layernorm in place", unsplit(o["x"].cpu()) if split else o["x"].cpu().double(), ref, *TOL_LN)
    return Run(launch, lambda: {"x": xd}, value, f"c {c} split {split} in place")


for _b, _h, _w, _c in ((1, 2, 2, 256), (2, 6, 10, 64), (1, 4, 6, 128), (3, 2, 34, 32), (1, 6, 2, 1024)):
    @case("wd_layernorm_rows_split_s2d", f"{_b}x{_h}x{_w} c{_c}", b=_b, h=_h, w=_w, c=_c)
    def _layernorm_s2d(ctx, b, h, w, c):
        L = ctx.L
        x, g, bt = _ln_inputs(b * h * w, c)
        xd, gd, bd = ctx.inp("x", x), ctx.inp("gamma", g), ctx.inp("beta", bt)
        y = ctx.out("y", (b * (h // 2) * (w // 2), 4 * c))

        def value(o):
            ref = F.layer_norm(x.double(), (c,), g.double(), bt.double(), 1e-6).view(b, h // 2, 2, w // 2, 2, c)
            ref = ref.permute(0, 1, 3, 2, 4, 5).reshape(b * (h // 2) * (w // 2), 4 * c)
            assert_close("layernorm s2d", unsplit(o["y"].cpu()), ref, *TOL_LN)
        return Run(lambda: L.layernorm_rows_split_s2d(xd, y, gd, bd, b, h, w, c), lambda: {"y": y}, value, f"c {c} map {h}x{w}")


@case("wd_l2norm_rows", "81 x 768", rows=81, c=768)
@case("wd_l2norm_rows", "1 x 64", rows=1, c=64)
@case("wd_l2norm_rows", "7 x 100", rows=7, c=100)
def _l2norm(ctx, rows, c):
    L = ctx.L
    x = _rand(61, rows, c, scale=3.0)
    xd = ctx.inp("x", x)
    y = ctx.out("y", (rows, c))
    return Run(lambda: L.l2norm_rows(xd, y), lambda: {"y": y},
               lambda o: assert_close("l2norm", o["y"].cpu(), F.normalize(x.double(), dim=-1), *TOL_L2), f"rows {rows} c {c}")


@case("wd_dfl_decode", "level 8x6 into the middle of 2 x 70 anchors, ld 72", hl=8, wl=6, off=10, ntot=70, ld=72)
@case("wd_dfl_decode", "level 1x1 last anchor", hl=1, wl=1, off=69, ntot=70, ld=64)
def _dfl(ctx, hl, wl, off, ntot, ld, b=2, stride=16):
    """boxes is the [b, ntot, 4] anchor tensor; the level writes rows [off, off + hl * wl) of every image only."""
    L = ctx.L
    d = _rand(71, b, hl * wl, 64, scale=2.0)
    dd = ctx.inp("dist", d, ld=ld)
    boxes = ctx.out("boxes", (b, hl * wl, 4), bs=ntot)
    base = boxes.data_ptr() - off * 16

    def launch():
        L.check(L.LIB.wd_dfl_decode(dd.data_ptr(), ld, base, b, hl, wl, stride, off, ntot, L.stream_ptr()), "wd_dfl_decode")

    def value(o):             # tests/test_gpu_kernels.py:251-257
        e = d.double().view(b, hl * wl, 4, 16).softmax(3).matmul(torch.arange(16.0, dtype=f64).view(-1, 1)).squeeze(-1) * stride
        ys, xs = torch.meshgrid(torch.arange(hl, dtype=f64), torch.arange(wl, dtype=f64), indexing="ij")
        px, py = ((xs + 0.5) * stride).reshape(-1)[None], ((ys + 0.5) * stride).reshape(-1)[None]
        ref = torch.stack([px - e[..., 0], py - e[..., 1], px + e[..., 2], py + e[..., 3]], -1)
        assert_close("dfl decode", o["boxes"].cpu(), ref, *TOL_DFL)
    return Run(launch, lambda: {"boxes": boxes}, value, f"level {hl}x{wl} at anchor {off} of {ntot}")


# ================================================================================================ postprocess.hip
def _topk_scores(kind, n_a=700, k=9):
    g = np.random.default_rng(31)
    a = g.random((n_a, k), dtype=np.float32)
    ties = (np.round(g.random((n_a, k), dtype=np.float32) * 16) / 16).astype(np.float32)
    low = (g.random((n_a, k), dtype=np.float32) * 1e-4).astype(np.float32)
    return [a, ties, low]


@case("wd_topk_candidates", "count 0 (nothing above the threshold)", thr=2.0, nms_pre=100)
@case("wd_topk_candidates", "exactly the capacity kept", thr=0.001, nms_pre=1024)
@case("wd_topk_candidates", "beyond the capacity: truncated at nms_pre 1000", thr=0.001, nms_pre=1000)
@case("wd_topk_candidates", "everything kept, capacity 32768", thr=0.001, nms_pre=30000)
def _topk(ctx, thr, nms_pre):
    L = ctx.L
    sl = _topk_scores(0)
    b, n, k = len(sl), sl[0].size, sl[0].shape[1]
    s = ctx.inp("scores", torch.from_numpy(np.stack([x.reshape(-1) for x in sl])))
    cap = L.topk_capacity(nms_pre)
    idx = ctx.out("out_idx", (b, cap), i32, mis=4, fillers=(-1,))
    sc = ctx.out("out_score", (b, cap), mis=4)
    cnt = ctx.out("out_count", (b,), i32, mis=4, fillers=(-1,))
    ws = ctx.ws("workspace", L.topk_workspace_bytes(b, n, nms_pre), mis=0)

    def value(o):             # tests/test_gpu_kernels.py:277-290 check_topk
        from oracle import postprocess as opp
        gi, gs, gc = o["out_idx"].cpu().numpy(), o["out_score"].cpu().numpy(), o["out_count"].cpu().numpy()
        for i, x in enumerate(sl):
            rs, rl, ra = opp.filter_scores_and_topk(x, thr, nms_pre)
            m = rs.shape[0]
            assert gc[i] == m, f"image {i}: count {gc[i]} vs oracle {m}"
            assert np.array_equal(gi[i, :m], ra * k + rl) and np.array_equal(gs[i, :m], rs)
            assert np.all(gi[i, m:] == -1)
    return Run(lambda: L.topk_candidates(s, b, n, np.float32(thr), nms_pre, idx, sc, cnt, ws),
               lambda: {"out_idx": idx, "out_score": sc, "out_count": cnt}, value, f"thr {thr} nms_pre {nms_pre} capacity {cap}")


@case("wd_nms_gather", "vanilla, more survivors than max_out, embeddings gathered", mode="vanilla", max_out=300)
@case("wd_nms_gather", "mmcv offsets (workspace), max_out 7", mode="mmcv", max_out=7)
@case("wd_nms_gather", "torchvision trick (workspace), everything fits", mode="torchvision", max_out=1024)
def _nms(ctx, mode, max_out, n=900, k=3, dim=32):
    L = ctx.L
    from oracle import postprocess as opp
    g = np.random.default_rng(33)
    ctr = g.random((n, 2), dtype=np.float32) * 300 + 20
    wh = g.random((n, 2), dtype=np.float32) * 80 + 2
    bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    sc = np.sort(g.random(n, dtype=np.float32))[::-1].copy()
    lb = g.integers(0, k, n).astype(np.int64)
    emb = g.standard_normal((2, n, dim)).astype(np.float32)
    counts = np.asarray([n, 0], np.int32)                           # the second image has no candidate
    cidx = np.full((2, n), -1, np.int32)
    cidx[0] = np.arange(n) * k + lb
    csc = np.zeros((2, n), np.float32)
    csc[0] = sc
    boxes = np.zeros((2, n, 4), np.float32)
    boxes[0] = bx
    meta = np.asarray([[0, 0, 0, 1, 1, 1e9, 1e9, 0]] * 2, np.float32)
    code = {"vanilla": L.NMS_VANILLA, "torchvision": L.NMS_TORCHVISION, "mmcv": L.NMS_MMCV}[mode]
    param = {"vanilla": 0, "torchvision": 4000, "mmcv": 10000}[mode]
    t = lambda a: torch.from_numpy(a)
    ci, cs, cc = ctx.inp("cand_idx", t(cidx), mis=4), ctx.inp("cand_score", t(csc), mis=4), ctx.inp("cand_count", t(counts), mis=4)
    bd, md, ed = ctx.inp("boxes", t(boxes)), ctx.inp("meta", t(meta), mis=4), ctx.inp("embed", t(emb))
    ob, os_ = ctx.out("out_boxes", (2, max_out, 4)), ctx.out("out_scores", (2, max_out), mis=4)
    ol = ctx.out("out_labels", (2, max_out), i32, mis=4, fillers=(-1,))
    oa = ctx.out("out_anchors", (2, max_out), i32, mis=4, fillers=(-1,))
    oc = ctx.out("out_count", (2,), i32, mis=4, fillers=(-1,))
    oe = ctx.out("out_embed", (2, max_out, dim))
    ws = None if mode == "vanilla" else ctx.ws("workspace", L.nms_workspace_bytes(2), mis=4)

    def launch():
        L.nms_gather(ci, cs, cc, n, bd, n, k, md, L.nms_threshold(0.7, code), max_out, ed, dim, ob, os_, ol, oa, oc, oe, 2,
                     nms_mode=code, mode_param=param, workspace=None if ws is None else ws)

    def value(o):             # tests/test_gpu_kernels.py:416-423 _check_forms
        keep = {"vanilla": lambda: opp.batched_nms(bx, sc, lb, 0.7, max_keep=max_out),
                "torchvision": lambda: opp.torchvision_batched_nms(bx, sc, lb, 0.7, "cpu", max_keep=max_out),
                "mmcv": lambda: opp.mmcv_batched_nms(bx, sc, lb, dict(type="nms", iou_threshold=0.7, split_thr=param), max_keep=max_out)}[mode]()
        c, a = o["out_count"].cpu().numpy(), o["out_anchors"].cpu().numpy()
        assert c.tolist() == [keep.shape[0], 0]
        assert np.array_equal(a[0, :c[0]], keep) and np.all(a[0, c[0]:] == -1) and np.all(a[1] == -1)
        assert np.array_equal(o["out_labels"].cpu().numpy()[0, :c[0]], lb[keep]) and np.array_equal(o["out_scores"].cpu().numpy()[0, :c[0]], sc[keep])
        assert np.array_equal(o["out_embed"].cpu().numpy()[0, :c[0]], emb[0, keep]) and not o["out_embed"].cpu().numpy()[0, c[0]:].any()
    return Run(launch, lambda: dict(out_boxes=ob, out_scores=os_, out_labels=ol, out_anchors=oa, out_count=oc, out_embed=oe), value,
               f"{mode} max_out {max_out}")


# ================================================================================================ retrieval / similarity
def _retr_inputs(n_img, rows, k, dim):
    e = _rand(81, n_img, rows, dim, scale=1.4 * (768 / dim) ** 0.5)
    t = F.normalize(_rand(82, k, dim), dim=-1)
    scale, bias = _rand(83, n_img, rows, scale=0.1, shift=-0.35), _rand(84, n_img, rows, scale=0.2, shift=-2.6)
    cnt = torch.randint(0, rows + 1, (n_img,), generator=torch.Generator().manual_seed(85), dtype=i32)
    cnt[0] = rows
    if n_img > 2:
        cnt[1], cnt[2] = 0, 1
    return e, t, scale, bias, cnt


def _retr_ref(e, t, scale, bias, cnt):
    lg = torch.einsum("nrd,kd->nrk", e.double(), t.double()) * scale.double().exp()[..., None] + bias.double()[..., None]
    valid = torch.arange(e.shape[1])[None, :] < cnt[:, None]
    return torch.where(valid[..., None], torch.sigmoid(lg), torch.zeros((), dtype=f64)).amax(dim=1)


@case("wd_retrieval_max", "3 x 300 rows, 81 classes", n_img=3, rows=300, k=81, dim=768)
@case("wd_retrieval_max", "4 x 7 rows, 7 classes, dim 36", n_img=4, rows=7, k=7, dim=36)
def _retrieval(ctx, n_img, rows, k, dim):
    L = ctx.L
    e, t, scale, bias, cnt = _retr_inputs(n_img, rows, k, dim)
    ed, td, sd, bd, cd = ctx.inp("e", e), ctx.inp("t", t), ctx.inp("scale", scale, mis=4), ctx.inp("bias", bias, mis=4), ctx.inp("count", cnt, mis=4)
    out = ctx.out("out", (n_img, k), mis=4)
    return Run(lambda: L.retrieval_max(ed, td, sd, bd, cd, out, n_img, rows, k, dim), lambda: {"out": out},
               lambda o: assert_close("retrieval_max", o["out"].cpu(), _retr_ref(e, t, scale, bias, cnt), *TOL_RETR), f"{n_img} x {rows} x {k}")


def _padded_split(ctx, name, x, scale):
    """fp32 rows -> an arena buffer of wd_split_weights_bytes() written by wd_split_weights_padded (zero rows up to 8)."""
    L = ctx.L
    r, k = x.shape
    buf = ctx.ar.take(name, (int(L.LIB.wd_split_weights_bytes(r, k)),), u8, misalign=16, role="input", row_pitch=(k + 15) // 16 * 64)
    xd = x.contiguous().cuda()
    L.check(L.LIB.wd_split_weights_padded(xd.data_ptr(), r, k, float(scale), buf.data_ptr(), L.stream_ptr()), "wd_split_weights_padded")
    torch.cuda.synchronize()
    return buf


@case("wd_retrieval_max_split", "256-tile kernel: 7 x 20 rows, 515 classes, dim 64", n_img=7, rows=20, k=515, dim=64)
@case("wd_retrieval_max_split", "256-tile kernel: 2 x 301 rows, 81 classes", n_img=2, rows=301, k=81, dim=768)
@case("wd_retrieval_max_split", "ping-pong kernel (dim % 32 != 0): 33 x 7 rows, 264 classes, dim 48", n_img=33, rows=7, k=264, dim=48)
@case("wd_retrieval_max_split", "one class", n_img=1, rows=300, k=1, dim=768)
def _retrieval_split(ctx, n_img, rows, k, dim):
    L = ctx.L
    e, t, scale, bias, cnt = _retr_inputs(n_img, rows, k, dim)
    tsc = 2.0 ** (13 - math.floor(math.log2(float(t.abs().max()))))
    es, ts = _padded_split(ctx, "e_split", e.reshape(-1, dim), 1.0), _padded_split(ctx, "t_split", t, tsc)
    sd, bd, cd = ctx.inp("scale", scale), ctx.inp("bias", bias), ctx.inp("count", cnt, mis=4)
    out = ctx.out("out", (n_img, k), mis=4)
    flag = ctx.flag()

    def launch():
        L.check(L.LIB.wd_retrieval_max_split(es.data_ptr(), ts.data_ptr(), 1.0 / tsc, sd.data_ptr(), bd.data_ptr(), cd.data_ptr(),
                                             out.data_ptr(), n_img, rows, k, dim, flag.data_ptr(), L.stream_ptr()), "wd_retrieval_max_split")
    return Run(launch, lambda: {"out": out},
               lambda o: assert_close("retrieval_max_split", o["out"].cpu(), _retr_ref(e, t, scale, bias, cnt), *TOL_RETR_SPLIT),
               f"{n_img} x {rows} x {k} dim {dim}", [flag])


@case("wd_similarity_split", "2 x 85 rows (buffer padded to 176), 7 classes, ldo 9", b=2, ntot=85, ends=(64, 80), k=7, ldo=9)
@case("wd_similarity_split", "3 x 84 rows, 83 classes, ldo 83", b=3, ntot=84, ends=(64, 80), k=83, ldo=83)
@case("wd_similarity_split", "1 x 525 rows, 264 classes, ldo 272", b=1, ntot=525, ends=(400, 500), k=264, ldo=272)
def _sim_split(ctx, b, ntot, ends, k, ldo, dim=768, es_scale=4.0):
    """e_split: the BUFFER holds a multiple of eight rows; what the rows behind the last one hold is not the caller's business
    (a WD_SPLIT_C producer never writes them), so they keep the surroundings' pattern."""
    L = ctx.L
    rows = b * ntot
    rows8 = (rows + 7) // 8 * 8
    e, t = _rand(91, rows, dim, scale=0.8), F.normalize(_rand(92, k, dim), dim=-1)
    es_val = split_cpu(e * es_scale)
    es = ctx.ar.take("e_split", (rows8, dim), f32, misalign=16, role="input")
    es[:rows].copy_(es_val.cuda())
    tsc = 2.0 ** (13 - math.floor(math.log2(float(t.abs().max()))))
    ts = _padded_split(ctx, "t_split", t, tsc)
    out = ctx.out("out", (rows, k), ld=ldo, mis=4)
    flag = ctx.flag()
    seg = (ntot, ends[0], ends[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))

    def value(o):
        lvl = torch.arange(rows) % ntot
        lvl = (lvl >= ends[0]).long() + (lvl >= ends[1]).long()
        ref = (unsplit(es_val) / es_scale) @ t.double().T * torch.tensor(seg[3], dtype=f64)[lvl][:, None] + torch.tensor(seg[4], dtype=f64)[lvl][:, None]
        assert_close("similarity_split", o["out"].cpu(), torch.sigmoid(ref), *TOL_SIM_SPLIT)
    return Run(lambda: L.similarity_split(es, rows, ts, (1.0 / tsc) / es_scale, out, k, dim, ldo, seg=seg, sigmoid=True, range_flag=flag),
               lambda: {"out": out}, value, f"rows {rows} classes {k} ldo {ldo}", [flag])


@case("wd_similarity_grouped", "ragged counts, ldo 83, out 4-byte aligned", b=2, ntot=84, ends=(64, 80), k_max=80, ldo=83, counts=[80, 37])
@case("wd_similarity_grouped", "a column tile no image reaches, one empty image", b=3, ntot=40, ends=(32, 38), k_max=96, ldo=96, counts=[12, 0, 80])
@case("wd_similarity_grouped", "count NULL, k_max 7", b=2, ntot=84, ends=(64, 80), k_max=7, ldo=7, counts=None)
def _sim_grouped(ctx, b, ntot, ends, k_max, ldo, counts, dim=768):
    """Rows of a bank at or above count[b] are never read: they hold the surroundings' pattern here."""
    L = ctx.L
    e, t = _rand(301, b, ntot, dim, scale=0.8), F.normalize(_rand(302, b, k_max, dim), dim=-1)
    ed, td = ctx.inp("embed", e), ctx.ar.take("bank", (b, k_max, dim), f32, misalign=16, role="input")
    for i in range(b):
        c = k_max if counts is None else counts[i]
        td[i, :c].copy_(t[i, :c].cuda())
    cd = None if counts is None else ctx.inp("count", torch.tensor(counts, dtype=i32), mis=4)
    out = ctx.out("out", (b, ntot, k_max), ld=ldo, mis=4)
    seg = (ntot, ends[0], ends[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))

    def value(o):             # tests/test_gpu_per_image_bank.py:53-65
        pos = torch.arange(ntot)
        lvl = (pos >= ends[0]).long() + (pos >= ends[1]).long()
        ref = torch.einsum("bnc,bkc->bnk", e.double(), t.double()) * torch.tensor(seg[3], dtype=f64)[lvl][None, :, None] \
            + torch.tensor(seg[4], dtype=f64)[lvl][None, :, None]
        got = o["out"].cpu()
        for i in range(b):
            c = k_max if counts is None else counts[i]
            pad = got[i, :, c:]
            assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), f"image {i}: padding is not +0"
            assert_close(f"similarity_grouped image {i}", got[i, :, :c], torch.sigmoid(ref[i, :, :c]), *TOL_GROUPED)
    return Run(lambda: L.similarity_grouped(ed, td, cd, out, b, ntot, k_max, dim, ldo, seg, sigmoid=True), lambda: {"out": out}, value,
               f"{b} x {ntot} rows k_max {k_max} ldo {ldo} counts {counts}")


# ================================================================================================ text.hip / bricks.hip
@case("wd_text_embed", "37 tokens dim 768", n_tok=37, dim=768)
@case("wd_text_embed", "1 token dim 100", n_tok=1, dim=100)
def _text_embed(ctx, n_tok, dim, vocab=50, npos=20):
    L = ctx.L
    g = torch.Generator().manual_seed(101)
    ids = torch.randint(0, vocab, (n_tok,), generator=g, dtype=i64).to(i32)
    pids = torch.randint(0, npos, (n_tok,), generator=g, dtype=i64).to(i32)
    ids[0], pids[0] = vocab - 1, npos - 1                            # the last rows of both tables
    word, pos, type0 = _rand(102, vocab, dim), _rand(103, npos, dim), _rand(104, dim)
    idd, pd = ctx.inp("ids", ids, mis=4), ctx.inp("pos_ids", pids, mis=4)
    wd, psd, td = ctx.inp("word", word), ctx.inp("pos", pos), ctx.inp("type0", type0)
    out = ctx.out("out", (n_tok, dim))
    return Run(lambda: L.text_embed(idd, pd, wd, psd, td, out), lambda: {"out": out},
               lambda o: assert_close("text_embed", o["out"].cpu(), word[ids.long()].double() + pos[pids.long()].double() + type0.double(), *TOL_TEXT),
               f"{n_tok} tokens dim {dim}")


@case("wd_attention_small", "seq_len 1", n=3, ln=1, heads=2, dh=16)
@case("wd_attention_small", "seq_len 64, one row with every key but the first masked", n=2, ln=64, heads=3, dh=32)
@case("wd_attention_small", "seq_len 13 head_dim 64, ld_qkv > 3 H dh", n=5, ln=13, heads=2, dh=64)
def _attention(ctx, n, ln, heads, dh):
    L = ctx.L
    hd = heads * dh
    qkv = _rand(111, n * ln, 3 * hd)
    g = torch.Generator().manual_seed(112)
    mask = (torch.rand(n, ln, generator=g) > 0.3).to(i32)
    mask[:, 0] = 1
    mask[0, 1:] = 0
    qd = ctx.inp("qkv", qkv, ld=3 * hd + 8)
    md = ctx.inp("mask", mask, mis=4)
    out = ctx.out("out", (n * ln, hd), ld=hd + 4)

    def launch():
        L.check(L.LIB.wd_attention_small(qd.data_ptr(), md.data_ptr(), out.data_ptr(), n, ln, heads, dh, 3 * hd + 8, hd + 4, L.stream_ptr()),
                "wd_attention_small")

    def value(o):             # tests/test_gpu_text.py:71-75
        q, k, v = [t.view(n, ln, heads, dh).permute(0, 2, 1, 3).double() for t in qkv.split(hd, dim=1)]
        s = (q @ k.transpose(-1, -2) / dh ** 0.5).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
        ref = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(n * ln, hd)
        assert_close("attention", o["out"].cpu(), ref, *TOL_ATTN)
    return Run(launch, lambda: {"out": out}, value, f"{n} x {ln} heads {heads} dh {dh}")


@case("wd_max_sigmoid_attn", "1203 guide rows, 128-wide heads (several LDS passes)", n_img=1, hw=35, n_guide=1203, heads=2, hc=128, ohc=32)
@case("wd_max_sigmoid_attn", "8-wide heads, ragged map, 3 guide rows", n_img=3, hw=85, n_guide=3, heads=8, hc=8, ohc=8)
@case("wd_max_sigmoid_attn", "32-wide heads, 80 guide rows, no head scale", n_img=2, hw=130, n_guide=80, heads=4, hc=32, ohc=32, scaled=False)
def _msa(ctx, n_img, hw, n_guide, heads, hc, ohc, scaled=True):
    L = ctx.L
    rows = n_img * hw
    embed, guide = _rand(121, rows, heads * hc), _rand(122, n_img, n_guide, heads * hc)
    hb, hs = _rand(123, heads, scale=0.2), _rand(124, heads, scale=0.2, shift=1.0)
    x0 = _rand(125, rows, heads * ohc)
    ed, gd, hbd = ctx.inp("embed", embed, ld=heads * hc + 4), ctx.inp("guide", guide), ctx.inp("head_bias", hb, mis=4)
    hsd = ctx.inp("head_scale", hs, mis=4) if scaled else None
    x = ctx.inout("x", x0, ld=heads * ohc + 8)
    x0d = x0.cuda()

    def launch():
        x.copy_(x0d)
        L.max_sigmoid_attn(ed, gd, hbd, hsd, x, n_img, hw, n_guide, heads, hc, ohc)

    def value(o):             # include/wedetect_hip.h, wd_max_sigmoid_attn
        e = embed.double().view(n_img, hw, heads, hc)
        gg = guide.double().view(n_img, n_guide, heads, hc)
        a = torch.einsum("bpmc,bnmc->bpmn", e, gg).amax(dim=-1) / hc ** 0.5 + hb.double()
        a = torch.sigmoid(a) * (hs.double() if scaled else 1.0)
        ref = (x0.double().view(n_img, hw, heads, ohc) * a[..., None]).reshape(rows, heads * ohc)
        assert_close("max_sigmoid_attn", o["x"].cpu(), ref, *TOL_BRICK)
    return Run(launch, lambda: {"x": x}, value, f"{n_img} x {hw} px, {n_guide} guides, heads {heads} x {hc}")


@case("wd_adaptive_maxpool_nhwc", "13x11 c64 pool 3", b=2, h=13, w=11, c=64, p=3)
@case("wd_adaptive_maxpool_nhwc", "2x2 c16 pool 3 (windows of one pixel)", b=2, h=2, w=2, c=16, p=3)
@case("wd_adaptive_maxpool_nhwc", "2x5 c1024 pool 2", b=3, h=2, w=5, c=1024, p=2)
def _maxpool(ctx, b, h, w, c, p):
    """out is one level's slice of the patch table [b, 2 p p, c]: rows [p p, 2 p p) of every image."""
    L = ctx.L
    x = _rand(131, b, c, h, w)
    xd = ctx.inp("x", x.permute(0, 2, 3, 1).reshape(b * h * w, c).contiguous(), ld=c + 4)
    out = ctx.out("out", (b, p * p, c), ld=c + 8, bs=2 * p * p)
    rows2d = out[0]                                                   # the wrapper reads the row pitch from stride(0)

    def value(o):             # tests/test_gpu_bricks.py:130-131: exact
        ref = F.adaptive_max_pool2d(x, (p, p)).permute(0, 2, 3, 1).reshape(b, p * p, c)
        assert torch.equal(o["out"].cpu(), ref)
    return Run(lambda: L.adaptive_maxpool_nhwc(xd, rows2d, 2 * p * p * (c + 8), b, h, w, c, p), lambda: {"out": out}, value,
               f"{b} x {h}x{w} c {c} pool {p}")


@case("wd_cross_attention_small", "200 queries, 64 keys, head_dim 64", b=1, nq=200, nk=64, heads=2, dh=64)
@case("wd_cross_attention_small", "one query, one key, head_dim 8", b=3, nq=1, nk=1, heads=8, dh=8)
@case("wd_cross_attention_small", "5 queries, 27 keys, head_dim 16", b=2, nq=5, nk=27, heads=4, dh=16)
def _xattn(ctx, b, nq, nk, heads, dh):
    L = ctx.L
    q, k, v = _rand(141, b, nq, heads, dh), _rand(142, b, nk, heads, dh), _rand(143, b, nk, heads, dh)
    hd = heads * dh
    qd = ctx.inp("q", q.view(b * nq, hd), ld=hd + 4)
    kd, vd = ctx.inp("k", k.view(b * nk, hd), ld=hd + 8), ctx.inp("v", v.view(b * nk, hd), ld=hd + 8)
    out = ctx.out("out", (b * nq, hd), ld=hd + 4)

    def value(o):             # tests/test_gpu_bricks.py:134-138
        a = F.softmax(torch.einsum("bnmc,bkmc->bmnk", q.double(), k.double()) / dh ** 0.5, dim=-1)
        assert_close("cross attention", o["out"].cpu(), torch.einsum("bmnk,bkmc->bnmc", a, v.double()).reshape(b * nq, hd), *TOL_XATTN)
    return Run(lambda: L.cross_attention_small(qd, kd, vd, out, b, nq, nk, heads, dh), lambda: {"out": out}, value,
               f"{b} x {nq} queries x {nk} keys, heads {heads} x {dh}")


# ================================================================================================ preprocess.hip
def _img(seed, h, w):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


@case("wd_letterbox_u8", "375x500 -> 64x96 canvas (shrink, pad top / bottom)", h=375, w=500, th=64, tw=96)
@case("wd_letterbox_u8", "17x5 -> 40x40 canvas (enlarge, pad left / right)", h=17, w=5, th=40, tw=40)
@case("wd_letterbox_u8", "9x601 -> 64x64 canvas (one-row result)", h=9, w=601, th=64, tw=64)
def _letterbox(ctx, h, w, th, tw):
    L = ctx.L
    from wedetect_amd.preprocess import letterbox_geometry, resample_coeffs
    src = _img(151, h, w)
    nw, nh, left, top, _, _ = letterbox_geometry(w, h, (th, tw))
    (bh, kh), (bv, kv) = resample_coeffs(w, nw), resample_coeffs(h, nh)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    sd = ctx.inp("src", src, mis=4)
    bhd, khd, bvd, kvd = ctx.inp("bounds_h", t(bh), mis=4), ctx.inp("kk_h", t(kh), mis=4), ctx.inp("bounds_v", t(bv), mis=4), ctx.inp("kk_v", t(kv), mis=4)
    tmp = ctx.ws("tmp", h * nw * 3, mis=4)
    dst = ctx.out("dst", (th, tw, 3), u8, mis=4)

    def value(o):             # tests/test_gpu_preprocess.py:37-38: the host letterbox, bit for bit
        from oracle import resample
        ref = resample.letterbox_u8(src.numpy(), (th, tw))
        ref = ref[0] if isinstance(ref, tuple) else ref
        assert np.array_equal(o["dst"].cpu().numpy(), np.asarray(ref))
    return Run(lambda: L.letterbox_u8(sd, h, w, bhd, khd, kh.shape[1], bvd, kvd, kv.shape[1], tmp, dst, th, tw, nw, nh, left, top, (114, 114, 114)),
               lambda: {"dst": dst}, value, f"{h}x{w} -> {nh}x{nw} at ({top}, {left}) of {th}x{tw}")


@case("wd_cv_resize_paste_u8", "area 33x47 -> 20x31", sh=33, sw=47, dh=20, dw=31, mode="area")
@case("wd_cv_resize_paste_u8", "area fast 2x: 36x50 -> 18x25", sh=36, sw=50, dh=18, dw=25, mode="area")
@case("wd_cv_resize_paste_u8", "bilinear 9x7 -> 23x31, channels swapped", sh=9, sw=7, dh=23, dw=31, mode="bilinear", swap=True)
@case("wd_cv_resize_paste_u8", "copy 21x31", sh=21, sw=31, dh=21, dw=31, mode="area")
def _cv_resize(ctx, sh, sw, dh, dw, mode, swap=False, ch=40, cw=44):
    L = ctx.L
    from wedetect_amd.pipeline import resize_plan
    src = _img(161, sh, sw)
    plan = resize_plan(sh, sw, dh, dw, mode)
    dev = {k_: ctx.inp(k_, torch.from_numpy(np.ascontiguousarray(v)), mis=4) for k_, v in plan.items() if isinstance(v, np.ndarray)}
    sd = ctx.inp("src", src, mis=4)
    dst = ctx.out("dst", (ch, cw, 3), u8, mis=4)
    top, left = (ch - dh) // 2, (cw - dw) // 2

    def launch():
        L.cv_resize_paste_u8(sd, sh, sw, plan["mode"], dev.get("xa"), dev.get("xidx"), dev.get("xw"), dev.get("ya"), dev.get("yidx"),
                             dev.get("yw"), plan.get("p0", 0), plan.get("p1", 0), plan.get("p2", 0.0), dst, ch, cw, dh, dw, top, left, 114, swap)

    def value(o):             # tests/test_gpu_entry.py:131-142
        from oracle import cv2_resize as cv
        ref = cv.cv2_resize_u8(src.numpy(), (dw, dh), mode) if (sh, sw) != (dh, dw) else src.numpy()
        want = np.full((ch, cw, 3), 114, np.uint8)
        want[top:top + dh, left:left + dw] = ref[..., ::-1] if swap else ref
        assert np.array_equal(o["dst"].cpu().numpy(), want)
    return Run(launch, lambda: {"dst": dst}, value, f"{mode} {sh}x{sw} -> {dh}x{dw}, kernel mode {plan['mode']}")


@case("wd_chw_to_hwc_u8", "uint8 2x3x8x12", b=2, h=8, w=12, is_f32=False)
@case("wd_chw_to_hwc_u8", "float32 1x3x5x7", b=1, h=5, w=7, is_f32=True)
def _chw(ctx, b, h, w, is_f32):
    L = ctx.L
    x = torch.from_numpy(np.random.default_rng(171).integers(0, 256, (b, 3, h, w), dtype=np.uint8))
    src = ctx.inp("src", x.float() + 0.25 if is_f32 else x, mis=4)
    dst = ctx.out("dst", (b, h, w, 3), u8, mis=4)
    return Run(lambda: L.chw_to_hwc_u8(src, dst), lambda: {"dst": dst},
               lambda o: None if torch.equal(o["dst"].cpu(), x.flip(1).permute(0, 2, 3, 1)) else pytest.fail("chw_to_hwc differs"),
               f"{b}x3x{h}x{w} f32 {is_f32}")


# ================================================================================================ evaluate / det_eval
@case("wd_recall_match", "6 images, up to 40 gts x 120 proposals, 3 budgets", legacy=False)
@case("wd_recall_match", "legacy coordinates", legacy=True)
def _recall(ctx, legacy, n_img=6):
    L = ctx.L
    g = np.random.default_rng(77)
    gts, props = [], []
    for i in range(n_img):
        ng, npr = (0, 9) if i == 1 else (int(g.integers(1, 41)), int(g.integers(0, 121)))
        a = g.uniform(0, 600, (ng, 2)); a = np.concatenate([a, a + g.uniform(5, 250, (ng, 2))], 1).astype(np.float32)
        b = g.uniform(0, 600, (npr, 2)); b = np.concatenate([b, b + g.uniform(5, 250, (npr, 2))], 1).astype(np.float32)
        if ng > 2 and npr > 6:
            b[0], b[5] = a[1], a[1]
        gts.append(a)
        props.append(b)
    nums = np.array([10, 100, 300])
    g_off, p_off = np.zeros(n_img + 1, np.int32), np.zeros(n_img + 1, np.int32)
    g_off[1:], p_off[1:] = np.cumsum([x.shape[0] for x in gts]), np.cumsum([x.shape[0] for x in props])
    total_gt, nb = int(g_off[-1]), nums.size
    per_block = int(L.LIB.wd_recall_scratch_floats(max(x.shape[0] for x in gts), max(min(x.shape[0], 300) for x in props)))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    gd, pd = ctx.inp("gts", t(np.concatenate(gts))), ctx.inp("props", t(np.concatenate(props)))
    god, pod, bud = ctx.inp("gt_off", t(g_off), mis=4), ctx.inp("prop_off", t(p_off), mis=4), ctx.inp("budgets", t(nums.astype(np.int32)), mis=4)
    scratch = ctx.ws("scratch", 4 * per_block * n_img * nb, row_pitch=4 * 300)
    out = ctx.out("out", (nb, total_gt), mis=4)

    def launch():
        L.check(L.LIB.wd_recall_match(gd.data_ptr(), god.data_ptr(), pd.data_ptr(), pod.data_ptr(), n_img, bud.data_ptr(), nb,
                                      scratch.data_ptr(), per_block, out.data_ptr(), total_gt, int(legacy), L.stream_ptr()), "wd_recall_match")

    def value(o):             # tests/test_gpu_evaluate.py:45-46: bit-exact vs the oracle
        from oracle import evaluate as oe
        assert np.array_equal(o["out"].cpu().numpy(), oe.matched_ious(gts, props, nums, legacy=legacy))
    return Run(launch, lambda: {"out": out}, value, f"{n_img} images, {total_gt} gts, scratch {per_block} floats per block")


def _det_case(ctx, set_kw, stage, want_scratch=None, want_padding=False):
    """wd_det_match -> wd_det_sort -> wd_det_accumulate with every operand of the three calls in the arena (the host side restates
    wedetect_amd.det_eval._device_eval); value: np.array_equal with tests/det_eval_ref.py (tests/test_gpu_det_eval.py:24-31)."""
    L = ctx.L
    from tests import det_eval_ref as R
    from wedetect_amd import det_eval as DE
    ann, dets = R.make_set(**set_kw)
    img_ids = np.unique(np.asarray([im["id"] for im in ann["images"]], np.int64))
    cat_ids = np.unique(np.asarray([c["id"] for c in ann["categories"]], np.int64))
    g_img, g_cat, g_box, g_area, g_flag = DE._gt_arrays(ann, lvis=False)
    d_img, d_cat, d_box, d_score = DE.flatten_dets(dets)
    d_flag = np.zeros(d_img.shape[0], np.uint8)
    max_dets, trunc = DE.COCO_MAX_DETS, DE.COCO_MAX_DETS[-1]
    T, Rr, K, A4, M = 10, 101, len(cat_ids), 4, len(max_dets)
    n_img = len(img_ids)
    gkey = np.searchsorted(cat_ids, g_cat) * n_img + np.searchsorted(img_ids, g_img)
    dkey = np.searchsorted(cat_ids, d_cat) * n_img + np.searchsorted(img_ids, d_img)
    go, do = np.argsort(gkey, kind="stable"), np.argsort(dkey, kind="stable")
    gk, dk = gkey[go], dkey[do]
    pkeys = np.union1d(gk, dk)
    P = pkeys.shape[0]
    g_off = np.append(np.searchsorted(gk, pkeys, "left"), gk.shape[0]).astype(np.int64)
    d_off = np.append(np.searchsorted(dk, pkeys, "left"), dk.shape[0]).astype(np.int64)
    n_det, n_gt = np.diff(d_off), np.diff(g_off)
    kept = np.minimum(n_det, trunc)
    slot_off = np.zeros(P + 1, np.int64)
    slot_off[1:] = np.cumsum(kept)
    n_slot = int(slot_off[-1])
    pair_cat = (pkeys // n_img).astype(np.int32)
    cat_pair_off = np.searchsorted(pair_cat, np.arange(K + 1)).astype(np.int64)
    cat_slot_off = slot_off[cat_pair_off]
    need = np.asarray([int(L.LIB.wd_det_match_workspace_bytes(int(a), int(b))) for a, b in zip(kept, n_gt)], np.int64)
    big = need > int(L.LIB.wd_det_match_lds_bytes())
    scr = np.full(P, -1, np.int64)
    if big.any():
        scr[big] = np.concatenate([[0], np.cumsum(need[big])[:-1]])
    scr_bytes = int(need[big].sum()) if big.any() else 16
    n2 = 2
    while n2 < n_slot:
        n2 *= 2
    if want_scratch is not None:
        assert bool(big.any()) == want_scratch, f"{int(big.sum())} of {P} pairs exceed the LDS slice: the case is named for {want_scratch}"
    if want_padding:
        assert n_slot < n2, "the case is named for a slot count that is not a power of two"
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt))
    pdo, pgo, pso = ctx.inp("pair_det_off", t(d_off, np.int32), mis=4), ctx.inp("pair_gt_off", t(g_off, np.int32), mis=4), ctx.inp("pair_slot_off", t(slot_off, np.int32), mis=4)
    pcat, pscr = ctx.inp("pair_cat", t(pair_cat, np.int32), mis=4), ctx.inp("pair_scratch", t(scr, np.int64), mis=8)
    dbox, dsc, dfl = ctx.inp("det_box", t(d_box[do], np.float32)), ctx.inp("det_score", t(d_score[do], np.float32), mis=4), ctx.inp("det_flag", t(d_flag[do], np.uint8), mis=1)
    gbox, gar, gfl = ctx.inp("gt_box", t(g_box[go], np.float64)), ctx.inp("gt_area", t(g_area[go], np.float64), mis=8), ctx.inp("gt_flag", t(g_flag[go], np.uint8), mis=1)
    thr = ctx.inp("iou_thr", t([min(v, 1 - 1e-10) for v in DE.iou_thrs()], np.float64), mis=8)
    rng = ctx.inp("area_rng", t(np.asarray(DE.AREA_RNG, np.float64).reshape(-1), np.float64), mis=8)
    scratch = ctx.ws("scratch", scr_bytes)
    slot_score, slot_rank = ctx.out("slot_score", (n_slot,), mis=4), ctx.out("slot_rank", (n_slot,), i32, mis=4)
    keys0 = torch.full((n2, 2), -1, dtype=i64)                       # WdDetSortKey padding: all ones
    sort_keys = ctx.inout("sort_keys", keys0)
    flags = ctx.out("flags", (40 * n_slot,), u8, mis=1)
    npig = ctx.inout("npig", torch.zeros(P * 4, dtype=i32), mis=4)
    err = ctx.flag("err")
    s_rank, s_score, s_flags = ctx.out("sorted_rank", (n_slot,), i32, mis=4), ctx.out("sorted_score", (n_slot,), mis=4), ctx.out("sorted_flags", (40 * n_slot,), u8, mis=1)
    cso, cpo = ctx.inp("cat_slot_off", t(cat_slot_off, np.int32), mis=4), ctx.inp("cat_pair_off", t(cat_pair_off, np.int32), mis=4)
    md, rec = ctx.inp("max_dets", t(max_dets, np.int32), mis=4), ctx.inp("rec_thr", t(DE.rec_thrs(), np.float64), mis=8)
    neg = lambda *s: torch.full(s, -1.0, dtype=f64)
    precision, recall, scores = ctx.inout("precision", neg(T, Rr, K, A4, M), mis=8), ctx.inout("recall", neg(T, K, A4, M), mis=8), ctx.inout("scores", neg(T, Rr, K, A4, M), mis=8)
    keys_d, npig0 = keys0.cuda(), torch.zeros(P * 4, dtype=i32, device="cuda")
    fill = [(precision, -1.0), (recall, -1.0), (scores, -1.0)]

    def launch():
        sort_keys.copy_(keys_d)
        npig.copy_(npig0)
        for buf, v in fill:
            buf.fill_(v)
        p = lambda x: x.data_ptr()
        L.check(L.LIB.wd_det_match(p(pdo), p(pgo), p(pso), p(pcat), p(pscr), P, p(dbox), p(dsc), p(dfl), p(gbox), p(gar), p(gfl), p(thr), p(rng),
                                   int(trunc), p(scratch), p(slot_score), p(slot_rank), p(sort_keys), p(flags), n_slot, p(npig), p(err),
                                   L.stream_ptr()), "wd_det_match")
        L.check(L.LIB.wd_det_sort(p(sort_keys), n2, L.stream_ptr()), "wd_det_sort")
        L.check(L.LIB.wd_det_accumulate(p(sort_keys), n_slot, p(slot_rank), p(slot_score), p(flags), p(s_rank), p(s_score), p(s_flags), p(cso),
                                        p(cpo), p(npig), K, p(rec), p(md), M, p(precision), p(recall), p(scores), L.stream_ptr()), "wd_det_accumulate")

    def value(o):
        ref = R.coco_eval(ann, dets)
        for k_ in ("precision", "recall", "scores"):
            assert np.array_equal(o[k_].cpu().numpy(), ref[k_]), k_
    outs = lambda: dict(precision=precision, recall=recall, scores=scores, sort_keys=sort_keys, slot_rank=slot_rank, slot_score=slot_score,
                        flags=flags, npig=npig, sorted_rank=s_rank, sorted_score=s_score, sorted_flags=s_flags)
    return Run(launch, outs, value, f"{stage}: {P} pairs ({int(big.sum())} on global scratch), {n_slot} slots sorted as {n2}", [err], finite=False)


_g_small = dict(seed=0, n_img=20, n_cat=5, crowd_frac=0.15, empty_frac=0.15, no_det_frac=0.15)
_g_big = dict(seed=12, n_img=12, n_cat=4, extra=[(3, 1, 1300, 6), (5, 2, 300, 120)])
CASES.append(Case("wd_det_match", "every pair in LDS", lambda ctx: _det_case(ctx, _g_small, "match", want_scratch=False)))
CASES.append(Case("wd_det_match", "pairs on global scratch, truncation at 1000", lambda ctx: _det_case(ctx, _g_big, "match", want_scratch=True)))
CASES.append(Case("wd_det_sort", "slot count not a power of two (padding keys sort last)", lambda ctx: _det_case(ctx, dict(_g_small, seed=1), "sort", want_padding=True)))
CASES.append(Case("wd_det_accumulate", "score ties", lambda ctx: _det_case(ctx, dict(seed=11, n_img=15, n_cat=5, tie_levels=4, dets_per_img=60), "accumulate")))


# ================================================================================================ sensitivity
def _case_named(entry, part):
    hit = [c for c in CASES if c.entry == entry and part in c.name]
    assert len(hit) == 1, (entry, part, [c.name for c in hit])
    return hit[0]


def test_harness_sees_the_kernels_own_last_stores():
    """Sensitivity without a misbehaving kernel: declare an output one row / one column / 16 bytes SMALLER than the truth and
    the kernel's legitimate stores at the edge are reported at the right offsets — the harness sees real device stores."""
    # (1) WD_SPLIT_C GEMM with ldc > n: one row less -> the last row's n * 4 bytes directly behind the declared end (the spare
    #     columns of the row before it lie in between: the report starts right after them)
    c = _case_named("wd_conv_gemm_split", "pre-split cfg60 m129 n136 k80 gelu -> hi/lo")
    _, v, _ = execute(c, 0x00, 0xFF, shrink=lambda ar: ar.shrink("c", rows=1))
    v = [r for r in v if r["buffer"] == "c"]
    assert len(v) == 1 and v[0]["side"] == "high guard", v
    assert 8 * 4 + 1 <= v[0]["first"] <= 8 * 4 + 4 and 8 * 4 + 136 * 4 - 3 <= v[0]["last"] <= 8 * 4 + 136 * 4 and v[0]["count"] > 136 * 4 * 0.9, v
    #     and one column (one float) less: 4 bytes behind every row
    _, v, _ = execute(c, 0xFF, 0xFF, shrink=lambda ar: ar.shrink("c", cols=1))
    v = {r["side"]: r for r in v if r["buffer"] == "c"}
    assert set(v) == {"high guard", "spare columns"}, v
    assert v["high guard"]["first"] <= 2 and v["high guard"]["last"] <= 4
    assert v["spare columns"]["first"][0] == 0 and v["spare columns"]["last"] == (127, v["spare columns"]["last"][1]) and v["spare columns"]["last"][1] <= 4
    # (2) a depthwise form: the last pixel's channels
    c = _case_named("wd_dwconv7_variant", "form 4 c32 17x20")
    _, v, _ = execute(c, 0xFF, 0xFF, shrink=lambda ar: ar.shrink("y", rows=1))
    v = [r for r in v if r["buffer"] == "y"]
    assert len(v) == 1 and v[0]["side"] == "high guard" and v[0]["first"] <= 2 and 32 * 4 - 1 <= v[0]["last"] <= 32 * 4, v
    assert v[0]["count"] >= 0.9 * 32 * 4, v                         # a byte of a float may equal the pattern by chance
    # (3) top-k: the last 16 bytes of the index rows (-1 filler of the last image) and of the workspace (all-ones padding keys)
    c = _case_named("wd_topk_candidates", "beyond the capacity")
    _, v, _ = execute(c, 0x00, 0xFF, shrink=lambda ar: (ar.shrink("out_idx", tail_bytes=16), ar.shrink("workspace", tail_bytes=16)))
    v = {r["buffer"]: r for r in v}
    assert set(v) == {"out_idx", "workspace"}, v
    assert v["out_idx"] == dict(buffer="out_idx", side="high guard", first=1, last=16, count=16), v
    assert v["workspace"]["side"] == "high guard" and v["workspace"]["last"] <= 16, v
