"""The size limits of the large-offset table (tests/offsets_cases.py) without a device: every row that says "refused" is taken
through the C ABI with aligned dummy pointers — a refusal precedes any launch, so nothing is dereferenced — at the boundary, one
unit past it, and one unit inside.

One unit INSIDE passes every check and reaches the launch.  Without a device that launch fails with WD_ERR_LAUNCH, which is the
assertion here (the limit under test did not refuse it).  Where a device is present the inside call is left out, since it would
launch on dummy pointers; tests/test_gpu_offsets.py runs the accepted side of each limit there, on real operands.
"""
import ctypes as C
import os
import re

import pytest
import torch

from tests import offsets_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED = [c for c in O.CASES if c.expect == "refused"]
PTR = C.c_void_p(1 << 20)                       # non-null, 4 KiB aligned, never dereferenced
FLT3 = (C.c_float * 3)(1.0, 1.0, 1.0)


def _no_device() -> bool:
    return torch.cuda.device_count() == 0


def _inside(call) -> None:
    """``call()`` is one unit inside a limit: it must get as far as the launch."""
    if _no_device():
        rc = call()
        assert rc == O.LAUNCH, f"one unit inside the limit: expected to reach the launch (WD_ERR_LAUNCH without a device), got {rc}"


def _gemm(L, *, m, n, cin, lda, kh=1, stride=1, pad=0, b=1, h=1, w=None, flags=1, cfg=-1):
    """wd_conv_gemm_split on dummy pointers; plain rows unless kh > 1."""
    if w is None:
        w = m
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kh) // stride + 1
    p = L.ConvGemm(a=PTR.value, w=0, bias=0, res=0, c=PTR.value, batch=b, hin=h, win=w, cin=cin, lda=lda, kh=kh, kw=kh, stride=stride,
                   pad=pad, hout=ho, wout=wo, m=b * ho * wo, n=n, k=kh * kh * cin, ldc=n, ldres=0, act=0, out_mode=0, res_alpha=1.0,
                   out_scale=1.0, out_bias=0.0, a_scale=1.0, c_split_scale=1.0)
    return L.LIB.wd_conv_gemm_split(C.byref(p), PTR, 1.0, flags, cfg, None)


def _fused(entry, *, rows=8, n_cls, dim, cls_offset=0, rows_per_img=8, n_cls_total=None, ldo=None):
    """One of the four fused score entries on dummy pointers (no seg affine, no range flag)."""
    head = (PTR, rows, PTR, 1.0, n_cls, dim, 0, 0, 0, None, None)
    if entry == "wd_best_similarity_split":
        from wedetect_amd import best as M
        return M.LIB.wd_best_similarity_split(*head, None, cls_offset, PTR, None)
    if entry == "wd_topn_similarity_split":
        from wedetect_amd import topn as M
        return M.LIB.wd_topn_similarity_split(*head, None, None, None, cls_offset, 4, PTR, None)
    if entry == "wd_group_similarity_split":
        from wedetect_amd import groups as M
        return M.LIB.wd_group_similarity_split(*head, None, PTR, PTR, cls_offset, PTR, ldo or 16, 16, None)
    if entry == "wd_sparse_similarity_split":
        from wedetect_amd import sparse as M
        total = n_cls_total if n_cls_total is not None else cls_offset + n_cls
        return M.LIB.wd_sparse_similarity_split(*head, None, cls_offset, rows_per_img, total, 0.5, PTR, 1024, PTR, None)
    raise KeyError(entry)


# ------------------------------------------------------------------------------------------------ the runners, by family
def run_presplit_limit(c, L):
    k = c.kw
    unit = 16 if k["cfg"] == 66 else 8                                            # the row group of the kernel's DMA
    call = lambda m, cfg=k["cfg"], n=k["n"], kk=k["k"], lda=k["lda"]: _gemm(L, m=m, n=n, cin=kk, lda=lda, cfg=cfg)
    assert k["m"] * k["lda"] * 4 == 1 << 32
    assert call(k["m"]) == c.code and call(k["m"] + unit) == c.code
    assert k["m_in"] == k["m"] - unit
    _inside(lambda: call(k["m_in"]))
    # the weight operand has the same limit: n * round_up(k, 16) * 4 == 2^32 with n = 2^20, k = 1024
    assert call(4096, n=1 << 20, kk=1024, lda=1024) == c.code and call(4096, n=(1 << 20) + 256, kk=1024, lda=1024) == c.code
    _inside(lambda: call(4096, n=(1 << 20) - 256, kk=1024, lda=1024))
    # production dispatch picks by shape, then by this limit: the shape the forced tile refuses is not refused
    _inside(lambda: call(k["m"], cfg=-1))
    _inside(lambda: call(M_LONG, cfg=-1, lda=k["lda"]))


M_LONG = 131072 + 256                              # the "very long m" class of pick_presplit_cfg (cfg 66 / 63)


def run_tap_limit(c, L):
    k = c.kw
    call = lambda lda, kh=k["kh"], stride=1, pad=1, cfg=k["cfg"]: _gemm(L, m=0, b=1, h=k["h"], w=k["w"], n=k["n"], cin=k["cin"], lda=lda, kh=kh,
                                                                      stride=stride, pad=pad, cfg=cfg)
    taps = (k["kh"] - 1) * k["w"] + k["kh"] - 1
    assert k["lda_in"] == O.tap_limit_lda(k["kh"], k["kh"], k["w"], k["cin"]) and k["lda"] == k["lda_in"] + 8
    assert taps * k["lda_in"] * 4 + k["cin"] * 4 <= 1 << 31 < taps * k["lda"] * 4 + k["cin"] * 4
    assert call(k["lda"]) == c.code and call(k["lda"] + 8) == c.code
    _inside(lambda: call(k["lda_in"]))
    if k["cfg"] == -1:                                                            # the strided and the 2 x 2 geometries: the same rule, their own taps
        for kh, stride, pad in ((3, 2, 1), (2, 2, 0)):
            lim = O.tap_limit_lda(kh, kh, k["w"], k["cin"])
            assert call(lim + 8, kh, stride, pad) == c.code
            _inside(lambda: call(lim, kh, stride, pad))
        # a 1 x 1 layer has no tap offset: the widest lda an int holds is not refused for it
        _inside(lambda: _gemm(L, m=8, n=k["n"], cin=k["cin"], lda=(1 << 31) - 8, cfg=70))


def run_cls_limit(c, L):
    k = c.kw
    unit = 32 if "group" in c.entry else 1
    call = lambda off: _fused(c.entry, n_cls=k["n_cls"], dim=k["dim"], cls_offset=off)
    assert k["cls_offset"] + k["n_cls"] > (1 << 31) - 1 >= k["cls_in"] + k["n_cls"] and k["cls_offset"] - k["cls_in"] == unit
    assert call(k["cls_offset"]) == c.code
    if k["cls_offset"] + unit < 1 << 31:                                           # one unit further still fits the int32 argument
        assert call(k["cls_offset"] + unit) == c.code
    _inside(lambda: call(k["cls_in"]))


def run_sparse_limit(c, L):
    k = c.kw
    call = lambda rpi, total: _fused(c.entry, rows=rpi, n_cls=264, dim=64, rows_per_img=rpi, n_cls_total=total)
    assert k["rows_per_img"] * k["total_in"] < 1 << 31 <= k["rows_per_img"] * k["n_cls_total"] and k["n_cls_total"] == k["total_in"] + 1
    assert call(512, 1 << 22) == c.code                                           # exactly 2^31
    assert call(k["rows_per_img"], k["n_cls_total"]) == c.code and call(k["rows_per_img"], k["n_cls_total"] + 1) == c.code
    _inside(lambda: call(k["rows_per_img"], k["total_in"]))


def run_bank_limit(c, L):
    dim = c.kw["dim"]
    unit = 32 if "group" in c.entry else 1
    n = unit
    while O.bank_fits(n + unit, dim):                                             # doubling walk to the last n that fits
        step = unit
        while O.bank_fits(n + 2 * step, dim):
            step *= 2
        n += step
    n_bad = n + unit
    assert O.bank_fits(n, dim) and not O.bank_fits(n_bad, dim)
    assert ((n_bad + 7) & ~7) * dim * 4 >= 1 << 32 > ((n + 7) & ~7) * dim * 4
    call = lambda nn: _fused(c.entry, n_cls=nn, dim=dim)
    assert call(n_bad) == c.code and call(n_bad + unit) == c.code
    _inside(lambda: call(n))


def run_dwconv_limit(c, L):
    """Forced variant 4 (the LDS-DMA form): 24-bit products and (h + 8) * w * c * 4 < 2^32 (elementwise.hip, dwconv7_dma_ok)."""
    k = c.kw
    x, y = PTR, C.c_void_p(2 << 20)
    call = lambda h, w=k["w"], cc=k["c"]: L.LIB.wd_dwconv7_variant(x, PTR, PTR, y, 1, h, w, cc, 4, None)
    assert (k["h"] + 8) * k["w"] * k["c"] * 4 == 1 << 32 and k["h_in"] == k["h"] - 1
    assert call(k["h"]) == c.code and call(k["h"] + 1) == c.code and call(1032) == c.code
    _inside(lambda: call(k["h_in"]))
    # the row of pixels itself: w * c * 4 < 2^23
    assert call(8, 2048, 1024) == c.code and call(8, 2049, 1024) == c.code
    _inside(lambda: call(8, 2047, 1024))
    # the production entry refuses neither: it takes another form
    _inside(lambda: L.LIB.wd_dwconv7(x, PTR, PTR, y, 1, 1032, k["w"], k["c"], None))


RUNNERS = {"dwconv_limit": run_dwconv_limit, "presplit_limit": run_presplit_limit, "tap_limit": run_tap_limit, "cls_limit": run_cls_limit, "sparse_limit": run_sparse_limit,
           "bank_limit": run_bank_limit}


@pytest.mark.parametrize("c", REFUSED, ids=[c.id for c in REFUSED])
def test_refused_at_the_boundary_and_one_past_accepted_one_inside(c):
    from wedetect_amd import lib as L
    assert c.code in (O.BAD_ARG, O.UNSUPPORTED)
    RUNNERS[c.family](c, L)


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "wedetect_hip.h")).read()
    for name, val in (("WD_OK", O.OK), ("WD_ERR_BAD_ARG", O.BAD_ARG), ("WD_ERR_LAUNCH", O.LAUNCH), ("WD_ERR_UNSUPPORTED", O.UNSUPPORTED)):
        m = re.search(rf"#define {name} \(?(-?\d+)\)?", hdr)
        assert m and int(m.group(1)) == val, name


def test_chunk_constants_of_the_fused_callers_fit_the_bank_limit():
    """The four FUSED_CHUNK constants are classes per fused launch of a 768-wide bank (engine.EMBED_DIM, the only width the
    detector's score step takes); parallel.TopNamer cuts banks of any width with a step of its own.  Both against
    wd_similarity_bank_fits, restated in offsets_cases.bank_fits and held to the library by the bank_limit rows above."""
    from wedetect_amd import best, engine, groups, sparse, topn
    chunks = {m.__name__: m.FUSED_CHUNK for m in (best, topn, groups, sparse)}
    assert set(chunks.values()) == {1 << 20}, chunks
    assert engine.EMBED_DIM == 768 and O.bank_fits(1 << 20, 768)
    assert groups.FUSED_CHUNK % 32 == 0 and (1 << 20) % 8 == 0                    # whole bins / whole row groups per chunk
    # at 1024 the constant alone is one row group too many: a caller at another width must cut like parallel.py does
    assert not O.bank_fits(1 << 20, 1024) and O.bank_fits((1 << 20) - 8, 1024)
    for dim in (768, 1024, 64, 4096):
        row_bytes = (dim + 15) // 16 * 16 * 4                                      # parallel.TopNamer._launch's expression
        step = min(topn.FUSED_CHUNK, (((1 << 32) - 1) // row_bytes - 8) // 8 * 8)
        assert step > 0 and step % 8 == 0 and O.bank_fits(step, dim), (dim, step)
        assert step == topn.FUSED_CHUNK or not O.bank_fits(step + 16, dim), (dim, step)     # and not needlessly small
        assert step == O.retrieval_chunk(dim)                                     # the C entry's own loop uses the same figure
    assert O.retrieval_chunk(768) == 1 << 20 and O.retrieval_chunk(1024) == (1 << 20) - 16


def test_retrieval_chunk_leaves_room_for_the_padding_group():
    """offsets_cases.retrieval_chunk restates the chunk of wd_retrieval_max_split; the device cases hold the restatement itself: they
    cut the bank at the seams it predicts and compare every class with separate calls."""
    for dim in (32, 64, 768, 1024, 4096):
        ch = O.retrieval_chunk(dim)
        assert ch % 8 == 0 and (ch + 8) * dim * 4 < 1 << 32                       # the chunk and its padding group end below 2^32


# ------------------------------------------------------------------------------------------------ coverage of the C ABI
HEADERS = ("wedetect_hip.h", "wedetect_hip_best.h", "wedetect_hip_topn.h", "wedetect_hip_groups.h", "wedetect_hip_sparse.h")
ADDRESSING = re.compile(r"^(ld\w*|\w*stride\w*|rows|rows_per_img|n_per_image|cls_offset)$")


def _addresses_by_argument(proto) -> bool:
    """A stride, row-count or class-offset parameter, or the WdConvGemm description (which carries lda / ldc / ldres / ldc2 /
    c_batch_stride) — of a function that takes device memory (size queries address nothing)."""
    from tests.test_cpu_arena import _takes_memory
    return _takes_memory(proto) and any("WdConvGemm" in p or ADDRESSING.match(p.split()[-1].lstrip("*")) for p in proto[1])


def test_every_entry_with_a_stride_row_count_or_class_offset_has_a_case_or_an_exemption():
    from tests.abi_decl import declared
    decl = {name: proto for h in HEADERS for name, proto in declared(h).items()}      # every wd_* function of the five headers
    assert len(decl) >= 70 and {"wd_conv_gemm", "wd_layernorm_rows", "wd_topk_candidates", "wd_group_rows"} <= set(decl)
    covered = {c.entry for c in O.CASES}
    assert not covered - set(decl), f"cases for entry points no header declares: {sorted(covered - set(decl))}"
    for name, params in sorted(decl.items()):
        if _addresses_by_argument(params):
            assert name in covered or name in O.EXEMPT, f"{name}: no row in tests/offsets_cases.py and no EXEMPT reason"
        assert not (name in covered and name in O.EXEMPT), f"{name}: both covered and exempt"
    for name, reason in O.EXEMPT.items():
        assert name in decl and _addresses_by_argument(decl[name]), f"EXEMPT names {name}, which has no such parameter"
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason
    ids = [c.id for c in O.CASES]
    assert len(ids) == len(set(ids)), "case ids must be unique"
    # every public header is either under the condition above or left out by name, with a reason
    from wedetect_amd import build as WB
    assert set(WB.PUBLIC_HEADERS) == set(HEADERS) | set(O.EXEMPT_HEADERS) and not set(HEADERS) & set(O.EXEMPT_HEADERS)
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in O.EXEMPT_HEADERS.values())
    # the table speaks the two words the two files read, and every family has a runner in its file
    from tests import test_gpu_offsets as G
    for c in O.CASES:
        assert c.expect in ("correct", "refused") and c.operand and c.boundary
        assert (c.family in RUNNERS) == (c.expect == "refused") and (c.family in G.RUNNERS) == (c.expect == "correct"), c.id
        assert (c.code == O.OK) == (c.expect == "correct")
