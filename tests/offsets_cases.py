"""The table of the large-offset tests: operands whose extent passes byte 2^31 and 2^32, the seams of chunked launches, and the
size limits at which an entry refuses.  tests/test_gpu_offsets.py runs the rows that say "correct" on the device;
tests/test_cpu_offsets.py takes the rows that say "refused" through the C ABI without one (a refusal precedes any launch) and holds
the coverage condition: every function of include/wedetect_hip.h and of the best / topn / groups / sparse headers that has a stride,
row-count or class-offset parameter is named by a row here or by EXEMPT.

Plain data: no torch, no device.  A giant operand is SPARSE: a row stride (lda, ldc, ...) far wider than the row, so that 65 792
rows span 4.3 GB while a launch touches 256 bytes of each.  With WIDE_LD = 16384 floats a row is 64 KiB: row 32768 starts at byte
2^31, row 65536 at byte 2^32.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

WIDE_LD = 16384                    # floats: 64 KiB per row
WIDE_LD_LN = 16448                 # LayerNorm: 65535 rows of it still pass 2^32 bytes (a multiple of 8 for the hi/lo output)
M_BIG = 65792                      # 257 tiles of 256 rows: 256 rows past byte 2^32 with WIDE_LD; a whole number of tiles of every height
M_RAGGED = 65780                   # the same number of tiles, the last one ragged for every tile height (two extra rows of the table)
GUARD = 2 << 30                    # bytes in front of and behind the operand under test
OK, BAD_ARG, LAUNCH, UNSUPPORTED = 0, -1, -2, -4   # WD_OK, WD_ERR_BAD_ARG, WD_ERR_LAUNCH, WD_ERR_UNSUPPORTED (include/wedetect_hip.h)


def bank_fits(n_cls: int, dim: int) -> bool:
    """wd_similarity_bank_fits (csrc/common.h) restated: the bank of one fused launch is addressed with 32-bit byte offsets."""
    return ((n_cls + 7) & ~7) * ((dim + 15) // 16 * 16) * 4 < 1 << 32


def retrieval_chunk(dim: int) -> int:
    """Classes per launch of wd_retrieval_max_split (split_gemm_pre.hip, the loop over c0): the largest multiple of eight whose
    rows, plus one padding group, end below 2^32 bytes; at most 2^20."""
    return min((((1 << 32) - 1) // (dim * 4) - 8) & ~7, 1 << 20)


def tap_limit_lda(kh: int, kw: int, win: int, cin: int) -> int:
    """Largest lda (a multiple of 8) the implicit-GEMM kernels of split_gemm_conv.hip accept for a kh x kw filter on rows of win
    pixels: ((kh - 1) * win + kw - 1) * lda * 4 + cin * 4 <= 2^31 (the tap offset is a 32-bit int)."""
    taps = (kh - 1) * win + kw - 1
    return ((1 << 31) - cin * 4) // (taps * 4) // 8 * 8


@dataclass(frozen=True)
class Case:
    entry: str                     # C ABI function
    name: str
    operand: str                   # the operand that crosses (or the argument the limit is on)
    expect: str                    # "correct" | "refused"
    boundary: str                  # which byte / element / class boundary, in words
    family: str                    # the runner of tests/test_gpu_offsets.py / tests/test_cpu_offsets.py
    kw: Dict = field(default_factory=dict)
    code: int = OK                 # refused: the error code

    @property
    def id(self) -> str:
        return f"{self.entry}[{self.name}]"


CASES: List[Case] = []


def _c(entry, name, operand, boundary, family, **kw):
    CASES.append(Case(entry, name, operand, "correct", boundary, family, kw))


def _r(entry, name, operand, boundary, family, code, **kw):
    CASES.append(Case(entry, name, operand, "refused", boundary, family, kw, code))


B31_32 = "rows on either side of byte 2^31 and 2^32"

# ---- 1. wd_conv_gemm (fp32 MFMA): m = 65 792, n = 48 and 81, cin = 64
for _n in (48, 81):
    for _op in ("a", "c", "res", "inplace"):
        _c("wd_conv_gemm", f"{_op} wide n{_n}", {"a": "a (lda)", "c": "c (ldc)", "res": "res (ldres)", "inplace": "c == res (ldc == ldres)"}[_op],
           B31_32, "gemm", kind="f32", wide=_op, m=M_BIG, n=_n, cin=64)
    _c("wd_conv_gemm", f"c_batch_stride n{_n}", "c (c_batch_stride: 16 rows per image, 5461 rows apart)", "images on either side of byte 2^31 and 2^32",
       "gemm", kind="f32", wide="cbs", m=M_BIG, n=_n, cin=64, hw=16, cbs=5461)
    _c("wd_conv_gemm", f"seg sigmoid ldo n{_n}", "c ([B, N, ldo] scores, ldo wide)", B31_32 + "; level boundaries inside each image",
       "gemm", kind="f32", wide="seg", m=M_BIG, n=_n, cin=64, seg_rows=8224, seg_ends=(6000, 7800))
_c("wd_conv_gemm", "deconv ldc n48", "c (OUT_DECONV2X2 scatter, ldc = 4096)", "output pixels on either side of byte 2^31 and 2^32", "gemm",
   kind="f32", wide="deconv", m=M_BIG, n=48, cin=64, b=2, h=257, w=128, ldc=4096)

_c("wd_conv_gemm", "c wide n81 ragged m", "c (ldc)", B31_32 + "; ragged last tile past byte 2^32", "gemm", kind="f32", wide="c", m=M_RAGGED, n=81,
   cin=64)

# ---- 2. wd_conv_gemm_split, loader-split (flags 0): cfg 50 / 51 / 52
for _cfg in (50, 51, 52):
    for _op in ("a", "c", "res"):
        _c("wd_conv_gemm_split", f"cfg{_cfg} {_op} wide", {"a": "a (lda)", "c": "c (ldc)", "res": "res (ldres)"}[_op], B31_32, "gemm",
           kind="split", cfg=_cfg, flags=0, wide=_op, m=M_BIG, n=48, cin=64)
_c("wd_conv_gemm_split", "cfg51 c wide ragged m", "c (ldc)", B31_32 + "; ragged last tile past byte 2^32", "gemm", kind="split", cfg=51, flags=0,
   wide="c", m=M_RAGGED, n=48, cin=64)
for _ldc in (WIDE_LD, WIDE_LD + 8):
    _c("wd_conv_gemm_split", f"WD_SPLIT_C ldc{_ldc}", "c (fp16 hi/lo groups, ldc wide)", B31_32, "gemm", kind="split", cfg=-1, flags=2,
       wide="c", m=M_BIG, n=48, cin=64, ldc=_ldc)
for _s in (2, 3):
    _c("wd_conv_gemm_split_ws", f"split-K {_s} c wide", "c (ldc), second pass of a forced split-K", B31_32, "gemm", kind="split", cfg=51,
       flags=0, wide="c", m=M_BIG, n=48, cin=64, splits=_s)

# ---- 3. pre-split plain layers (WD_SPLIT_A, K = 256, n = 256, lda = 16384)
for _cfg, _m in ((64, 65536), (65, 65536), (66, 65536)):
    _r("wd_conv_gemm_split", f"cfg{_cfg} m*lda*4 == 2^32", "a (m * lda * 4)", "m = 65536, lda = 16384: exactly 2^32 bytes", "presplit_limit",
       UNSUPPORTED, cfg=_cfg, m=_m, m_in=65528 if _cfg != 66 else 65520, lda=WIDE_LD, n=256, k=256)
    _c("wd_conv_gemm_split", f"cfg{_cfg} one row group inside", "a (lda)", "last rows within 512 KiB of byte 2^32, middle rows across 2^31",
       "gemm", kind="split", cfg=_cfg, flags=1, wide="a", m=65528 if _cfg != 66 else 65520, n=256, cin=256)
for _cfg in (60, 63):
    _c("wd_conv_gemm_split", f"cfg{_cfg} a wide", "a (lda)", B31_32, "gemm", kind="split", cfg=_cfg, flags=1, wide="a", m=M_BIG, n=256, cin=256)
_c("wd_conv_gemm_split", "production a wide == cfg60", "a (lda), cfg = -1", B31_32 + "; the shape cfg 64 refuses", "gemm", kind="split", cfg=-1,
   flags=1, wide="a", m=M_BIG, n=256, cin=256, same_as_cfg=60)
_c("wd_conv_gemm_split", "residual c wide", "c (ldc), WD_SPLIT_A with an fp32 residual", B31_32, "gemm", kind="split", cfg=-1, flags=1, wide="c",
   m=M_BIG, n=256, cin=256, res="sep")
_c("wd_conv_gemm_split", "dual output c wide", "c (hi/lo groups, ldc), fp32 twin c2 compact", B31_32, "gemm", kind="split", cfg=-1, flags=3,
   wide="c", m=M_BIG, n=256, cin=256, c2=True)
_c("wd_conv_gemm_split", "dual output c2 wide", "c2 (ldc2)", B31_32, "gemm", kind="split", cfg=-1, flags=3, wide="c2", m=M_BIG, n=256, cin=256,
   c2=True)

# ---- 4. implicit-GEMM kernels on pre-split activations: A crossed through the pixel index (B = 2, 182 x 182 pixels of lda = 16384)
for _name, _g in (("3x3 s1", dict(kh=3, stride=1, pad=1)), ("3x3 s2", dict(kh=3, stride=2, pad=1)), ("2x2 s2", dict(kh=2, stride=2, pad=0)),
                  ("deconv", dict(kh=1, stride=1, pad=0, deconv=True))):
    for _cfg in ((-1, 70, 77, 78, 79) if _name == "3x3 s1" else (-1,)):
        _c("wd_conv_gemm_split", f"conv {_name} cfg{_cfg} a wide", "a (pixel index * lda)", "pixels on either side of byte 2^31 and 2^32", "conv",
           cfg=_cfg, b=2, h=182, w=182, cin=16, n=32, lda=WIDE_LD, **_g)
_LDA_TAP = tap_limit_lda(3, 3, 16, 16)
for _cfg in (70, -1):
    _c("wd_conv_gemm_split", f"tap offset just below 2^31 cfg{_cfg}", "a (filter tap offset)", "8 x 16 map, last tap (2 * 16 + 2) * lda * 4 + 64 <= 2^31",
       "conv", cfg=_cfg, b=1, h=8, w=16, cin=16, n=32, lda=_LDA_TAP, kh=3, stride=1, pad=1, tap=True)
for _cfg in (-1, 70, 77):
    _r("wd_conv_gemm_split", f"tap offset past 2^31 cfg{_cfg}", "a (filter tap offset)", "the same map, lda one group of 8 wider", "tap_limit",
       UNSUPPORTED, cfg=_cfg, h=8, w=16, cin=16, n=32, lda=_LDA_TAP + 8, lda_in=_LDA_TAP, kh=3)

# ---- 5. LayerNorm rows
for _entry in ("wd_layernorm_rows", "wd_layernorm_rows_split"):
    for _rows in (M_BIG, 65535):
        for _cc in (128, 512):
            for _op in ("x", "y"):
                _c(_entry, f"{_op} wide rows{_rows} c{_cc}", f"{_op} (ld{_op})", B31_32 + (" (four rows per lane group)" if _rows >= 65536 and _cc <= 256 else ""),
                   "layernorm", rows=_rows, c=_cc, wide=_op, split=_entry.endswith("split"))
_c("wd_layernorm_rows_split_s2d", "dense 2 x 1026 x 1024 c512", "x and y (dense: ldy = 4 c is fixed by the entry)", "pixels and space-to-depth rows on either side of byte 2^31 and 2^32",
   "layernorm_s2d", b=2, h=1026, w=1024, c=512)

# ---- 6. depthwise family: dense NHWC, real 4 GiB tensors
#      (a) the batch index crosses: 1040 images of 32 x 32 x 1024 (4 MiB each: images 512 and 1024 start at byte 2^31 and 2^32)
for _mode, _entry in (("variant1", "wd_dwconv7_variant"), ("variant2", "wd_dwconv7_variant"), ("variant4", "wd_dwconv7_variant"),
                      ("production", "wd_dwconv7"), ("ln", "wd_dwconv7_ln"), ("stats", "wd_dwconv7_stats")):
    _c(_entry, f"batch 1040 x 32 x 32 x 1024 {_mode}", "x and y (batch index)" + (", then wd_ln_stats_finalize" if _mode == "stats" else ""),
       "images on either side of byte 2^31 and 2^32", "dwconv_batch", mode=_mode, b=1040, h=32, w=32, c=1024)
#      (b) one image past the LDS-DMA form's own limit (h + 8) * w * c * 4 < 2^32: production takes the 1 x 4-strip LDS tile kernel
_c("wd_dwconv7", "one image 1032 x 1024 x 1024", "x and y (pixel rows of one image)", "pixel rows on either side of byte 2^31 and 2^32", "dwconv_image",
   h=1032, w=1024, c=1024)
_r("wd_dwconv7_variant", "variant 4 (h + 8) * w * c * 4 == 2^32", "x (staged window of the LDS-DMA form)", "h = 1016, w = c = 1024: exactly 2^32 bytes",
   "dwconv_limit", UNSUPPORTED, h=1016, h_in=1015, w=1024, c=1024)

# ---- 7. score entries on the 256 x 256 kernel
for _seg in ((32768 - 8, 32768 + 8), (0, 0)):
    _c("wd_similarity_split", f"ldo wide seg{_seg[0]}", "out (ldo)", B31_32 + "; seg boundaries on either side of row 32768", "similarity",
       rows=M_BIG, n_cls=264, dim=64, seg_rows=M_BIG if _seg[0] else 8224, seg_ends=_seg if _seg[0] else (6000, 7800))
_CLS_MAX = (1 << 31) - 1
for _entry, _ncls in (("wd_best_similarity_split", 264), ("wd_topn_similarity_split", 264), ("wd_group_similarity_split", 256)):
    _off = (_CLS_MAX - _ncls) // 32 * 32
    _c(_entry, "cls_offset near 2^31", "cls_offset + n_cls", f"cls_offset = {_off}: the last class index is just below 2^31", "fused",
       rows=520, n_cls=_ncls, dim=64, cls_offset=_off)
    _bad = _CLS_MAX - _ncls + 1 if "group" not in _entry else (_CLS_MAX - _ncls) // 32 * 32 + 32
    _r(_entry, "cls_offset + n_cls past 2^31 - 1", "cls_offset + n_cls", "one unit past 2^31 - 1", "cls_limit", BAD_ARG, n_cls=_ncls, dim=64,
       cls_offset=_bad, cls_in=_CLS_MAX - _ncls if "group" not in _entry else _off)
_c("wd_group_similarity_split", "out wide", "out ([rows][G], ldo wide)", B31_32, "fused", rows=M_BIG, n_cls=256, dim=64, cls_offset=0, ldo=WIDE_LD)
_c("wd_sparse_similarity_split", "flat index near 2^31", "rows_per_img * n_cls_total", "the last flat index anchor * n_cls_total + class is just below 2^31",
   "fused", rows=520, n_cls=264, dim=64, rows_per_img=520, n_cls_total=((1 << 31) - 1) // 520)
_r("wd_sparse_similarity_split", "flat index past 2^31", "rows_per_img * n_cls_total", "rows_per_img * n_cls_total >= 2^31", "sparse_limit",
   UNSUPPORTED, rows_per_img=520, n_cls_total=((1 << 31) + 519) // 520, total_in=((1 << 31) - 1) // 520)
for _entry in ("wd_best_similarity_split", "wd_topn_similarity_split", "wd_group_similarity_split", "wd_sparse_similarity_split"):
    for _dim in (768, 1024):
        _r(_entry, f"bank past 2^32 dim{_dim}", "t_split (n_cls * dim * 4)", "round_up(n_cls, 8) * dim * 4 >= 2^32", "bank_limit", UNSUPPORTED, dim=_dim)

# ---- 8. wd_retrieval_max_split: the seams of the chunk loop
_c("wd_retrieval_max_split", "dim1024 2^20+8", "t_split, out + c0", "the shape a fixed 2^20 chunk overran: seam at class chunk(1024), bank across 2^32",
   "retrieval", dim=1024, n_cls=(1 << 20) + 8)
_c("wd_retrieval_max_split", "dim4096 chunk+40", "t_split, out + c0", "seam inside a bank that crosses byte 2^32", "retrieval", dim=4096,
   n_cls=retrieval_chunk(4096) + 40)
_c("wd_retrieval_max_split", "dim64 2*chunk+8", "t_split, out + c0", "two seams where the 2^20 cap is the chunk", "retrieval", dim=64,
   n_cls=2 * retrieval_chunk(64) + 8)

# ---- 9. wd_topk_candidates: batch * n past 2^31 elements
_c("wd_topk_candidates", "5 x (2^29 + 256)", "scores (batch * n_per_image elements)", "elements on either side of element 2^30, 2^31 and 2^31 + 2^29",
   "topk", batch=5, n=(1 << 29) + 256, nms_pre=1000, thr=0.001)


# Entry points with a stride, row-count or class-offset parameter that no row above names: one line each.
EXEMPT: Dict[str, str] = {
    "wd_conv_gemm_tuned": "diagnostic tiles of wd_conv_gemm's kernel template (same loader and epilogue code); not on the product path",
    "wd_mlp_fused_split": "not covered: dense [rows][128] operands pass 2^32 bytes only from 8.4 M rows; rows / 128 tiles are refused past 2^31",
    "wd_mlp_fused_wide": "not covered: dense [rows][c] operands, c <= 512, pass 2^32 bytes only from 2.1 M rows",
    "wd_mlp_fused_wide_ln": "not covered: dense [rows][256] operands pass 2^32 bytes only from 4.2 M rows",
    "wd_ln_stats_finalize": "no row of its own: it runs inside the wd_dwconv7_stats row (1 064 960 rows, every image against a batch slice)",
    "wd_retrieval_max": "fp32 form, rows_per_img <= 320 and one workgroup per (64 classes, image); out index 64-bit by reading (conv_gemm.hip:293)",
    "wd_similarity_grouped": "per-image banks [n_img][k_max][768]: bounded by the detector's k_max (thousands); not covered",
    "wd_attention_small": "text tower: seq_len <= 64, operands of a few MB",
    "wd_max_sigmoid_attn": "bricks of the neck: feature maps of one step, far below 2^31 bytes",
    "wd_adaptive_maxpool_nhwc": "bricks of the neck: feature maps of one step, far below 2^31 bytes",
    "wd_cross_attention_small": "bricks of the neck: n_k <= 64 keys, operands of a few MB",
    "wd_l2norm_rows": "not covered: dense [rows][768] banks pass 2^32 bytes from 1.4 M rows; row index is long long by reading (elementwise.hip, l2norm_rows_kernel)",
    "wd_dfl_decode": "head maps of one step (at most 80 x 80 anchors per image); 'stride' is the anchor stride in pixels",
    "wd_nms_gather": "not covered, 64-bit by reading: candidate rows (postprocess.hip:465-471) and the embedding gather at B >= 167 (postprocess.hip:563, 566)",
    "wd_nms_gather_labeled": "the same kernels as wd_nms_gather (postprocess.hip:465-471, 485)",
    "wd_best_rows": "reads a materialised [rows][ld] block of at most ROWS_CHUNK columns; cls_offset limit shared with wd_best_similarity_split (best.hip:67)",
    "wd_best_unpack": "[rows] keys, 8 bytes each: 2^32 bytes only from 537 M rows; rows is refused past 2^31 - 16",
    "wd_topn_rows": "reads a materialised [rows][ld] block; cls_offset limit shared with wd_topn_similarity_split (topn.hip:85)",
    "wd_topn_unpack": "[rows][n_top] keys: rows * n_top is refused past 2^31 - 16",
    "wd_group_rows": "reads a materialised [rows][ld] block; cls_offset limit shared with wd_group_similarity_split (groups.hip:44)",
    "wd_sparse_rows": "reads a materialised [rows][ld] block; the flat-index limit is the one of wd_sparse_similarity_split (sparse.hip:159)",
}

# Headers outside the coverage condition: their operands are bounded by their own arguments, far below 2^31 bytes.
EXEMPT_HEADERS: Dict[str, str] = {
    "wedetect_hip_feed.h": "decoded images and canvases of one batch: bounded by the feed's max_in pixels per image",
    "wedetect_hip_tile.h": "tiles of one image and merge lists of n_tile * max_in candidates (n_tile <= 128)",
    "wedetect_hip_views.h": "views of one image (at most a handful) and their candidate lists",
    "wedetect_hip_track.h": "track state of n_seq * max_tracks slots (max_tracks <= 256), refused past 2^31 elements",
    "wedetect_hip_tune.h": "bank slabs of n_split * K_pad * dim floats for a few thousand classes",
    "wedetect_hip_exemplar.h": "example slots of batch * max_ex * m anchors",
    "wedetect_hip_fold.h": "one level of the folded head: the implicit-GEMM kernel of wd_conv_gemm_split, covered there",
}
