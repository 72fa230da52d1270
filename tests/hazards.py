"""Happens-before checker for the cross-stream schedules of wedetect_amd (plain Python, no device code).

``track()`` records, while it is active, what every launch reads and writes and on which stream — the HIP wrappers through the
``ACCESS`` table below, torch's own device work through a ``TorchDispatchMode`` — rebuilds the happens-before order from the
``Event`` / ``Stream`` calls the code under test really makes (one vector clock per stream) and reports every pair of
conflicting accesses on different streams that no chain of record / wait / synchronise orders.  Nothing depends on timing:
the answer is the same on an idle and on a loaded chip, at the smallest shapes.  The tracker only observes — every real
method is called with the caller's arguments — so nothing that reaches the device changes.

What it does not see: host writes into pinned memory, buffers a kernel owns that are not arguments (the zero page of the
LDS-DMA loaders), and allocator reuse (every tensor seen is held until the context exits, so an address means one buffer).

``Model`` is the device-free core (clocks, accesses, intersection); tests/test_cpu_hazards.py drives it with fake streams.
"""
from __future__ import annotations

import bisect
import contextlib
import inspect
import sys
from collections import namedtuple
from types import SimpleNamespace

R, W, A = "R", "W", "A"          # read, write, atomic / commutative (see BENIGN)

# ---------------------------------------------------------------------------------------------------------------------
# strided rectangles of bytes: (base, rows, stride, width) = rows runs of ``width`` bytes, ``stride`` bytes apart
# ---------------------------------------------------------------------------------------------------------------------


def normalise(acc):
    """One access tuple (mode, base, rows, row_stride_bytes, row_bytes[, batch, batch_stride_bytes]) -> a list of
    (mode, base, rows, stride, width) with the batch expanded, dense rows merged into one run and empty ones dropped."""
    mode, base, rows, stride, width = acc[:5]
    batch, bstride = (acc[5], acc[6]) if len(acc) > 5 else (1, 0)
    base, rows, stride, width, batch, bstride = int(base), int(rows), int(stride), int(width), int(batch), int(bstride)
    if rows <= 0 or width <= 0 or batch <= 0 or base == 0:
        return []
    if rows == 1 or width >= stride:                      # dense (or overlapping) rows: one run
        width, rows, stride = (rows - 1) * stride + width, 1, 0
    if batch > 1 and rows == 1 and bstride > 0:           # a batch of single runs is itself a rectangle
        return normalise((mode, base, batch, bstride, width))
    return [(mode, base + b * bstride, rows, stride if rows > 1 else width, width) for b in range(batch)]


def _run_hits_rect(p, length, b0, rb, s, wb):
    """Does the run [p, p + length) meet a row of the rectangle (b0, rb, s, wb)?  Exact."""
    jmin = max(0, (p - b0 - wb) // s + 1)
    jmax = min(rb - 1, -((b0 - p - length) // s) - 1)
    return jmin <= jmax


def rects_intersect(x, y):
    """Do two normalised rectangles (base, rows, stride, width) share a byte?  Exact for a run against anything and for
    two rectangles of equal stride (column intervals modulo the stride, row intervals); bounding ranges otherwise."""
    a0, ra, sa, wa = x
    b0, rb, sb, wb = y
    if a0 + (ra - 1) * sa + wa <= b0 or b0 + (rb - 1) * sb + wb <= a0:
        return False
    if ra == 1 and rb == 1:
        return True
    if ra == 1:
        return _run_hits_rect(a0, wa, b0, rb, sb, wb)
    if rb == 1:
        return _run_hits_rect(b0, wb, a0, ra, sa, wa)
    if sa != sb:
        return True                                        # bounding ranges overlap: conservative
    s = sa
    q, r = divmod(b0 - a0, s)
    # byte i*s + x of A equals byte (q + j)*s + r + y of B: x - y - r is 0 or -s (widths are at most one stride)
    if r < wa and -rb < q < ra:
        return True
    if r > s - wb and -rb < q + 1 < ra:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------------
# the model: vector clocks, launches, hazards
# ---------------------------------------------------------------------------------------------------------------------
Hazard = namedtuple("Hazard", "buffer first second")         # first / second: "name@stream#ordinal mode"


def _join(into: dict, other: dict) -> None:
    for k, v in other.items():
        if into.get(k, 0) < v:
            into[k] = v


class Model:
    """Streams and events are any hashable keys.  ``bucket_of(address)`` groups addresses that can alias (a storage);
    ``label_of(lo, hi)`` names a byte range for the report; ``stream_label(key)`` names a stream."""

    def __init__(self, bucket_of=None, label_of=None, stream_label=None):
        self.clock = {}                  # stream -> {stream: ticks}
        self.host = {}                   # what the host has waited for
        self.events = {}                 # event -> snapshot
        self.launches = []               # (name, stream, tick, clock copy)
        self.buckets = {}                # bucket -> {"W": [...], "A": [...], "R": [...]} of (launch index, base, rows, stride, width)
        self.bucket_of = bucket_of or (lambda addr: 0)
        self.label_of = label_of or (lambda lo, hi: hex(lo))
        self.stream_label = stream_label or (lambda s: str(s))

    def _clk(self, stream) -> dict:
        c = self.clock.setdefault(stream, {})
        _join(c, self.host)              # everything the host waited for precedes whatever it issues next
        return c

    def launch(self, stream, name, accesses) -> int:
        c = self._clk(stream)
        c[stream] = c.get(stream, 0) + 1
        idx = len(self.launches)
        self.launches.append((name, stream, c[stream], dict(c)))
        for acc in accesses:
            for mode, base, rows, stride, width in normalise(acc):
                self.buckets.setdefault(self.bucket_of(base), {W: [], A: [], R: []})[mode].append((idx, base, rows, stride, width))
        return idx

    def record(self, event, stream) -> None:
        self.events[event] = dict(self._clk(stream))          # a later record replaces the snapshot

    def wait(self, event, stream, ignored: bool = False) -> None:
        snap = self.events.get(event)                          # never recorded: adds nothing
        if snap is not None and not ignored:
            _join(self._clk(stream), snap)

    def wait_stream(self, stream, other) -> None:
        _join(self._clk(stream), self._clk(other))

    def host_sync(self, stream=None, event=None) -> None:
        """The host waits for one stream, for an event's snapshot, or (neither given) for every stream."""
        if event is not None:
            _join(self.host, self.events.get(event) or {})
        elif stream is not None:
            _join(self.host, self.clock.get(stream, {}))
        else:
            for c in self.clock.values():
                _join(self.host, c)

    def _ordered(self, i: int, j: int) -> bool:
        """Same stream, or the earlier-issued launch happens before the later one."""
        if i > j:
            i, j = j, i
        _, si, ti, _ = self.launches[i]
        _, sj, _, cj = self.launches[j]
        return si == sj or cj.get(si, 0) >= ti

    def _describe(self, idx: int, mode: str) -> str:
        name, stream, _, _ = self.launches[idx]
        return f"{name}@{self.stream_label(stream)}#{idx} {mode}"

    def hazards(self):
        """Every pair of launches on different streams with intersecting byte sets, at least one of them a write (A / A
        is fine, A / R and A / W are not), neither ordered before the other.  One entry per (launch pair, modes)."""
        out, seen = [], set()

        def scan(xs, mx, ys, my, same):
            for n, x in enumerate(xs):
                xlo, xhi = x[1], x[1] + (x[2] - 1) * x[3] + x[4]
                for y in (ys[n + 1:] if same else ys):
                    if y[1] >= xhi or y[1] + (y[2] - 1) * y[3] + y[4] <= xlo or x[0] == y[0]:
                        continue
                    if self._ordered(x[0], y[0]) or not rects_intersect(x[1:], y[1:]):
                        continue
                    first, second = ((x, mx), (y, my)) if x[0] < y[0] else ((y, my), (x, mx))
                    key = (first[0][0], second[0][0], first[1], second[1])
                    if key in seen:
                        continue
                    seen.add(key)
                    lo = max(xlo, y[1])
                    hi = min(xhi, y[1] + (y[2] - 1) * y[3] + y[4])
                    out.append(Hazard(self.label_of(lo, hi), self._describe(first[0][0], first[1]),
                                      self._describe(second[0][0], second[1])))

        for b in self.buckets.values():
            scan(b[W], W, b[W], W, True)
            scan(b[W], W, b[R], R, False)
            scan(b[W], W, b[A], A, False)
            scan(b[A], A, b[R], R, False)
        return out


def format_hazards(hz, limit: int = 12) -> str:
    lines = [f"{len(hz)} unordered conflicting pair(s)"]
    for h in hz[:limit]:
        lines.append(f"  {h.buffer}: {h.first}  ||  {h.second}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# the ACCESS table: wrapper -> what the launch touches, from its scalar arguments (include/wedetect_hip*.h, "Extents:")
# ---------------------------------------------------------------------------------------------------------------------
def _run(mode, t, nbytes, off=0):
    return None if t is None else (mode, t.data_ptr() + off, 1, nbytes, nbytes)


def _rect(mode, t, rows, stride, width, batch=1, bstride=0):
    return None if t is None else (mode, t.data_ptr(), rows, stride, width, batch, bstride)


def _whole(mode, t):
    return None if t is None else (mode, t.data_ptr(), 1, t.numel() * t.element_size(), t.numel() * t.element_size())


def _up8(n):
    return (n + 7) // 8 * 8


def _gemm_out(mode, t, a, ld, m, hw):
    """Output addressing of WdConvGemm: plain rows, per-image row map (c_batch_stride) or the 2 x 2 scatter."""
    if a.out_mode == 1:                                   # WD_OUT_DECONV2X2: 4 m output pixels of n / 4 channels
        return _rect(mode, t, 4 * m, ld * 4, a.n)
    if a.c_batch_stride:
        return _rect(mode, t, hw, ld * 4, a.n * 4, a.batch, a.c_batch_stride * ld * 4)
    return _rect(mode, t, m, ld * 4, a.n * 4)


def _conv_gemm(a, ret):
    hout = (a.hin + 2 * a.pad - a.kh) // a.stride + 1 if a.hout is None else a.hout
    wout = (a.win + 2 * a.pad - a.kw) // a.stride + 1 if a.wout is None else a.wout
    m, k = a.batch * hout * wout, a.kh * a.kw * a.cin
    acc = [_rect(R, a.a, a.batch * a.hin * a.win, a.lda * 4, a.cin * 4),
           _whole(R, a.w_split[0]) if a.w_split is not None else _run(R, a.w, a.n * k * 4),
           _run(R, a.bias, a.n * 4),
           _rect(R, a.res, m, a.ldres * 4, a.n * 4),
           _gemm_out(W, a.c, a, a.ldc, m, hout * wout),
           _gemm_out(W, a.c2, a, a.ldc2, m, hout * wout) if a.out_mode == 0 else None,
           _run(R, a.ln_stats, m * 8), _run(R, a.ln_u, a.n * 4),
           _whole(W, a.workspace) if a.w_split is not None else None,      # partial sums / parked accumulators: read and written
           _run(A, a.range_flag, 4) if a.w_split is not None else None]
    return acc


def _mlp(a, ret, w1, w2, extra):
    return [_run(R, extra[0], a.rows * a.c * 4), _whole(R, w1[0]), _whole(R, w2[0]), _run(R, a.b2, a.c * 4),
            _run(W, a.x, a.rows * a.c * 4), _run(A, a.range_flag, 4), _whole(W, getattr(a, "workspace", None))] + extra[1:]


def _fold_similarity(a, ret):
    return [_rect(R, a.c2_split, a.batch * a.rows, a.cin * 4, a.cin * 4), _run(R, a.w_split, _up8(a.n) * a.cin * 4),
            _run(R, a.unscale_dev, 4), _run(R, a.bias, _up8(a.n) * 4),
            _rect(W, a.out, a.rows, a.n * 4, a.n * 4, a.batch, a.c_batch_stride * a.n * 4), _run(A, a.range_flag, 4)]


def _split_weights(a, ret):
    n, k = a.w.shape
    return [_run(R, a.w, n * k * 4) if a.w.is_contiguous() else None, None if ret is None else _whole(W, ret[0])]


def _split_weights_scaled(a, ret):
    from wedetect_amd import lib as L
    n, k = a.w.shape
    return [_run(R, a.w, n * k * 4) if a.w.is_contiguous() else None, _run(W, a.out, int(L.LIB.wd_split_weights_bytes(n, k)))]


def _dwconv(a, ret, out, extra=()):
    n = a.batch * a.h * a.w * a.c * 4
    return [_run(R, a.x, n), _run(R, a.w7, 49 * a.c * 4), _run(R, a.bias, a.c * 4), _run(W, out, n), *extra]


def _nms_gather(a, ret):
    b, mo = a.batch, a.max_out
    return [_run(R, a.cand_idx, b * a.cand_stride * 4), _run(R, a.cand_score, b * a.cand_stride * 4), _run(R, a.cand_count, b * 4),
            _run(R, a.boxes, b * a.n_anchor * 16), _run(R, a.meta, b * 32), _run(R, a.embed, b * a.n_anchor * a.embed_dim * 4),
            _run(W, a.out_boxes, b * mo * 16), _run(W, a.out_scores, b * mo * 4), _run(W, a.out_labels, b * mo * 4),
            _run(W, a.out_anchors, b * mo * 4), _run(W, a.out_count, b * 4), _run(W, a.out_embed, b * mo * a.embed_dim * 4),
            _whole(W, a.workspace)]


def _topk(a, ret):
    from wedetect_amd import lib as L
    cap = L.topk_capacity(a.nms_pre)
    return [_run(R, a.scores, a.batch * a.n * 4), _run(W, a.out_idx, a.batch * cap * 4), _run(W, a.out_score, a.batch * cap * 4),
            _run(W, a.out_count, a.batch * 4), _whole(W, a.workspace)]


def _kept_reorder(a, ret):
    b, mo = a.batch, a.max_out
    return [_run(R, a.level_scores, 3 * b * mo * a.k * 4), _run(W, a.out_boxes, b * mo * 16), _run(W, a.out_scores, b * mo * 4),
            _run(W, a.out_labels, b * mo * 4), _run(W, a.out_anchors, b * mo * 4), _run(R, a.out_count, b * 4), _run(W, a.perm, b * mo * 4)]


def _merge(a, n_in, plan_ptr, plan_bytes, n_img=1):
    """wd_tile_merge / wd_views_merge: n_in stacked (tile | view x image) row sets in, n_img merged lists out."""
    rows_in, rows_out = n_in * a.max_in, n_img * a.max_out
    return [_run(R, a.boxes, rows_in * 16), _run(R, a.scores, rows_in * 4), _run(R, a.labels, rows_in * 4), _run(R, a.counts, n_in * 4),
            (R, plan_ptr, 1, plan_bytes, plan_bytes), _run(W, a.out_boxes, rows_out * 16), _run(W, a.out_scores, rows_out * 4),
            _run(W, a.out_labels, rows_out * 4), _run(W, a.out_src, rows_out * 4), _run(W, a.out_count, n_img * 4), _whole(W, a.workspace)]


ACCESS = {
    "lib.conv_gemm": _conv_gemm,
    "lib.mlp_fused": lambda a, r: _mlp(a, r, a.w1_split, a.w2_split, [a.a_split, _run(R, a.b1, a.hidden * 4)]),
    "lib.mlp_fused_wide": lambda a, r: _mlp(a, r, a.w1_frag, a.w2_frag, [a.a_split, _run(R, a.b1, a.hidden * 4)]),
    "lib.mlp_fused_wide_ln": lambda a, r: _mlp(a, r, a.w1g_frag, a.w2_frag, [a.d_split, _run(R, a.v, a.hidden * 4), _run(R, a.u, a.hidden * 4),
                                                                              _run(R, a.ln_stats, a.rows * 8)]),
    "lib.split_weights": _split_weights,
    "lib.split_weights_scaled": _split_weights_scaled,
    "lib.stem_patchify": lambda a, r: [_whole(R, a.img_u8), _run(W, a.out, a.img_u8.numel() // 3 * 12)],
    "lib.stem_fused": lambda a, r: [_whole(R, a.img_u8), _whole(R, a.wgt), _whole(R, a.bias), _whole(R, a.gamma), _whole(R, a.beta),
                                    _run(W, a.out, a.img_u8.numel() // 48 * a.wgt.shape[0] * 4)],
    "lib.dwconv7": lambda a, r: _dwconv(a, r, a.y),
    "lib.dwconv7_ln": lambda a, r: _dwconv(a, r, a.y, (_run(R, a.gamma, a.c * 4), _run(R, a.beta, a.c * 4))),
    "lib.dwconv7_stats": lambda a, r: _dwconv(a, r, a.y_split, (_run(W, a.part, a.c // 32 * a.batch * a.h * a.w * 8),)),
    "lib.ln_stats_finalize": lambda a, r: [_run(R, a.part, a.c // 32 * a.rows * 8), _run(W, a.stats, a.rows * 8)],
    "lib.layernorm_rows": lambda a, r: [_rect(R, a.x, a.rows, (a.ldx or a.c) * 4, a.c * 4), _rect(W, a.y, a.rows, (a.ldy or a.c) * 4, a.c * 4),
                                        _run(R, a.gamma, a.c * 4), _run(R, a.beta, a.c * 4)],
    "lib.layernorm_rows_split_s2d": lambda a, r: [_run(R, a.x, a.batch * a.h * a.w * a.c * 4), _run(W, a.y, a.batch * a.h * a.w * a.c * 4),
                                                  _run(R, a.gamma, a.c * 4), _run(R, a.beta, a.c * 4)],
    "lib.l2norm_rows": lambda a, r: [_run(R, a.x, a.x.shape[0] * a.x.shape[1] * 4), _run(W, a.y, a.x.shape[0] * a.x.shape[1] * 4)],
    "lib.dfl_decode": lambda a, r: [_rect(R, a.dist, a.batch * a.hl * a.wl, a.ld * 4, 256),
                                    (W, a.boxes.data_ptr() + a.anchor_off * 16, 1, a.hl * a.wl * 16, a.hl * a.wl * 16, a.batch, a.anchors_total * 16)],
    "lib.topk_candidates": _topk,
    "lib.nms_gather": _nms_gather,
    "lib.similarity_split": lambda a, r: [_run(R, a.e_split, _up8(a.rows) * a.dim * 4), _whole(R, a.t_split), _rect(W, a.out, a.rows, a.ldo * 4, a.n_cls * 4),
                                          _run(A, a.range_flag, 4)],
    "lib.similarity_grouped": lambda a, r: [_run(R, a.embed, a.n_img * a.rows_per_img * a.dim * 4), _run(R, a.bank, a.n_img * a.k_max * a.dim * 4),
                                            _run(R, a.count, a.n_img * 4), _rect(W, a.out, a.n_img * a.rows_per_img, a.ldo * 4, a.k_max * 4)],
    "lib.chw_to_hwc_u8": lambda a, r: [_whole(R, a.src), _whole(W, a.dst)],
    "lib.cv_resize_paste_u8": lambda a, r: [_run(R, a.src, a.sh * a.sw * 3), *(_whole(R, t) for t in (a.xa, a.xidx, a.xw, a.ya, a.yidx, a.yw)),
                                            _run(W, a.dst, a.dst_h * a.dst_w * 3)],
    "feed.feed_batch_u8": lambda a, r: [_whole(R, a.src), (R, a.images_dev_ptr, 1, a.images_host.nbytes, a.images_host.nbytes),
                                        (R, a.tables_dev_ptr, 1, a.table_elems * 4, a.table_elems * 4), _whole(W, a.tmp), _whole(W, a.dst)],
    "tile.tile_cut_u8": lambda a, r: [_rect(R, a.img, a.img.shape[0], a.img.stride(0), a.img.shape[1] * 3),
                                      (R, a.plan_dev_ptr, 1, a.plan_host.nbytes, a.plan_host.nbytes), _whole(W, a.dst)],
    "tile.tile_merge": lambda a, r: _merge(a, a.n_tile, a.plan_dev_ptr, a.n_tile * 32),
    "views.flip_u8": lambda a, r: [_whole(R, a.src), _whole(W, a.dst)],
    "views.views_merge": lambda a, r: _merge(a, a.n_view * a.batch, 0, 0, a.batch) + [_run(R, a.view_flip, a.n_view * 4), _run(R, a.img_wh, a.batch * 8)],
    "fold.fold_similarity": _fold_similarity,
    "fold.kept_rows_gather": lambda a, r: [*(_run(R, a.c2[l], a.batch * a.rows[l] * a.row_floats * 4) for l in range(3)),
                                           _run(R, a.out_anchors, a.batch * a.max_out * 4), _run(R, a.out_count, a.batch * 4),
                                           _run(W, a.gathered, 3 * a.batch * a.max_out * a.row_floats * 4)],
    "fold.kept_rows_select": lambda a, r: [_run(R, a.level_embed, 3 * a.batch * a.max_out * a.dim * 4), _run(R, a.out_anchors, a.batch * a.max_out * 4),
                                           _run(R, a.out_count, a.batch * 4), _run(R, a.perm, a.batch * a.max_out * 4),
                                           _run(W, a.out_embed, a.batch * a.max_out * a.dim * 4)],
    "fold.kept_rows_reorder": _kept_reorder,
}

# (wrapper, argument) pairs classed A above, each with the kernel source line that makes the access commutative: a sticky
# word that only ever receives a plain store of the constant 1 (any order, any number of times, the same bytes; nothing in a
# kernel reads it).  Nothing else may be A.
BENIGN = [
    ("lib.conv_gemm", "range_flag", "csrc/split_gemm_impl.h:106, 232, 316, 430 and csrc/split_epi_oct.h:25 — `if (non-finite) *p.range_flag = 1u;`, csrc/split_gemm_p8.hip:157 — `if (bad) *p.range_flag = 1u;`"),
    ("lib.mlp_fused", "range_flag", "csrc/split_gemm_mlp.hip:236 — `pe.range_flag = q.range_flag`: the epilogues of split_gemm_impl.h above"),
    ("lib.mlp_fused_wide", "range_flag", "csrc/split_gemm_mlpw.hip:581 — `pe.range_flag = q.range_flag`: the epilogues of split_gemm_impl.h above"),
    ("lib.mlp_fused_wide_ln", "range_flag", "csrc/split_gemm_mlpw.hip:581 — the same launcher"),
    ("lib.similarity_split", "range_flag", "csrc/split_gemm_impl.h:106 — `if (non-finite) *p.range_flag = 1u;` in epi_quad, the storing epilogue of wd_launch_p8_similarity"),
    ("fold.fold_similarity", "range_flag", "wd_conv_gemm_split's implicit-GEMM kernel: the epilogues of split_gemm_impl.h / split_epi_oct.h above"),
]

# Functions of wedetect_amd that call stream_ptr() and have no ACCESS entry: not reachable from the schedules tracked here.
# Reaching one inside track() raises "untracked launch" (they are not wrapped), so the list cannot hide a launch.
EXEMPT = {
    "lib.retrieval_max": "retrieval evaluator, not reachable from a detect step",
    "lib.retrieval_max_split": "retrieval evaluator, not reachable from a detect step",
    "lib.text_embed": "text tower, runs before any detect step",
    "lib.attention_small": "text tower, runs before any detect step",
    "lib.max_sigmoid_attn": "text-guided bricks, not part of the image tower",
    "lib.adaptive_maxpool_nhwc": "text-guided bricks, not part of the image tower",
    "lib.cross_attention_small": "text-guided bricks, not part of the image tower",
    "lib.letterbox_u8": "per-image preprocessing of the detectors, one stream, ahead of the tower",
    "evaluate.matched_ious": "proposal-recall evaluator, not reachable from a detect step",
    "det_eval._device_eval": "evaluator, not reachable from a detect step",
}


# ---------------------------------------------------------------------------------------------------------------------
# track(): the model fed by the real calls
# ---------------------------------------------------------------------------------------------------------------------
class Tracker:
    def __init__(self, names=None, stream_names=None, ignore_wait=None, audit=False):
        self.names, self.stream_names, self.ignore_wait, self.audit = names, stream_names, ignore_wait, audit
        self.model = Model(self._bucket_of, self._label_of, self._stream_label)
        self.inside = 0                       # depth of recording wrappers on the stack (lib.stream_ptr guard)
        self.held = []                        # every tensor / event seen: addresses and ids stay meaningful
        self.starts, self.stores = [], {}     # sorted storage start addresses -> (end, byte view)
        self.seen_storages = set()
        self.calls = {}                       # wrapper -> launches recorded
        self.ignored_waits = 0
        self.mismatches = []                  # audit mode: (wrapper, ordinal, operand address, first changed byte)
        self.audited = 0

    # ---- storages
    def hold(self, t) -> None:
        import torch
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            return
        st = t.untyped_storage()
        p = st.data_ptr()
        if p == 0 or p in self.seen_storages:
            return
        self.seen_storages.add(p)
        self.held.append(t)
        view = torch.empty(0, dtype=torch.uint8, device=t.device).set_(st) if self.audit else None
        bisect.insort(self.starts, p)
        self.stores[p] = (p + st.nbytes(), view)

    def _hold_tree(self, v) -> None:
        import torch
        if isinstance(v, torch.Tensor):
            self.hold(v)
        elif isinstance(v, (list, tuple)):
            for e in v:
                self._hold_tree(e)
        elif isinstance(v, dict):
            for e in v.values():
                self._hold_tree(e)

    def _bucket_of(self, addr):
        i = bisect.bisect_right(self.starts, addr) - 1
        if i >= 0 and addr < self.stores[self.starts[i]][0]:
            return self.starts[i]
        # a raw-pointer operand (plan_dev_ptr, tables_dev_ptr) over memory no tensor was seen for would land in a bucket of
        # its own and its conflicts would be missed silently
        raise RuntimeError(f"access at {addr:#x} belongs to no tensor seen so far")

    def _label_of(self, lo, hi):
        names = self.names() if callable(self.names) else (self.names or {})
        hits = []
        for label, t in names.items():
            if t is None:
                continue
            p = t.data_ptr()
            ext = (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size() if t.numel() else 0
            if p < hi and lo < p + ext:
                hits.append(label)
        return "/".join(hits) if hits else hex(lo)

    def _stream_label(self, key):
        names = self.stream_names() if callable(self.stream_names) else (self.stream_names or {})
        for label, s in names.items():
            if s is not None and s.cuda_stream == key:
                return label
        return "default" if key == 0 else f"stream{key:#x}"

    def hazards(self):
        return self.model.hazards()

    # ---- audit: what a launch really changed against what ACCESS declares
    def _audit_call(self, name, accs, real, args, kwargs):
        """Snapshots the WHOLE storage of every tensor passed to the launch and of every declared rectangle, so that a write
        past an under-declared extent, or into an operand the entry leaves out, shows as a changed byte outside the
        rectangles declared written."""
        import torch
        rects = [r for acc in accs for r in normalise(acc)]
        groups, passed = {}, []

        def walk(v):
            if isinstance(v, torch.Tensor):
                if v.device.type == "cuda" and v.untyped_storage().data_ptr():
                    passed.append(v.untyped_storage().data_ptr())
            elif isinstance(v, (list, tuple)):
                for e in v:
                    walk(e)
        walk(args)
        walk(list(kwargs.values()))
        for b in passed:
            groups.setdefault(b, [b, self.stores[b][0], []])
        for mode, base, rows, stride, width in rects:
            b = self._bucket_of(base)
            if b not in self.stores:
                raise RuntimeError(f"audit: {name} touches {base:#x}, which belongs to no tensor seen")
            g = groups.setdefault(b, [b, self.stores[b][0], []])
            hi = base + (rows - 1) * stride + width
            if hi > self.stores[b][0]:
                raise RuntimeError(f"audit: {name} declares bytes up to {hi:#x}, past the end of the buffer at {b:#x}")
            g[2].append((mode, base, rows, stride, width))
        torch.cuda.synchronize()
        before = {b: self.stores[b][1][lo - b: hi - b].clone() for b, (lo, hi, _) in groups.items()}
        ret = real(*args, **kwargs)
        torch.cuda.synchronize()
        for b, (lo, hi, rs) in groups.items():
            changed = self.stores[b][1][lo - b: hi - b] != before[b]
            for mode, base, rows, stride, width in rs:
                if mode != R:
                    changed[base - lo:].as_strided((rows, width), (stride, 1)).fill_(False)
            if bool(changed.any()):
                self.mismatches.append((name, self.audited, hex(lo), int(changed.nonzero()[0])))
        self.audited += 1
        return ret


def _arguments(real, args, kwargs):
    ba = inspect.signature(real).bind(*args, **kwargs)
    ba.apply_defaults()
    return SimpleNamespace(**ba.arguments)


HOST_READS = ("_local_scalar_dense", "equal", "is_nonzero", "item")
NO_DEVICE_WORK = ("record_stream", "empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "is_pinned", "detach", "alias")


def _tensor_access(mode, t):
    """A tensor's own extent: one run when it is dense, rows of its innermost dense dimensions under one outer stride when
    that describes it, the bounding range otherwise."""
    es = t.element_size()
    dims = [(s, st) for s, st in zip(t.shape, t.stride()) if s > 1]
    if t.numel() == 0:
        return None
    width, k = 1, len(dims)
    while k and dims[k - 1][1] == width:
        width *= dims[k - 1][0]
        k -= 1
    if k == 0:
        return (mode, t.data_ptr(), 1, width * es, width * es)
    if k == 1 and dims[0][1] > width:
        return (mode, t.data_ptr(), dims[0][0], dims[0][1] * es, width * es)
    ext = (sum((s - 1) * st for s, st in dims) + 1) * es
    return (mode, t.data_ptr(), 1, ext, ext)


@contextlib.contextmanager
def track(names=None, stream_names=None, ignore_wait=None, audit=False):
    """See the module docstring.  ``names`` / ``stream_names``: dicts (or callables returning dicts, evaluated when a report is
    written) label -> tensor / stream.  ``ignore_wait(event)``: leave the waits on such events out of the MODEL (the real
    wait is still issued).  ``audit=True``: no clocks — every wrapped launch is bracketed by device synchronisations and bit
    snapshots, and whatever changed outside the rectangles ACCESS declares written lands in ``Tracker.mismatches``."""
    import importlib

    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    tr = Tracker(names, stream_names, ignore_wait, audit)
    M = tr.model
    cur = lambda: torch.cuda.current_stream().cuda_stream
    mods = {m: importlib.import_module("wedetect_amd." + m) for m in sorted({k.split(".")[0] for k in ACCESS})}
    saved, benign = [], {w for w, _, _ in BENIGN}

    def patch(obj, attr, new):
        saved.append((obj, attr, getattr(obj, attr)))
        setattr(obj, attr, new)

    def wrap(key, real):
        def recording(*args, **kwargs):
            tr._hold_tree(args)
            tr._hold_tree(kwargs)
            a = _arguments(real, args, kwargs)
            tr.inside += 1
            try:
                if audit:
                    ret = tr._audit_call(key, [x for x in ACCESS[key](a, None) if x is not None], real, args, kwargs)
                else:
                    ret = real(*args, **kwargs)
            finally:
                tr.inside -= 1
            tr._hold_tree(ret)
            accs = [x for x in ACCESS[key](a, ret) if x is not None]
            if any(x[0] == A for x in accs) and key not in benign:
                raise RuntimeError(f"{key} classes an operand A without a BENIGN entry")
            if not audit:
                M.launch(cur(), key, accs)
            tr.calls[key] = tr.calls.get(key, 0) + 1
            return ret
        recording.__name__ = real.__name__
        return recording

    for key in ACCESS:
        m, f = key.split(".")
        patch(mods[m], f, wrap(key, getattr(mods[m], f)))
    real_ptr = mods["lib"].stream_ptr

    def guarded_stream_ptr():
        if not tr.inside:
            raise RuntimeError(f"untracked launch: {sys._getframe(1).f_code.co_name}")
        return real_ptr()
    patch(mods["lib"], "stream_ptr", guarded_stream_ptr)

    class Mode(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            kwargs = kwargs or {}
            out = func(*args, **kwargs)
            name = func._schema.name.split("::")[-1]
            if name in NO_DEVICE_WORK:
                return out
            ins, accs = [], []
            for i, arg in enumerate(func._schema.arguments):
                v = args[i] if i < len(args) else kwargs.get(arg.name)
                wr = arg.alias_info is not None and arg.alias_info.is_write
                for t in (v if isinstance(v, (list, tuple)) else (v,)):
                    if isinstance(t, torch.Tensor) and t.is_cuda:
                        ins.append(t)
                        accs.append(_tensor_access(W if wr else R, t))
            outs = [t for t in (out if isinstance(out, (list, tuple)) else (out,)) if isinstance(t, torch.Tensor)]
            if not ins and not any(t.is_cuda for t in outs):
                return out
            in_stores = {t.untyped_storage().data_ptr() for t in ins}
            fresh = [t for t in outs if t.is_cuda and t.untyped_storage().data_ptr() not in in_stores]
            wrote = any(a is not None and a[0] == W for a in accs)
            to_host = ins and (name in HOST_READS or any(not t.is_cuda for t in outs)
                               or (name == "copy_" and isinstance(args[0], torch.Tensor) and not args[0].is_cuda))
            if not fresh and not wrote and not to_host:
                return out                                 # a view: no device work
            for t in ins + fresh:
                tr.hold(t)
            accs += [_tensor_access(W, t) for t in fresh]
            M.launch(cur(), "aten." + name, [x for x in accs if x is not None])
            if to_host and not kwargs.get("non_blocking", False) and not (name == "copy_" and len(args) > 2 and args[2]):
                M.host_sync(stream=cur())                  # a blocking read: the host has waited for this stream
            return out

    E, S = torch.cuda.Event, torch.cuda.Stream
    real_record, real_wait, real_esync, real_ssync, real_sync = E.record, E.wait, E.synchronize, S.synchronize, torch.cuda.synchronize
    real_wait_event, real_wait_stream, real_record_event = S.wait_event, S.wait_stream, S.record_event

    def key_of(stream):
        return cur() if stream is None else stream.cuda_stream

    def record(self, stream=None):
        tr.held.append(self)
        M.record(id(self), key_of(stream))
        return real_record(self, stream)

    def wait(self, stream=None):
        tr.held.append(self)
        ign = bool(tr.ignore_wait and tr.ignore_wait(self))
        tr.ignored_waits += ign
        M.wait(id(self), key_of(stream), ignored=ign)
        return real_wait(self, stream)

    def esync(self):
        M.host_sync(event=id(self))
        return real_esync(self)

    def ssync(self):
        M.host_sync(stream=self.cuda_stream)
        return real_ssync(self)

    def sync(device=None):
        M.host_sync()
        return real_sync(device)

    # Stream.wait_event / wait_stream / record_event are Python that lands in Event.wait / Event.record (patched above);
    # they are patched too so that a torch that routes them elsewhere is still seen (the model's joins are idempotent)
    def wait_event(self, event):
        tr.held.append(event)
        ign = bool(tr.ignore_wait and tr.ignore_wait(event))
        M.wait(id(event), self.cuda_stream, ignored=ign)
        return real_wait_event(self, event)

    def wait_stream(self, stream):
        M.wait_stream(self.cuda_stream, stream.cuda_stream)
        return real_wait_stream(self, stream)

    def record_event(self, event=None):
        ev = real_record_event(self, event)
        tr.held.append(ev)
        M.record(id(ev), self.cuda_stream)
        return ev

    if not audit:
        for obj, attr, new in ((E, "record", record), (E, "wait", wait), (E, "synchronize", esync), (S, "synchronize", ssync),
                               (S, "wait_event", wait_event), (S, "wait_stream", wait_stream), (S, "record_event", record_event),
                               (torch.cuda, "synchronize", sync)):
            patch(obj, attr, new)
    try:
        with (contextlib.nullcontext() if audit else Mode()):
            yield tr
    finally:
        for obj, attr, old in reversed(saved):
            setattr(obj, attr, old)
