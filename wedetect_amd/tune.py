"""Bank tuning (include/wedetect_hip_tune.h, csrc/tune.hip): the rows of a class bank learned from labelled boxes with both towers
frozen.  ctypes binding of ``wd_tune_targets`` / ``wd_tune_grad`` / ``wd_tune_update`` / ``wd_tune_plan`` with a version and an
export list of its own, like exemplar.py (the main ABI stays as it is), and ``BankTuner``: region embeddings of the labelled
images cached once per batch, then one fused two-GEMM launch per cached chunk and one update launch per optimisation step."""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

from . import lib as L
from .lib import f32, i32, i64, vp

TUNE_ABI_VERSION = 1
DIM = 768                        # WD_TUNE_DIM
CLASS_BLOCK = 32                 # WD_TUNE_CLASS_BLOCK
ROW_TILE = 128                   # WD_TUNE_ROW_TILE
MAX_SPLIT = 256                  # WD_TUNE_MAX_SPLIT
BYTES_PER_ROW = DIM * 4 + 8      # a cached row: the embedding, pos_cls and pos_y

SIGNATURES = {
    "wd_tune_abi_version": (None, []),
    "wd_tune_plan": (i32, [i64, i32]),
    "wd_tune_targets": (None, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "wd_tune_grad": (None, [vp, i32, i32, i32, i32, i32, f32, f32, f32, f32, f32, f32, vp, vp, vp, i32, f32, i32, vp, vp, vp]),
    "wd_tune_update": (None, [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, f32, vp, i32, vp, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("tune", TUNE_ABI_VERSION, SIGNATURES)


def k_pad(n_cls: int) -> int:
    return -(-int(n_cls) // CLASS_BLOCK) * CLASS_BLOCK


def plan(rows: int, n_cls: int) -> int:
    """``wd_tune_plan``: the split count of ``tune_grad`` for a chunk of ``rows`` rows and ``n_cls`` classes (a pure function)."""
    s = int(LIB.wd_tune_plan(int(rows), int(n_cls)))
    if s < 1:
        raise ValueError(f"no plan for rows {rows}, classes {n_cls}: both must be positive")
    return s


def tune_targets(sel_anchors, sel_iou, ex_cls, max_ex: int, m: int, batch: int, n_anchor: int, pos_cls, pos_y) -> None:
    """``wd_tune_targets`` on the current stream: ``sel_anchors`` int32 / ``sel_iou`` fp32 [batch, max_ex * m] (wd_exemplar_assign),
    ``ex_cls`` int32 [batch, max_ex]; writes ``pos_cls`` int32 / ``pos_y`` fp32 [batch, n_anchor], whole."""
    L.check(LIB.wd_tune_targets(L.ptr(sel_anchors), L.ptr(sel_iou), L.ptr(ex_cls), int(max_ex), int(m), int(batch), int(n_anchor),
                                L.ptr(pos_cls), L.ptr(pos_y), L.stream_ptr()), "wd_tune_targets")


def tune_grad(embed, rows: int, n_anchor: int, off1: int, off2: int, scale, bias, pos_cls, pos_y, bank, n_cls: int, inv_norm: float,
              n_split: int, slabs, loss_parts, dim: int = DIM) -> None:
    """``wd_tune_grad`` on the current stream: one chunk ``embed`` fp32 [rows, 768] with ``pos_cls`` int32 / ``pos_y`` fp32 [rows],
    the three levels' ``scale`` / ``bias`` floats, ``bank`` fp32 [n_cls, 768] unit rows; writes ``slabs`` fp32
    [n_split, k_pad(n_cls), 768] and ``loss_parts`` fp32 [n_split, k_pad(n_cls) / 32], whole."""
    L.check(LIB.wd_tune_grad(L.ptr(embed), int(rows), int(dim), int(n_anchor), int(off1), int(off2), float(scale[0]), float(scale[1]),
                             float(scale[2]), float(bias[0]), float(bias[1]), float(bias[2]), L.ptr(pos_cls), L.ptr(pos_y), L.ptr(bank),
                             int(n_cls), float(inv_norm), int(n_split), L.ptr(slabs), L.ptr(loss_parts), L.stream_ptr()), "wd_tune_grad")


def tune_update(slabs, n_slab: int, loss_parts, n_cls: int, w, m, v, bank, trainable, lr: float, beta1: float, beta2: float, eps: float,
                step: int, loss_out, status, dim: int = DIM) -> None:
    """``wd_tune_update`` on the current stream for the 0-based ``step`` (Adam's t = step + 1): sums the ``n_slab`` slabs and their
    partial losses, steps the rows of ``w`` / ``m`` / ``v`` (fp32 [n_cls, 768]) whose ``trainable`` byte is non-zero, rewrites their
    rows of ``bank``, writes ``loss_out[step]`` and sets ``status[0]`` on a bad norm."""
    t = int(step) + 1
    beta1, beta2 = C.c_float(beta1).value, C.c_float(beta2).value           # the corrections use the betas the kernel receives: fp32
    L.check(LIB.wd_tune_update(L.ptr(slabs), int(n_slab), L.ptr(loss_parts), int(n_cls), int(dim), L.ptr(w), L.ptr(m), L.ptr(v), L.ptr(bank),
                               L.ptr(trainable), float(lr), beta1, beta2, float(eps), 1.0 - beta1 ** t, 1.0 - beta2 ** t, L.ptr(loss_out),
                               int(step), L.ptr(status), L.stream_ptr()), "wd_tune_update")


def check_bank(bank, what: str = "init_bank") -> torch.Tensor:
    """One shared [K, 768] bank; per-image banks are refused by name."""
    if not isinstance(bank, torch.Tensor):
        raise ValueError(f"{what}: a [K, {DIM}] tensor is supported, got {type(bank).__name__}")
    if bank.dim() == 3:
        raise NotImplementedError(f"{what}: bank tuning with per-image banks (a [B, k, {DIM}] bank) is not implemented")
    if bank.dim() != 2 or bank.shape[0] < 1 or bank.shape[1] != DIM:
        raise ValueError(f"{what}: a [K, {DIM}] tensor is supported, got {tuple(bank.shape)}")
    return bank


class BankTuner:
    """Cache of labelled batches and the optimisation loop over it.  ``add_batch`` runs the image tower once per batch and keeps
    the region embeddings and the static targets as one chunk (chunks stay as they are, never concatenated); ``fit`` then issues,
    per step, one ``wd_tune_grad`` per chunk and one ``wd_tune_update``, with no host synchronisation inside the loop."""

    def __init__(self, tower, max_cache_bytes: int = 8 << 30):
        self.tower = tower
        self.max_cache_bytes = int(max_cache_bytes)
        self.chunks: List[dict] = []
        self.cache_bytes = 0

    def chunk_bytes(self, tower=None) -> int:
        tw = tower or self.tower
        return tw.B * tw.ntot * BYTES_PER_ROW

    def check_room(self, tower=None) -> None:
        need = self.chunk_bytes(tower)
        if self.cache_bytes + need > self.max_cache_bytes:
            raise ValueError(f"bank tuning cache: this batch needs {need / 1e6:.1f} MB on top of {self.cache_bytes / 1e6:.1f} MB held, past "
                             f"max_cache_bytes = {self.max_cache_bytes / 1e6:.1f} MB (the cache holds fp32 region embeddings: 25.8 MB per "
                             f"640 x 640 image); raise max_cache_bytes or add fewer images")

    def add_batch(self, images_u8, meta, gt_boxes, gt_count, gt_cls, anchors_per_box: int = 4, min_iou: float = 0.1, tower=None) -> dict:
        """One labelled batch -> one chunk.  ``gt_boxes`` fp32 [B, max_ex, 4] in original-image pixels with ``gt_count`` int32 [B] of
        them per image and ``gt_cls`` int32 [B, max_ex] their classes; ``meta`` [B, 8] as in postprocess().  features() unfolded,
        ``embed`` cloned, wd_exemplar_assign and wd_tune_targets; all in line on the current stream.  ``tower``: another tower of
        the same weights (a batch of another shape); a chunk keeps its own anchor geometry."""
        from . import exemplar as EX
        tw = tower or self.tower
        m, min_iou = EX.check_m(anchors_per_box), EX.check_min_iou(min_iou)
        if gt_boxes.dim() != 3 or gt_boxes.shape[0] != tw.B or gt_boxes.shape[2] != 4 or not 1 <= gt_boxes.shape[1] <= EX.MAX_EX:
            raise ValueError(f"gt_boxes must be [{tw.B}, 1..{EX.MAX_EX}, 4], got {tuple(gt_boxes.shape)}")
        max_ex = int(gt_boxes.shape[1])
        if tuple(gt_cls.shape) != (tw.B, max_ex) or gt_cls.dtype != torch.int32:
            raise ValueError(f"gt_cls must be int32 [{tw.B}, {max_ex}], got {gt_cls.dtype} {tuple(gt_cls.shape)}")
        self.check_room(tw)
        i32, f32 = dict(dtype=torch.int32, device=tw.dev), dict(dtype=torch.float32, device=tw.dev)
        embed, boxes = tw.features(images_u8)
        rows = tw.B * tw.ntot
        chunk = dict(E=embed.reshape(rows, DIM).clone(), rows=rows, n_anchor=tw.ntot, off1=tw.off[1], off2=tw.off[2], pos_cls=torch.empty(tw.B, tw.ntot, **i32),
                     pos_y=torch.empty(tw.B, tw.ntot, **f32), sel_anchors=torch.empty(tw.B, max_ex * m, **i32),
                     sel_iou=torch.empty(tw.B, max_ex * m, **f32), sel_count=torch.empty(tw.B, **i32))
        EX.exemplar_assign(boxes, tw.ntot, gt_boxes, gt_count, meta, max_ex, tw.B, m, min_iou, chunk["sel_anchors"], chunk["sel_iou"],
                           chunk["sel_count"])
        tune_targets(chunk["sel_anchors"], chunk["sel_iou"], gt_cls, max_ex, m, tw.B, tw.ntot, chunk["pos_cls"], chunk["pos_y"])
        chunk["pos_sum"] = chunk["pos_y"].sum(dtype=torch.float64)          # stays on the device until fit() adds the chunks' sums
        chunk["finite"] = torch.isfinite(chunk["E"]).all()                  # read back by fit() with the sums: no sync here
        chunk["bytes"] = self.chunk_bytes(tw)
        self.chunks.append(chunk)
        self.cache_bytes += chunk["bytes"]
        return chunk

    def truncate(self, n: int) -> None:
        """Drop the chunks past the first ``n`` (a batch repeated under the range guard replaces its chunk)."""
        for c in self.chunks[n:]:
            self.cache_bytes -= c["bytes"]
        del self.chunks[n:]

    def fit(self, init_bank, steps: int, lr: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8, trainable=None):
        """``steps`` Adam steps from ``init_bank`` [K, 768] (any non-zero rows: they are normalised) over the cached chunks ->
        ``(bank, info)``: the unit rows fp32 [K, 768], and the loss before each step (``loss``), the positives per class
        (``positives``; ``no_positive`` lists the classes that learn from negatives only), the split count per chunk (``plan``) and
        ``status`` (1: a row's norm became zero or not finite and the row was left as it was).  ``lr`` and ``steps`` are
        parameters, not tuned values: nothing here has been run on trained weights.  ``trainable`` (bool [K]): False rows serve as
        negatives only and come back as the normalised start rows, bit for bit (every row of ``init_bank`` is L2-normalised once
        before the first step, as the device normalises text rows; normalising a row that is a unit row already can move an ulp).
        ValueError if a cached chunk holds a non-finite embedding: wd_tune_grad lets rows past the end of a ragged tile re-read
        the chunk's last row with a zero weight, and 0 * inf would reach every class."""
        if not self.chunks:
            raise ValueError("bank tuning: no labelled batch has been added")
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"steps: a positive int is supported, got {steps!r}")
        init_bank = check_bank(init_bank)
        tw = self.tower
        K = int(init_bank.shape[0])
        f32 = dict(dtype=torch.float32, device=tw.dev)
        w = init_bank.to(**f32).contiguous().clone()
        bank = w / w.norm(dim=1, keepdim=True)
        m, v = torch.zeros_like(w), torch.zeros_like(w)
        tr = torch.ones(K, dtype=torch.uint8, device=tw.dev) if trainable is None else \
            torch.as_tensor(trainable).to(device=tw.dev).ne(0).to(torch.uint8).contiguous()
        if tuple(tr.shape) != (K,):
            raise ValueError(f"trainable: one flag per class ({K}) is supported, got {tuple(tr.shape)}")
        splits = [plan(c["rows"], K) for c in self.chunks]
        n_slab, kp = sum(splits), k_pad(K)
        slabs = torch.empty(n_slab, kp, DIM, **f32)
        loss_parts = torch.empty(n_slab, kp // CLASS_BLOCK, **f32)
        loss = torch.zeros(steps, **f32)
        status = torch.zeros(1, dtype=torch.int32, device=tw.dev)
        pos = torch.zeros(K, dtype=torch.int64, device=tw.dev)
        for c in self.chunks:
            pc = c["pos_cls"].reshape(-1)
            pos += torch.bincount(pc[(pc >= 0) & (pc < K)].to(torch.int64), minlength=K)
        # the one read-back, before the loop: the chunks' target sums and whether every cached embedding is finite
        head = torch.stack([torch.stack([c["pos_sum"] for c in self.chunks]).sum(),
                            torch.stack([c["finite"] for c in self.chunks]).all().to(torch.float64)]).tolist()
        if head[1] != 1.0:
            raise ValueError("bank tuning: a cached chunk holds non-finite region embeddings (an image tower out of its range); "
                             "nothing was fitted")
        inv_norm = 1.0 / max(head[0], 1.0)
        for step in range(steps):
            o = 0
            for c, s in zip(self.chunks, splits):
                tune_grad(c["E"], c["rows"], c["n_anchor"], c["off1"], c["off2"], tw.lvl_scale, tw.lvl_bias, c["pos_cls"], c["pos_y"], bank,
                          K, inv_norm, s, slabs[o:o + s], loss_parts[o:o + s])
                o += s
            tune_update(slabs, n_slab, loss_parts, K, w, m, v, bank, tr, lr, betas[0], betas[1], eps, step, loss, status)
        positives = pos.tolist()
        info = dict(loss=loss.tolist(), positives=positives, no_positive=[k for k, n in enumerate(positives) if n == 0], plan=splits,
                    status=int(status.item()), norm=1.0 / inv_norm, w=w, m=m, v=v)
        return bank, info
