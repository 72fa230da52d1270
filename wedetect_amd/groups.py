"""Prompt groups (include/wedetect_hip_groups.h, csrc/groups.hip, the class-max epilogue of csrc/split_gemm_p8.hip): a class with
several names is scored as the best of them.  This module holds the host-side packing of the prompts (:class:`PromptGroups`) and the
ctypes binding of the two entry points.  A version and an export list of its own, like best.py, sparse.py and topn.py: the main
ABI stays as it is."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L
from .lib import f32, fp, i32, i64, vp

GROUPS_ABI_VERSION = 1
BIN = 32                         # WD_GROUP_BIN: bank rows per bin; no class straddles one
FUSED_CHUNK = 1 << 20            # bank rows per wd_group_similarity_split launch (32-bit DMA offsets); a multiple of BIN
ROWS_CHUNK = 4096                # bank rows per materialised block on the other paths; a multiple of BIN

SIGNATURES = {
    "wd_groups_abi_version": (None, []),
    "wd_group_similarity_split": (None, [vp, i64, vp, f32, i32, i32, i32, i32, i32, fp, fp, vp, vp, vp, i32, vp, i32, i32, vp]),
    "wd_group_rows": (None, [vp, i64, i32, i32, vp, vp, i32, vp, i32, i32, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("groups", GROUPS_ABI_VERSION, SIGNATURES)


class PromptGroups:
    """The layout of a bank of P prompts of G classes for the grouped score step: next-fit in class order into bins of 32 bank
    rows, so that no class straddles a bin and output column g is class g.  A class goes into the current bin if all its prompts
    still fit; otherwise the bin is closed and a new one starts.  A closed bin (and the last one) is padded by REPEATING the last
    real row of its last class: a duplicate row scores what its original scores, so the class maximum is unchanged.

    ``rows``       int64 [K_pad]: gather index into the flat prompt list — the bank the tower sees is ``bank_flat[rows]``
    ``group_of``   int32 [K_pad]: the class of every padded row, non-decreasing
    ``bin_first``  int32 [K_pad / 32 + 1]: the classes of bin s are ``[bin_first[s], bin_first[s + 1])``
    ``sizes``      prompts per class; ``G`` classes, ``P`` prompts, ``K_pad`` padded rows (a multiple of 32)
    ``flat``       the prompts in class order (``from_texts``), None for ``from_sizes``

    A class with no prompt or with more than 32 prompts is refused (ValueError naming the class)."""

    def __init__(self, sizes: Sequence[int], flat: Optional[List[str]] = None, names: Optional[Sequence[str]] = None):
        sizes = [int(s) for s in sizes]
        if not sizes:
            raise ValueError("prompt groups: at least one class is needed")
        rows: List[int] = []
        group_of: List[int] = []
        bin_first = [0]
        first = 0                                  # flat index of the class's first prompt
        for g, n in enumerate(sizes):
            if not 1 <= n <= BIN:
                what = f"class {g}" + (f" ({names[g]!r})" if names is not None else "")
                raise ValueError(f"prompt groups: {what} has {n} prompts; 1 .. {BIN} are supported")
            if len(rows) % BIN + n > BIN:          # does not fit: close the bin with copies of the row before
                pad = BIN - len(rows) % BIN
                rows += [rows[-1]] * pad
                group_of += [group_of[-1]] * pad
                bin_first.append(g)
            elif rows and len(rows) % BIN == 0:    # the class before filled its bin exactly
                bin_first.append(g)
            rows += range(first, first + n)
            group_of += [g] * n
            first += n
        pad = -len(rows) % BIN
        rows += [rows[-1]] * pad
        group_of += [group_of[-1]] * pad
        bin_first.append(len(sizes))
        self.sizes = tuple(sizes)
        self.flat = flat
        self.G, self.P, self.K_pad = len(sizes), first, len(rows)
        self.rows = torch.tensor(rows, dtype=torch.int64)
        self.group_of = torch.tensor(group_of, dtype=torch.int32)
        self.bin_first = torch.tensor(bin_first, dtype=torch.int32)
        assert self.K_pad % BIN == 0 and len(bin_first) == self.K_pad // BIN + 1
        self._dev: Dict[str, tuple] = {}

    @classmethod
    def from_sizes(cls, sizes: Sequence[int]) -> "PromptGroups":
        return cls(sizes)

    @classmethod
    def from_texts(cls, texts: Sequence[Sequence[str]]) -> "PromptGroups":
        """``texts``: one list of prompts per class (a bare string is a class of one prompt), as the class-text files hold them."""
        lists = [[t] if isinstance(t, str) else list(t) for t in texts]
        return cls([len(t) for t in lists], [p for t in lists for p in t], [(t[0] if t else "") for t in lists])

    def first_of(self) -> torch.Tensor:
        """int64 [G]: the flat index of every class's first prompt (the 'first caption' bank is ``bank_flat[first_of()]``)."""
        s = torch.tensor(self.sizes, dtype=torch.int64)
        return torch.cumsum(s, 0) - s

    def device(self, dev) -> tuple:
        """(rows, group_of, bin_first) on ``dev``, copied once per plan and device."""
        key = str(torch.device(dev))
        hit = self._dev.get(key)
        if hit is None:
            hit = self._dev[key] = (self.rows.to(dev), self.group_of.to(dev), self.bin_first.to(dev))
        return hit

    def pad_bank(self, bank_flat: torch.Tensor) -> torch.Tensor:
        """``bank_flat`` [P, D] (one row per prompt, class order) -> the padded bank [K_pad, D] the tower sees."""
        if bank_flat.dim() != 2 or bank_flat.shape[0] != self.P:
            raise ValueError(f"prompt groups: the bank holds {tuple(bank_flat.shape)}, expected ({self.P}, D): one row per prompt")
        rows = self.device(bank_flat.device)[0] if bank_flat.is_cuda else self.rows
        return bank_flat.index_select(0, rows).contiguous()

    def class_max(self, scores):
        """numpy / torch restatement of the result: ``scores`` [..., K_pad] -> [..., G], the maximum over every class's rows."""
        if isinstance(scores, np.ndarray):
            go = self.group_of.numpy()
            starts = np.flatnonzero(np.r_[True, go[1:] != go[:-1]])
            return np.maximum.reduceat(scores, starts, axis=-1)
        go = self.group_of.to(scores.device).to(torch.int64)
        out = torch.full(scores.shape[:-1] + (self.G,), float("-inf"), dtype=scores.dtype, device=scores.device)
        return out.scatter_reduce(-1, go.expand(scores.shape), scores, reduce="amax", include_self=True)

    def __repr__(self) -> str:
        return f"PromptGroups(G={self.G}, P={self.P}, K_pad={self.K_pad})"


def _check_tables(groups: PromptGroups, group_of, bin_first) -> None:
    if group_of.dtype != torch.int32 or bin_first.dtype != torch.int32 or not group_of.is_contiguous() or not bin_first.is_contiguous():
        raise L.WedetectHipError("prompt groups: the tables must be contiguous int32 tensors")
    if group_of.numel() != groups.K_pad or bin_first.numel() != groups.K_pad // BIN + 1:
        raise L.WedetectHipError("prompt groups: the tables do not belong to this plan")


def group_similarity_split(e_split, rows, t_split, unscale, n_cls, dim, group_of, bin_first, cls_offset, out, ldo, n_groups, seg=None,
                           range_flag=None, t_row=0) -> None:
    """``wd_group_similarity_split`` on the current stream; operands as :func:`best.best_similarity_split`.  ``group_of`` /
    ``bin_first``: the WHOLE device tables of the plan; ``cls_offset`` the bank row at which this launch's ``n_cls`` rows begin
    (both multiples of 32), ``t_row`` that row's position in ``t_split``.  ``out`` fp32 rows of stride ``ldo``."""
    sr, e0, e1, sc, sb = L.seg_args(seg)
    L.check(LIB.wd_group_similarity_split(L.ptr(e_split), int(rows), L.bank_row_ptr(t_split, t_row, dim), float(unscale), int(n_cls),
                                          int(dim), sr, e0, e1, sc, sb, L.ptr(range_flag), L.ptr(group_of), L.ptr(bin_first),
                                          int(cls_offset), L.ptr(out), int(ldo), int(n_groups), L.stream_ptr()), "wd_group_similarity_split")


def group_rows(block, rows, n_cls, ld, group_of, bin_first, cls_offset, out, ldo, n_groups) -> None:
    """``wd_group_rows`` on the current stream: the class maxima of a materialised [rows, ld] block of scores of bank rows
    [cls_offset, cls_offset + n_cls)."""
    L.check(LIB.wd_group_rows(L.ptr(block), int(rows), int(n_cls), int(ld), L.ptr(group_of), L.ptr(bin_first), int(cls_offset), L.ptr(out),
                              int(ldo), int(n_groups), L.stream_ptr()), "wd_group_rows")
