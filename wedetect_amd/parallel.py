"""Multi-GPU plumbing: one process per GPU, images sharded, one exchange step.

The reference shards the image list contiguously per rank (InferenceSampler,
eval_retrieval/extract_embedding.py:1620-1644) and, at the very end, pickles four Python
lists of CPU tensors through ``all_gather_object`` (1753-1756).  Here the per-image results
live in fixed-shape device tensors, so the exchange is ``all_gather_into_tensor`` on
[B_local, 300, 768] (+ counts, scales, bias, ids) over RCCL (backend "nccl" on ROCm; "gloo"
in the CPU tests).  The detector forward itself needs no communication (eval-mode BN).
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist


class PhaseWatchdog:
    """Per-rank progress deadline for multi-process runs (round 5).  A collective never returns when one rank is missing, and
    seven healthy ranks waiting in an all-gather say nothing about WHICH rank is gone.  Every rank therefore carries its
    own deadline: ``phase(name)`` marks progress and names what the rank is doing; when ``timeout_s`` pass without a new
    mark, a daemon thread prints ``rank r: no progress for T s in phase '<name>'`` to stderr and calls ``on_expire``
    (default ``os._exit(3)``): the launcher (torch.distributed.run) then tears the job down with a non-zero status.  The
    rank that is stuck OUTSIDE a collective names itself; the ranks waiting for it name the collective they wait in."""

    def __init__(self, rank: int, timeout_s: float, on_expire=None, poll_s: float = 0.25):
        import threading
        import time
        self.rank, self.timeout_s, self._name = rank, float(timeout_s), "start"
        self._t0, self._time, self._stop = time.monotonic(), time, False
        self._on_expire = on_expire
        self.expired = None
        self._th = threading.Thread(target=self._loop, args=(poll_s,), daemon=True)
        self._th.start()

    def phase(self, name: str) -> None:
        self._name, self._t0 = name, self._time.monotonic()

    def stop(self) -> None:
        self._stop = True

    def _loop(self, poll_s: float) -> None:
        import os
        import sys
        while not self._stop:
            self._time.sleep(poll_s)
            waited = self._time.monotonic() - self._t0
            if not self._stop and waited > self.timeout_s:
                self.expired = f"rank {self.rank}: no progress for {waited:.0f} s in phase '{self._name}'"
                print(f"wedetect_amd watchdog: {self.expired}; failing the run", file=sys.stderr, flush=True)
                if self._on_expire is not None:
                    self._on_expire(self)
                    return
                os._exit(3)


def bounded_wait(work, timeout_s: float, what: str, rank: int) -> None:
    """``work.wait`` with a deadline: a collective that does not complete within ``timeout_s`` raises with the rank and
    the collective's name instead of blocking for the backend's default (30 min for gloo / RCCL)."""
    import datetime
    try:
        ok = work.wait(datetime.timedelta(seconds=timeout_s))
    except RuntimeError as ex:                       # gloo / RCCL raise on a timed-out wait
        raise RuntimeError(f"rank {rank}: collective '{what}' did not complete within {timeout_s:.0f} s ({ex})") from ex
    if ok is False:
        raise RuntimeError(f"rank {rank}: collective '{what}' did not complete within {timeout_s:.0f} s")


def shard_range(total: int, world: int, rank: int) -> range:
    """Contiguous shard of ``range(total)`` for ``rank`` — the same split as
    InferenceSampler._get_local_indices (extract_embedding.py:1631-1638): the first
    ``total % world`` ranks get one extra item."""
    if world <= 0 or not (0 <= rank < world) or total < 0:
        raise ValueError(f"bad shard request total={total} world={world} rank={rank}")
    base, left = divmod(total, world)
    begin = rank * base + min(rank, left)
    return range(begin, begin + base + (1 if rank < left else 0))


def _world(group=None) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def gather_ragged(fields: Dict[str, torch.Tensor], group=None) -> Dict[str, torch.Tensor]:
    """All-gather per-image tensors whose leading axis (images held by this rank) may DIFFER between ranks — the
    last batches of an ``InferenceSampler`` split (extract_embedding.py:1631-1638: the first ``total % world`` ranks
    hold one image more) or a short final batch.  One small all-gather of the lengths, every field padded to the
    longest rank for ``all_gather_into_tensor`` and trimmed afterwards; result rows are rank-major = the global image
    order of ``shard_range``.  Every field of one call must have the same leading length; a rank may hold 0 images."""
    if not fields:
        return {}
    lens = {int(v.shape[0]) for v in fields.values()}
    if len(lens) != 1:
        raise ValueError(f"fields disagree on the number of local images: {sorted(lens)}")
    n_local = lens.pop()
    if _world(group) == 1:
        return dict(fields)
    world = dist.get_world_size(group)
    any_t = next(iter(fields.values()))
    n_all = torch.empty(world, dtype=torch.int64, device=any_t.device)
    dist.all_gather_into_tensor(n_all, torch.tensor([n_local], dtype=torch.int64, device=any_t.device), group=group)
    n_all = [int(v) for v in n_all.tolist()]
    widest = max(n_all)
    out = {}
    for k, v in fields.items():
        if n_local < widest:
            pad = torch.zeros((widest - n_local,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            v = torch.cat([v, pad], dim=0)
        o = torch.empty((world * widest,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
        dist.all_gather_into_tensor(o, v.contiguous(), group=group)
        if min(n_all) == widest:
            out[k] = o
        else:
            o = o.view((world, widest) + tuple(v.shape[1:]))
            out[k] = torch.cat([o[r, : n_all[r]] for r in range(world)], dim=0)
    return out


def gather_regions(embeddings: torch.Tensor, count: torch.Tensor, group=None) -> Dict[str, torch.Tensor]:
    """All-gather the kept-region embeddings [B_local, R, D] and counts [B_local] of every
    rank -> [sum B_local, R, D], [sum B_local]; rank-major order, i.e. the global image order when images were
    sharded with ``shard_range``.  Ranks may hold different numbers of images (ragged final batch)."""
    if embeddings.shape[0] != count.shape[0]:
        raise ValueError("embeddings and count disagree on the number of images")
    return gather_ragged(dict(embeddings=embeddings, count=count), group)


class RegionGatherer:
    """Pipelined form of :func:`gather_regions` for a stream of batches: ``submit`` copies the
    step's kept-region tensors into one of two staging slots and starts the all-gather
    asynchronously (RCCL runs it on its own stream, behind the producing kernels); the caller's
    stream goes straight on to the next batch and picks the result up with ``collect`` — at the
    next ``submit`` at the latest.  Over xGMI a [32, 300, 768] fp32 block per rank is ~4 ms at 8
    ranks; overlapped it costs the step nothing.  The tower's output buffers may be overwritten
    as soon as ``submit`` returns (the staging copy is ordered before it on the same stream) — with or without a
    process group.  Every rank must submit the same B_local per step (pad the final short batch with count = 0
    rows, or use ``gather_ragged`` for it).

    Per step TWO collectives: the embeddings block, and one int32 block [B_local, 2 R + 3] that carries everything
    else the reference gathers (extract_embedding.py:1753-1756): per-region ``scales`` and ``bias`` (fp32 bit
    patterns), the kept count and the 64-bit image id as two int32 words — instead of four pickled object gathers.
    The block is cleared on every ``submit``: a field the caller leaves out reads as zeros, never as the previous
    step's values."""

    def __init__(self, group=None, timeout_s: Optional[float] = None):
        """``timeout_s``: deadline for the host-side wait on a gather in ``collect`` (None: the backend's own)."""
        self.group = group
        self.timeout_s = timeout_s
        self.slots = [None, None]
        self.turn = 0
        self.pending = None               # (work handles, slot, has_extra)

    def _slot(self, emb, world):
        s = self.slots[self.turn]
        b, r = emb.shape[0], emb.shape[1]
        if s is None or s["emb"].shape != emb.shape or s["emb"].dtype != emb.dtype or s["emb"].device != emb.device:
            s = dict(emb=torch.empty_like(emb), meta=torch.zeros(b, 2 * r + 3, dtype=torch.int32, device=emb.device),
                     out_e=torch.empty((world * b,) + tuple(emb.shape[1:]), dtype=emb.dtype, device=emb.device),
                     out_m=torch.empty(world * b, 2 * r + 3, dtype=torch.int32, device=emb.device))
            self.slots[self.turn] = s
        return s

    def submit(self, embeddings: torch.Tensor, count: torch.Tensor, scales: Optional[torch.Tensor] = None,
               bias: Optional[torch.Tensor] = None, image_ids: Optional[torch.Tensor] = None) -> Optional[Dict[str, torch.Tensor]]:
        """Starts the exchange of this step; returns the PREVIOUS step's gathered result (or None).  ``embeddings``
        [B, R, D], ``count`` [B]; optional ``scales`` / ``bias`` [B, R] fp32 and ``image_ids`` [B] (any int64)."""
        prev = self.collect()
        single = not dist.is_available() or not dist.is_initialized()
        world = 1 if single else dist.get_world_size(self.group)
        s = self._slot(embeddings, world)
        r = embeddings.shape[1]
        s["emb"].copy_(embeddings, non_blocking=True)
        m = s["meta"]
        m.zero_()
        if scales is not None:
            m[:, :r].copy_(scales.contiguous().view(torch.int32), non_blocking=True)
        if bias is not None:
            m[:, r:2 * r].copy_(bias.contiguous().view(torch.int32), non_blocking=True)
        m[:, 2 * r].copy_(count.to(torch.int32), non_blocking=True)
        if image_ids is not None:
            m[:, 2 * r + 1:2 * r + 3].copy_(image_ids.to(torch.int64).contiguous().view(-1, 1).view(torch.int32), non_blocking=True)
        extra = (scales is not None, bias is not None, image_ids is not None)
        if single:                                    # same contract without a process group: the caller's buffers
            self.pending = (None, dict(out_e=s["emb"], out_m=s["meta"]), extra)   # are free again as soon as submit returns
            self.turn ^= 1
            return prev
        h1 = dist.all_gather_into_tensor(s["out_e"], s["emb"], group=self.group, async_op=True)
        h2 = dist.all_gather_into_tensor(s["out_m"], s["meta"], group=self.group, async_op=True)
        self.pending = ((h1, h2), s, extra)
        self.turn ^= 1
        return prev

    def collect(self) -> Optional[Dict[str, torch.Tensor]]:
        """Waits (stream-side on GPUs) for the exchange in flight; its tensors stay valid until the
        second ``submit`` after this call."""
        if self.pending is None:
            return None
        handles, s, extra = self.pending
        self.pending = None
        if handles is not None:
            for i, h in enumerate(handles):
                if self.timeout_s is None:
                    h.wait()
                else:
                    bounded_wait(h, self.timeout_s, "region gather: " + ("embeddings" if i == 0 else "metadata"),
                                 dist.get_rank(self.group))
        e, m = s["out_e"], s["out_m"]
        r = e.shape[1]
        out = dict(embeddings=e, count=m[:, 2 * r])
        if extra[0]:
            out["scales"] = m[:, :r].view(torch.float32)
        if extra[1]:
            out["bias"] = m[:, r:2 * r].view(torch.float32)
        if extra[2]:
            out["image_ids"] = m[:, 2 * r + 1:2 * r + 3].contiguous().view(torch.int64).view(-1)
        return out


class StreamedRecordCollector:
    """Result collection for a whole evaluation run (extract_embedding.py:1746-1761) with BOUNDED device memory: every
    step's kept regions go through a :class:`RegionGatherer` (two staging slots of world x B_local x R x D floats,
    whatever the size of the image set); ``dst`` trims each gathered image to its kept rows and moves those to the
    host, the other ranks drop the block.  The reference moves only kept rows through its object gathers too; the
    round-2 form (all results dense on the device, one final all-gather onto EVERY rank) needed N_total x 0.92 MB per
    GPU.  Every rank must call ``step`` the same number of times with the same B_local (``pad_step`` for ranks whose
    shard ran out; short batches are padded with count-0 rows)."""

    def __init__(self, batch: int, regions: int, dim: int, device, dst: int = 0, group=None):
        self.g = RegionGatherer(group)
        self.batch, self.regions, self.dim, self.dev = batch, regions, dim, device
        single = not dist.is_available() or not dist.is_initialized()
        self.world = 1 if single else dist.get_world_size(group)
        self.rank = 0 if single else dist.get_rank(group)
        self.dst = dst
        self.per_rank = [[] for _ in range(self.world)]        # dst only: records in each rank's own image order

    def _pad(self, t, shape, dtype):
        out = torch.zeros(shape, dtype=dtype, device=self.dev)
        if t is not None and t.shape[0]:
            out[: t.shape[0]] = t
        return out

    def step(self, embeddings, count, scales, bias, image_ids) -> None:
        b, r, d = self.batch, self.regions, self.dim
        n = 0 if embeddings is None else int(embeddings.shape[0])
        if n > b:
            raise ValueError(f"step holds {n} images, collector was built for {b}")
        if n < b:                                              # short final batch / exhausted shard: count-0 rows
            embeddings = self._pad(embeddings, (b, r, d), torch.float32)
            count = self._pad(count, (b,), torch.int32)
            scales, bias = self._pad(scales, (b, r), torch.float32), self._pad(bias, (b, r), torch.float32)
            image_ids = self._pad(image_ids, (b,), torch.int64)
            valid = torch.zeros(b, dtype=torch.int32, device=self.dev)
            valid[:n] = 1
        else:
            valid = torch.ones(b, dtype=torch.int32, device=self.dev)
        # the validity flag rides in the count word's sign-free high bit space: count <= R < 2^16
        self._drain(self.g.submit(embeddings, count.to(torch.int32) + (valid << 16), scales=scales, bias=bias, image_ids=image_ids))

    def pad_step(self) -> None:
        self.step(None, None, None, None, None)

    def _drain(self, got) -> None:
        """dst: the step's kept rows -> host.  ONE device-to-host copy per field per step (round 3 copied three slices per
        image: ~770 small synchronising copies per step at 8 ranks x 32 images): the kept rows of all gathered images are
        compacted on the device with one row mask, moved as three tensors, and split per image on the host."""
        if got is None or self.rank != self.dst:
            return
        cw = got["count"]
        valid_d = (cw >> 16) != 0
        cnt_d = torch.where(valid_d, cw & 0xFFFF, torch.zeros_like(cw))
        rows = torch.arange(got["embeddings"].shape[1], device=cw.device)[None, :] < cnt_d[:, None]      # [N, R] kept-row mask
        emb = got["embeddings"][rows].cpu()                       # [sum(count), D]
        sc = got["scales"][rows].cpu()
        bi = got["bias"][rows].cpu()
        head = torch.stack([cnt_d.to(torch.int64), valid_d.to(torch.int64), got["image_ids"].to(torch.int64)]).cpu()
        cnt, valid, ids = head[0].tolist(), head[1].tolist(), head[2].tolist()
        b = self.batch
        off = 0
        for i, (v, c, iid) in enumerate(zip(valid, cnt, ids)):
            if not v:
                continue
            self.per_rank[i // b].append({"image_id": int(iid), "embedding": emb[off:off + c].clone(),
                                          "scale": sc[off:off + c].clone(), "bias": bi[off:off + c].clone()})
            off += c

    def finish(self):
        """Records in global (rank-major = ``shard_range``) image order on ``dst``; [] elsewhere."""
        self._drain(self.g.collect())
        return [rec for lst in self.per_rank for rec in lst]


def gather_results(fields: Dict[str, torch.Tensor], group=None) -> Dict[str, torch.Tensor]:
    """Same exchange for any dict of per-image tensors with a leading B_local axis (image ids,
    scales, bias ... — the four lists of extract_embedding.py:1753-1756 in one place); ragged-safe."""
    return gather_ragged(fields, group)


def shard_bank_by_class(bank: torch.Tensor, world: int, rank: int) -> torch.Tensor:
    """Class-shard of a [K, D] text bank for the 1M-class retrieval configuration
    (SURVEY.md §8e): every rank scores ALL gathered regions against its K/world classes."""
    r = shard_range(bank.shape[0], world, rank)
    return bank[r.start:r.stop]


class BankScorer:
    """Scores kept regions against a [K, D] text bank (or a rank's class shard of it): [N, K] fp32, per image the max over
    its kept regions of sigmoid(<e, t_k> exp(scale) + bias) (retrieval_metric.py:369-375), logits never materialised.

    ``precision`` (None = $WEDETECT_RETRIEVAL_PRECISION, default "fp16x3"): "fp16x3" = wd_retrieval_max_split — operands as
    fp16 (hi, lo) pairs, three fp16-MFMA passes, fp32 accumulate, the bank split ONCE here — under the tower's kind of
    range guard: the kernel raises a sticky flag when an accumulator is inf / NaN (an embedding beyond 65504), and the
    scorer then switches to the fp32-MFMA kernel (wd_retrieval_max) for good and repeats the call.  "fp32" = that kernel
    from the start.  Round 4 shipped the fp32 kernel here and kept the 2.5 x faster one for tests and scripts."""

    FP32_MAX_ROWS = 320          # wd_retrieval_max keeps an image's rows in one workgroup

    def __init__(self, bank: torch.Tensor, precision: Optional[str] = None, hold_bank: bool = True):
        """``hold_bank`` False (the module-level cache below): a bank that is already contiguous is held by WEAK reference only, so
        that caching the scorer does not pin a 3 GB bank the caller has dropped; the fp32 kernel then needs the caller's
        tensor to be alive, which it is for as long as the cache can hit."""
        import os
        import weakref
        if precision is None:
            precision = os.environ.get("WEDETECT_RETRIEVAL_PRECISION", "fp16x3")
        if precision not in ("fp32", "fp16x3"):
            raise ValueError("precision must be 'fp32' or 'fp16x3'")
        if bank.dim() != 2 or bank.dtype != torch.float32 or not bank.is_cuda:
            raise ValueError("bank must be a device float32 [K, D] tensor")
        cont = bank.contiguous()
        self._bank = cont if (hold_bank or cont is not bank) else None
        self._bank_ref = weakref.ref(bank) if self._bank is None else None
        self.n_classes, self.dim = int(bank.shape[0]), int(bank.shape[1])
        self.precision = precision
        self.overflowed = False
        self._split = None
        self.flag = torch.zeros(1, dtype=torch.int32, device=bank.device)

    @property
    def bank(self) -> torch.Tensor:
        b = self._bank if self._bank is not None else self._bank_ref()
        if b is None:
            raise RuntimeError("BankScorer: the text bank this scorer was built for has been freed")
        return b

    def _launch(self, e, c, s, b, out):
        from . import lib as L
        n, r, d = e.shape
        k = self.n_classes
        if self.precision == "fp16x3" and d % 16 == 0:
            if self._split is None:
                self._split = L.split_weights(self.bank)
            L.retrieval_max_split(e, self._split, s, b, c, out, n, r, k, d, range_flag=self.flag)
            return True
        # the fp32 kernel — asked for, reached after a range trip, or because dim % 16 != 0: its row limit is checked HERE, with
        # its own message, whatever ``precision`` read before the call
        if r > self.FP32_MAX_ROWS:
            raise ValueError(f"the fp32 retrieval kernel takes at most {self.FP32_MAX_ROWS} regions per image, got {r} "
                             f"(precision {self.precision!r}{', after a range trip' if self.overflowed else ''}, dim {d})")
        L.retrieval_max(e, self.bank, s, b, c, out, n, r, k, d)
        return False

    def __call__(self, embeddings, count, scales, bias, out: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
        """``check`` False skips the host read of the range flag (a caller that pipelines steps reads ``tripped()`` itself
        before it trusts the scores)."""
        n = embeddings.shape[0]
        if out is None:
            out = torch.empty(n, self.n_classes, dtype=torch.float32, device=embeddings.device)
        e, c = embeddings.contiguous(), count.to(torch.int32).contiguous()
        s, b = scales.contiguous(), bias.contiguous()
        guarded = self._launch(e, c, s, b, out)
        if guarded and check and self.tripped():
            import warnings
            warnings.warn("wedetect_amd: a region embedding left the fp16 range in the fp16x3 retrieval kernel; this scorer now "
                          "runs the fp32 MFMA kernel")
            self.precision, self.overflowed = "fp32", True
            self.flag.zero_()
            self._launch(e, c, s, b, out)
        return out

    def tripped(self) -> bool:
        return bool(int(self.flag.item()))


_SCORERS: list = []      # small cache of (weakref to the bank, version, precision, BankScorer): splitting a 1M-class bank is a pass over 3 GB


def clear_scorer_cache() -> None:
    """Drops the cached scorers (and with them the split copies of their banks: 3 GB per 1M x 768 bank)."""
    _SCORERS.clear()
    _NAMERS.clear()


def device_retrieval_scores(embeddings: torch.Tensor, count: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor,
                            bank: torch.Tensor, precision: Optional[str] = None, check: bool = True) -> torch.Tensor:
    """[N, K] fp32: max over an image's kept regions of sigmoid(<e, t_k> exp(scale) + bias) on the device
    (retrieval_metric.py:369-375).  ``embeddings`` [N, R, D], ``scales`` / ``bias`` [N, R], ``count`` [N].  Runs the fp16x3
    kernel under its range guard by default (:class:`BankScorer`); the bank's split form is cached per bank tensor — by WEAK
    reference: an entry dies with its bank (and takes the split copy with it), :func:`clear_scorer_cache` drops the rest.
    ``check`` False skips the per-call host read of the range flag (a pipelined caller reads ``BankScorer.tripped()`` itself)."""
    import weakref
    # keyed by the tensor OBJECT (weak reference) and its version counter — never by address: a freed bank's address can be
    # handed to the next one, which would then be scored against the old split
    _SCORERS[:] = [ent for ent in _SCORERS if ent[0]() is not None]
    for ref, ver, prec, sc in _SCORERS:
        if ref() is bank and ver == bank._version and prec == precision:
            return sc(embeddings, count, scales, bias, check=check)
    sc = BankScorer(bank, precision, hold_bank=False)
    _SCORERS.append((weakref.ref(bank), bank._version, precision, sc))
    del _SCORERS[:-2]
    return sc(embeddings, count, scales, bias, check=check)


class RegionNamer:
    """Names kept regions from a [K, D] text bank: for every region the ``n_top`` (1..8) best classes by
    sigmoid(<e, t_k> exp(scale) + bias) — the per-region score of retrieval_metric.py:373 BEFORE its max over regions — score
    descending, class ascending among equal scores (include/wedetect_hip_topn.h).  The [N * R, K] logits are never materialised:
    the auto-labelling use of the class-agnostic proposals against banks where that tensor cannot exist.

    Structure as :class:`BankScorer`.  ``precision`` "fp16x3" (the default, $WEDETECT_RETRIEVAL_PRECISION): the bank is split ONCE
    here and scored by ``wd_topn_similarity_split`` with the row affine, in class chunks under the kernel's 2^32-byte limit, under the
    range guard: the flag is read once per call, and a trip switches the namer for good to the fp32 path and repeats the call.
    "fp32", banks below 256 rows, dim % 32: ``wd_conv_gemm`` logit blocks of at most 4096 classes, then ``wd_topn_rows`` with the row
    affine.  One rank, one bank: keys of class shards merge by sorting, which a later change can add."""

    FUSED_MIN = 256              # rows of a bank from which the 256 x 256 kernel is used (engine.ImageTower.SIM_SPLIT_MIN)

    def __init__(self, bank: torch.Tensor, n_top: int, precision: Optional[str] = None):
        import os
        from . import topn as TN
        if precision is None:
            precision = os.environ.get("WEDETECT_RETRIEVAL_PRECISION", "fp16x3")
        if precision not in ("fp32", "fp16x3"):
            raise ValueError("precision must be 'fp32' or 'fp16x3'")
        if bank.dim() != 2 or bank.dtype != torch.float32 or not bank.is_cuda:
            raise ValueError("bank must be a device float32 [K, D] tensor")
        self.n_top = TN.check_n_top(n_top)
        self.bank = bank.contiguous()
        self.n_classes, self.dim = int(bank.shape[0]), int(bank.shape[1])
        self.precision = precision
        self.overflowed = False
        self._split = None
        self.flag = torch.zeros(1, dtype=torch.int32, device=bank.device)

    def _fused_ok(self) -> bool:
        return self.precision == "fp16x3" and self.dim % 32 == 0 and self.n_classes >= self.FUSED_MIN

    def _launch(self, e, s, b, key) -> bool:
        from . import lib as L
        from . import topn as TN
        rows, d, k, n = e.shape[0], self.dim, self.n_classes, self.n_top
        if self._fused_ok():
            if self._split is None:
                self._split = L.split_weights(self.bank)
            es = torch.empty(L.LIB.wd_split_weights_bytes(rows, d), dtype=torch.uint8, device=e.device)
            L.split_weights_scaled(e, es)                       # scale 1, as wd_retrieval_max_split's callers split the region rows
            row_bytes = (d + 15) // 16 * 16 * 4
            step = min(TN.FUSED_CHUNK, (((1 << 32) - 1) // row_bytes - 8) // 8 * 8)
            for c0 in range(0, k, step):
                TN.topn_similarity_split(es, rows, self._split[0], self._split[1], min(step, k - c0), d, n, key, c0, row_scale=s, row_bias=b,
                                         range_flag=self.flag, t_row=c0)
            return True
        block = torch.empty(rows, min(TN.ROWS_CHUNK, k), dtype=torch.float32, device=e.device)
        for c0 in range(0, k, TN.ROWS_CHUNK):
            kc = min(TN.ROWS_CHUNK, k - c0)
            L.conv_gemm(e, self.bank[c0:c0 + kc], None, block, batch=1, hin=1, win=rows, cin=d, lda=d, n=kc, ldc=kc)
            TN.topn_rows(block, 1, rows, kc, kc, n, key, c0, row_scale=s, row_bias=b)
        return False

    def __call__(self, embeddings, count, scales, bias):
        """``embeddings`` [N, R, D], ``count`` [N], ``scales`` / ``bias`` [N, R] -> (scores [N, R, n_top] fp32, labels [N, R, n_top]
        int32); regions r >= count[i] and slots beyond the bank come out empty: (0, -1)."""
        import warnings
        from . import topn as TN
        n_img, r, d = embeddings.shape
        if d != self.dim:
            raise ValueError(f"embeddings of dim {d} against a bank of dim {self.dim}")
        dev, n = embeddings.device, self.n_top
        e = embeddings.contiguous().view(n_img * r, d)
        s, b = scales.contiguous().view(-1), bias.contiguous().view(-1)
        c = count.to(torch.int32).contiguous()
        key = torch.zeros(n_img * r, n, dtype=torch.int64, device=dev)
        if self._launch(e, s, b, key) and bool(int(self.flag.item())):
            warnings.warn("wedetect_amd: a region embedding left the fp16 range in the fp16x3 top-n kernel; this namer now runs the "
                          "fp32 path")
            self.precision, self.overflowed = "fp32", True
            self.flag.zero_()
            key.zero_()
            self._launch(e, s, b, key)
        # every region is its own "kept row": wd_topn_kept lays the lists out as [N][R][n] and empties the rows from count on
        rows_of = torch.arange(r, dtype=torch.int32, device=dev).repeat(n_img, 1)
        scores = torch.empty(n_img, r, n, dtype=torch.float32, device=dev)
        labels = torch.empty(n_img, r, n, dtype=torch.int32, device=dev)
        TN.topn_kept(key, n, r, rows_of, c, r, n_img, scores, labels)
        return scores, labels


_NAMERS: list = []       # (weakref to the bank, version, n_top, precision, RegionNamer), as _SCORERS


def device_region_names(embeddings: torch.Tensor, count: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor, bank: torch.Tensor,
                        n_top: int, precision: Optional[str] = None):
    """:class:`RegionNamer` with the namer (and the bank's split form) cached per bank tensor, as
    :func:`device_retrieval_scores` caches its scorer: by weak reference and version counter, the last two banks."""
    import weakref
    _NAMERS[:] = [ent for ent in _NAMERS if ent[0]() is not None]
    for ref, ver, nt, prec, nm in _NAMERS:
        if ref() is bank and ver == bank._version and nt == n_top and prec == precision:
            return nm(embeddings, count, scales, bias)
    nm = RegionNamer(bank, n_top, precision)
    _NAMERS.append((weakref.ref(bank), bank._version, n_top, precision, nm))
    del _NAMERS[:-2]
    return nm(embeddings, count, scales, bias)


def class_sharded_retrieval(embeddings: torch.Tensor, count: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor,
                            bank_shard: torch.Tensor, n_classes: int, score_fn: Callable = device_retrieval_scores,
                            group=None) -> torch.Tensor:
    """The large-bank retrieval step of configs[4]: images are sharded over the ranks, and so is the
    text bank — by class, ``bank_shard = shard_bank_by_class(bank, world, rank)`` (a 1M x 768 bank is 384 MB per rank
    at 8 ranks instead of 3 GB).  (1) one all-gather of the kept regions (+ counts, scales, bias); (2) every rank
    scores ALL images against ITS classes — ``score_fn(emb, count, scales, bias, bank_shard) -> [N_total, K_shard]``,
    by default the device kernel; (3) one all-gather of the score blocks.  Returns [N_total, n_classes] on every rank,
    images in global order, classes in bank order.  Shards of unequal size (n_classes % world != 0) are padded to the
    largest for the exchange and trimmed afterwards."""
    if not dist.is_available() or not dist.is_initialized():
        if bank_shard.shape[0] != n_classes:
            raise ValueError("single process: the shard must be the whole bank")
        return score_fn(embeddings, count, scales, bias, bank_shard)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    mine = shard_range(n_classes, world, rank)
    if bank_shard.shape[0] != len(mine):
        raise ValueError(f"rank {rank} holds {bank_shard.shape[0]} classes, shard_range gives {len(mine)}")
    allv = gather_results(dict(e=embeddings, c=count, s=scales, b=bias), group)
    block = score_fn(allv["e"], allv["c"], allv["s"], allv["b"], bank_shard)              # [N_total, len(mine)]
    n_total, widest = block.shape[0], len(shard_range(n_classes, world, 0))
    padded = torch.zeros(n_total, widest, dtype=block.dtype, device=block.device)
    padded[:, : block.shape[1]] = block
    blocks = torch.empty(world * n_total, widest, dtype=block.dtype, device=block.device)
    dist.all_gather_into_tensor(blocks, padded, group=group)
    blocks = blocks.view(world, n_total, widest)
    return torch.cat([blocks[r][:, : len(shard_range(n_classes, world, r))] for r in range(world)], dim=1)


def gather_to_rank0(items: list, group=None) -> Optional[list]:
    """Host objects of every rank (a list each, possibly empty) concatenated in rank order on rank 0 (``None`` on the
    other ranks; the list itself without a process group).  test.py gathers its per-image predictions this way: a few
    KB per image, so a pickled object gather is enough."""
    if not (dist.is_available() and dist.is_initialized()):
        return list(items)
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    out = [None] * world if rank == 0 else None
    dist.gather_object(list(items), out, dst=0, group=group)
    if rank != 0:
        return None
    return [x for part in out for x in part]
