"""Tracking in numpy: the result definition of include/wedetect_hip_track.h restated — predict, the two greedy rounds on the keys
``bits(value) << 32 | (0xFFFF - slot) << 16 | (0xFFFF - row)``, the update, births into the lowest free slot.  Elementwise
arithmetic is fp32, one rounding per operation (numpy never fuses), in the operation order of ``oracle.postprocess._iou_f32`` for
the IoU; the sums over the embedding dimension are float64 (the kernel's fp32 tree is within ``(dim + 16) * 2^-24`` of them for unit
vectors).

``RefTracker.step`` is vectorised and sorts the candidate keys once per round; ``brute=True`` takes the largest free key by a full
scan per pick instead — tests/test_cpu_track.py holds the two equal.  While it runs the reference records the MARGINS a device
comparison needs: the smallest distance of an evaluated value from its threshold, and the smallest distance between a chosen pair
and a competing candidate sharing its slot or row (bit-identical competitors excepted: they tie exactly on the device as well)."""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle.postprocess import _iou_f32

f32 = np.float32
STATUS_FULL, STATUS_BAD_COUNT = 1, 2


@dataclasses.dataclass
class Params:
    high_thr: float = 0.5
    low_thr: float = 0.1
    new_thr: float = 0.6
    match_thr: float = 0.3
    iou2_thr: float = 0.5
    w_iou: float = 0.5
    ema_embed: float = 0.9
    ema_vel: float = 0.5
    max_age: int = 30
    match_labels: bool = False


def margin_needed(dim: int) -> float:
    """What every generated case must keep: the fp32 dot and norm error of unit vectors of ``dim`` elements, with room for the EMA
    history."""
    return (dim + 16) * 2.0 ** -22


def embed_bound(updates: int, dim: int) -> float:
    """Per component of a slot's embedding after ``updates`` writes."""
    return max(updates, 1) * (dim + 16) * 2.0 ** -24


def pack_key(value, slot, row) -> np.ndarray:
    v = np.asarray(value, f32).view(np.uint32).astype(np.uint64)
    return (v << np.uint64(32)) | ((np.uint64(0xFFFF) - np.asarray(slot).astype(np.uint64)) << np.uint64(16)) | \
        (np.uint64(0xFFFF) - np.asarray(row).astype(np.uint64))


def iou_matrix(pred: np.ndarray, det: np.ndarray) -> np.ndarray:
    """fp32 [n_slot, n_row]: the IoU of every predicted box with every row's box, NaN counted as 0."""
    out = np.zeros((pred.shape[0], det.shape[0]), f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(pred.shape[0]):
            out[i] = _iou_f32(pred[i], det)
    out[np.isnan(out)] = 0
    return out


class Seq:
    """The slots of one sequence."""

    def __init__(self, max_tracks: int, dim: int):
        m = max_tracks
        self.id, self.label, self.hits, self.miss = (np.zeros(m, np.int32) for _ in range(4))
        self.has = np.zeros(m, bool)
        self.score = np.zeros(m, f32)
        self.box, self.vel = np.zeros((m, 4), f32), np.zeros((m, 4), f32)
        self.emb = np.zeros((m, dim), f32)
        self.n_upd = np.zeros(m, np.int64)                # writes of the slot's embedding since its birth
        self.next_id, self.status = 1, 0


class RefTracker:
    def __init__(self, n_seq: int, max_tracks: int, dim: int, params=None, brute: bool = False, margins: bool = True):
        self.n_seq, self.max_tracks, self.dim, self.brute = n_seq, max_tracks, dim, brute
        self.margins = margins                            # False: no replay of the picks against their competitors (timing runs)
        self.p = params if params is not None else Params()
        self.seqs = [Seq(max_tracks, dim) for _ in range(n_seq)]
        self.thr_margin = float("inf")                    # evaluated value against its threshold
        self.pick_margin = float("inf")                   # chosen pair against a competitor sharing its slot or row
        self.picks = [0, 0]                               # matches of round 1 / round 2
        self.exact_ties = 0                               # competitors left out because their inputs are bit-identical

    def reset(self, seqs=None) -> None:
        for s in range(self.n_seq) if seqs is None else seqs:
            self.seqs[s] = Seq(self.max_tracks, self.dim)

    @property
    def margin(self) -> float:
        return min(self.thr_margin, self.pick_margin)

    # ------------------------------------------------------------------------------------------------------------ greedy
    def _greedy(self, val, ok, slots, rows, same_slot, same_row):
        """val fp32 [n_slot, n_row], ok the candidate mask; slots / rows the indices that go into the keys.  Returns the list of
        (i, j) picks in pick order.  same_slot(i, i2) / same_row(j, j2): whether two slots / rows have bit-identical inputs."""
        ii, jj = np.nonzero(ok)
        if ii.size == 0:
            return []
        keys = pack_key(val[ii, jj], slots[ii], rows[jj])
        free_i, free_j = np.ones(val.shape[0], bool), np.ones(val.shape[1], bool)
        picks = []
        if self.brute:
            while True:
                live = free_i[ii] & free_j[jj]
                if not live.any():
                    break
                k = int(np.nonzero(live)[0][np.argmax(keys[live])])
                picks.append((int(ii[k]), int(jj[k])))
                free_i[ii[k]] = free_j[jj[k]] = False
        else:
            for k in np.argsort(keys)[::-1]:
                if free_i[ii[k]] and free_j[jj[k]]:
                    picks.append((int(ii[k]), int(jj[k])))
                    free_i[ii[k]] = free_j[jj[k]] = False
        if not self.margins:
            return picks
        # the margins of the picks, replayed in order
        free_i[:], free_j[:] = True, True
        v64 = val.astype(np.float64)
        for i, j in picks:
            col = ok[:, j] & free_i
            col[i] = False
            for i2 in np.nonzero(col)[0]:
                d = abs(v64[i, j] - v64[i2, j])
                if d == 0 and same_slot(i, int(i2)):
                    self.exact_ties += 1
                else:
                    self.pick_margin = min(self.pick_margin, d)
            row = ok[i] & free_j
            row[j] = False
            for j2 in np.nonzero(row)[0]:
                d = abs(v64[i, j] - v64[i, j2])
                if d == 0 and same_row(j, int(j2)):
                    self.exact_ties += 1
                else:
                    self.pick_margin = min(self.pick_margin, d)
            free_i[i] = free_j[j] = False
        return picks

    # ------------------------------------------------------------------------------------------------------------- frame
    def _frame(self, q: Seq, boxes, scores, labels, count, embed):
        p, m = self.p, self.max_tracks
        max_out = boxes.shape[0]
        ids, hits = np.zeros(max_out, np.int32), np.zeros(max_out, np.int32)
        cnt = int(count)
        if cnt < 0:
            q.status |= STATUS_BAD_COUNT
            cnt = 0
        cnt = min(cnt, max_out)
        boxes, scores, labels, embed = boxes[:cnt], scores[:cnt], labels[:cnt], embed[:cnt]
        w_iou, w_app = f32(p.w_iou), f32(f32(1) - f32(p.w_iou))
        ema_e, w_e = f32(p.ema_embed), f32(f32(1) - f32(p.ema_embed))
        ema_v, w_v = f32(p.ema_vel), f32(f32(1) - f32(p.ema_vel))
        live = np.nonzero(q.id > 0)[0]
        pred = (q.box + q.vel).astype(f32)
        with np.errstate(invalid="ignore"):
            hi = np.nonzero(scores >= f32(p.high_thr))[0]
            lo = np.nonzero((scores >= f32(p.low_thr)) & (scores < f32(p.high_thr)))[0]
        # 1 / |e| of the high-score rows; 0 = not usable
        e64 = embed[hi].astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            ss = (e64 * e64).sum(axis=1).astype(f32)
            usable = (ss > 0) & np.isfinite(ss)
            inv_e = np.where(usable, (1.0 / np.sqrt((e64 * e64).sum(axis=1))), 0).astype(f32)
        match = np.full(m, -1, np.int64)                  # row of a matched slot
        mround = np.zeros(m, np.int64)
        row_slot = np.full(max_out, -1, np.int64)
        same_box = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))

        if live.size and hi.size:
            iou = iou_matrix(pred[live], boxes[hi])
            with np.errstate(over="ignore", invalid="ignore"):
                dot = (q.emb[live].astype(np.float64) @ e64.T).astype(f32)
                cos = (dot * inv_e[None, :]).astype(f32)
            cos = np.where(q.has[live][:, None] & usable[None, :], np.maximum(np.nan_to_num(cos, nan=0.0), f32(0)), f32(0)).astype(f32)
            sim = ((w_iou * iou).astype(f32) + (w_app * cos).astype(f32)).astype(f32)
            lab_ok = np.ones(sim.shape, bool) if not p.match_labels else q.label[live][:, None] == labels[hi][None, :]
            if lab_ok.any():
                self.thr_margin = min(self.thr_margin, float(np.abs(sim[lab_ok].astype(np.float64) - float(f32(p.match_thr))).min()))
            ok = (sim >= f32(p.match_thr)) & lab_ok

            def same_slot(a, b):
                sa, sb = live[a], live[b]
                return same_box(pred[sa], pred[sb]) and q.has[sa] == q.has[sb] and (not q.has[sa] or same_box(q.emb[sa], q.emb[sb]))

            def same_row(a, b):
                ra, rb = hi[a], hi[b]
                return same_box(boxes[ra], boxes[rb]) and same_box(embed[ra], embed[rb])
            for i, j in self._greedy(sim, ok, live, hi, same_slot, same_row):
                match[live[i]], mround[live[i]], row_slot[hi[j]] = hi[j], 1, live[i]
                self.picks[0] += 1

        rest = np.array([s for s in live if match[s] < 0 and q.miss[s] == 0], np.int64)
        if rest.size and lo.size:
            iou = iou_matrix(pred[rest], boxes[lo])
            lab_ok = np.ones(iou.shape, bool) if not p.match_labels else q.label[rest][:, None] == labels[lo][None, :]
            if lab_ok.any():
                self.thr_margin = min(self.thr_margin, float(np.abs(iou[lab_ok].astype(np.float64) - float(f32(p.iou2_thr))).min()))
            ok = (iou >= f32(p.iou2_thr)) & lab_ok
            for i, j in self._greedy(iou, ok, rest, lo, lambda a, b: same_box(pred[rest[a]], pred[rest[b]]),
                                     lambda a, b: same_box(boxes[lo[a]], boxes[lo[b]])):
                match[rest[i]], mround[rest[i]], row_slot[lo[j]] = lo[j], 2, rest[i]
                self.picks[1] += 1

        inv_of = dict(zip(hi.tolist(), inv_e.tolist()))
        for s in live:
            r = int(match[s])
            if r >= 0:
                d = (boxes[r] - q.box[s]).astype(f32)
                q.vel[s] = ((ema_v * q.vel[s]).astype(f32) + (w_v * d).astype(f32)).astype(f32)
                q.box[s], q.label[s], q.score[s] = boxes[r], labels[r], scores[r]
                q.hits[s] += 1
                q.miss[s] = 0
                if mround[s] == 1 and inv_of[r] > 0:
                    eh = (embed[r] * f32(inv_of[r])).astype(f32)
                    if q.has[s]:
                        v = ((ema_e * q.emb[s]).astype(f32) + (w_e * eh).astype(f32)).astype(f32)
                        ss = float((v.astype(np.float64) ** 2).sum())
                        if f32(ss) > 0 and np.isfinite(f32(ss)):
                            q.emb[s] = (v * f32(1.0 / np.sqrt(ss))).astype(f32)
                            q.n_upd[s] += 1
                    else:
                        q.emb[s], q.has[s] = eh, True
                        q.n_upd[s] += 1
            else:
                q.box[s] = pred[s]
                q.miss[s] += 1
                if q.miss[s] > p.max_age:
                    q.id[s] = 0
        for r in hi:
            if row_slot[r] >= 0 or not scores[r] >= f32(p.new_thr):
                continue
            free = np.nonzero(q.id == 0)[0]
            if free.size == 0:
                q.status |= STATUS_FULL
                break
            s = int(free[0])
            q.id[s], q.next_id = q.next_id, q.next_id + 1
            q.label[s], q.score[s], q.box[s], q.vel[s] = labels[r], scores[r], boxes[r], 0
            q.hits[s], q.miss[s], q.has[s], q.n_upd[s] = 1, 0, False, 0
            if inv_of[int(r)] > 0:
                q.emb[s], q.has[s], q.n_upd[s] = (embed[r] * f32(inv_of[int(r)])).astype(f32), True, 1
            row_slot[r] = s
        for r in range(cnt):
            if row_slot[r] >= 0:
                ids[r], hits[r] = q.id[row_slot[r]], q.hits[row_slot[r]]
        return ids, hits

    def step(self, boxes, scores, labels, count, embed, n_frame: int):
        """boxes fp32 [n_img, max_out, 4], scores fp32 / labels int32 [n_img, max_out], count int32 [n_img], embed fp32
        [n_img, max_out, dim] with n_img = n_seq * n_frame -> track_ids, track_hits int32 [n_img, max_out]."""
        boxes, scores, embed = np.asarray(boxes, f32), np.asarray(scores, f32), np.asarray(embed, f32)
        labels, count = np.asarray(labels, np.int32), np.asarray(count, np.int32)
        n_img, max_out = scores.shape
        assert n_img == self.n_seq * n_frame
        ids, hits = np.zeros((n_img, max_out), np.int32), np.zeros((n_img, max_out), np.int32)
        for s in range(self.n_seq):
            for f in range(n_frame):
                b = s * n_frame + f
                ids[b], hits[b] = self._frame(self.seqs[s], boxes[b], scores[b], labels[b], count[b], embed[b])
        return ids, hits

    def export(self) -> dict:
        """What wd_track_export writes: a free slot's fields are 0."""
        k = lambda name, dt: np.stack([np.where(q.id > 0, getattr(q, name), 0).astype(dt) for q in self.seqs])
        lv = np.stack([q.id > 0 for q in self.seqs])
        return dict(ids=k("id", np.int32), labels=k("label", np.int32), hits=k("hits", np.int32), misses=k("miss", np.int32),
                    scores=k("score", f32), boxes=np.where(lv[:, :, None], np.stack([q.box for q in self.seqs]), f32(0)),
                    vel=np.where(lv[:, :, None], np.stack([q.vel for q in self.seqs]), f32(0)),
                    embed=np.stack([q.emb * (q.has & (q.id > 0))[:, None] for q in self.seqs]),
                    n_upd=np.stack([q.n_upd for q in self.seqs]),
                    seq_info=np.array([[q.next_id, int((q.id > 0).sum()), q.status, 0] for q in self.seqs], np.int32))
