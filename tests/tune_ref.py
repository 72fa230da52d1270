"""Bank tuning in numpy: the result definition of include/wedetect_hip_tune.h restated — the static targets, the loss and its
gradient through the row normalisation, the Adam step with frozen rows — in float64 (``dtype=np.float32`` evaluates the same
formulas in plain fp32: the yardstick the kernel's rounding error is measured against)."""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64
DIM, CLASS_BLOCK, ROW_TILE, MAX_SPLIT = 768, 32, 128, 256


def level_of(anchor, off1: int, off2: int):
    return (np.asarray(anchor) >= off1).astype(np.int64) + (np.asarray(anchor) >= off2).astype(np.int64)


def row_consts(rows: int, n_anchor: int, off1: int, off2: int, scale, bias, dtype=f64):
    """a_r, b_r of rows 0 .. rows - 1: row r is anchor r % n_anchor."""
    lv = level_of(np.arange(rows) % n_anchor, off1, off2)
    return np.asarray(scale, dtype)[lv], np.asarray(bias, dtype)[lv]


def targets(sel_anchors, sel_iou, ex_cls, m: int, n_anchor: int):
    """sel_anchors int32 / sel_iou fp32 [B, max_ex * m] (wd_exemplar_assign), ex_cls int32 [B, max_ex] -> pos_cls int32 [B, n_anchor],
    pos_y fp32 [B, n_anchor]: an anchor keeps the claim with the larger IoU, ties going to the lower slot; others (-1, 0)."""
    sel_anchors, sel_iou, ex_cls = np.asarray(sel_anchors), np.asarray(sel_iou, f32), np.asarray(ex_cls)
    B, S = sel_anchors.shape
    pos_cls, pos_y = np.full((B, n_anchor), -1, np.int32), np.zeros((B, n_anchor), f32)
    for b in range(B):
        claimed = np.zeros(n_anchor, bool)
        for i in range(S):                                       # ascending slots: a later slot wins only with a LARGER IoU
            a = int(sel_anchors[b, i])
            if 0 <= a < n_anchor and (not claimed[a] or sel_iou[b, i] > pos_y[b, a]):
                claimed[a], pos_cls[b, a], pos_y[b, a] = True, ex_cls[b, i // m], sel_iou[b, i]
    return pos_cls, pos_y


def norm_of(chunks) -> float:
    """max(sum of pos_y over all chunks, 1)."""
    return max(float(sum(np.asarray(c["pos_y"], f64).sum() for c in chunks)), 1.0)


def chunk_dt(c, T, inv_norm, dtype=f64):
    """One chunk: (sum of bce / norm, dt [K, 768]) with dt_k = sum_r a_r g[r,k] E_r."""
    E = np.asarray(c["E"], dtype)
    rows, K = E.shape[0], T.shape[0]
    a, b = row_consts(rows, c["n_anchor"], c["off1"], c["off2"], c["scale"], c["bias"], dtype)
    pc, py = np.asarray(c["pos_cls"]).reshape(-1), np.asarray(c["pos_y"], dtype).reshape(-1)
    z = (a[:, None] * (E @ T.T.astype(dtype)) + b[:, None]).astype(dtype)
    y = np.zeros((rows, K), dtype)
    hit = (pc >= 0) & (pc < K)
    y[np.nonzero(hit)[0], pc[hit]] = py[hit]
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(dtype)
    bce = np.maximum(z, 0) - z * y + np.log1p(e)
    g = ((p - y) * dtype(inv_norm)).astype(dtype)
    return bce.sum(dtype=dtype) * dtype(inv_norm), ((a[:, None] * g).astype(dtype)).T @ E


def loss_grad(chunks, W, norm=None, dtype=f64):
    """loss, dt [K, 768], dW [K, 768] and the unit rows T over all chunks."""
    W = np.asarray(W, dtype)
    nrm = np.sqrt((W * W).sum(axis=1, keepdims=True))
    T = W / nrm
    inv = 1.0 / (norm_of(chunks) if norm is None else norm)
    loss, dt = dtype(0), np.zeros_like(W)
    for c in chunks:
        l, d = chunk_dt(c, T, inv, dtype)
        loss, dt = loss + l, dt + d
    dW = (dt - (dt * T).sum(axis=1, keepdims=True) * T) / nrm
    return loss, dt, dW, T


def loss_of(chunks, W, norm=None) -> float:
    return float(loss_grad(chunks, W, norm)[0])


def adam_step(W, m, v, dW, t: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, trainable=None):
    """One Adam step without weight decay on the rows with a non-zero ``trainable`` byte -> W, m, v, T (float64)."""
    W, m, v, dW = (np.array(x, f64) for x in (W, m, v, dW))
    tr = np.ones(W.shape[0], bool) if trainable is None else np.asarray(trainable).astype(bool)
    b1, b2 = betas
    m2, v2 = b1 * m + (1 - b1) * dW, b2 * v + (1 - b2) * dW * dW
    W2 = W - lr * (m2 / (1 - b1 ** t)) / (np.sqrt(v2 / (1 - b2 ** t)) + eps)
    for x, x2 in ((W, W2), (m, m2), (v, v2)):
        x[tr] = x2[tr]
    return W, m, v, W / np.sqrt((W * W).sum(axis=1, keepdims=True))


def plan(rows: int, n_cls: int) -> int:
    """wd_tune_plan."""
    if rows <= 0 or n_cls <= 0:
        return 0
    return min(-(-rows // ROW_TILE), max(1, MAX_SPLIT // -(-n_cls // CLASS_BLOCK)))


def split_rows(rows: int, n_split: int, s: int):
    """Rows [lo, hi) of split s: whole tiles of 128 rows."""
    nt = -(-rows // ROW_TILE)
    return min(s * nt // n_split * ROW_TILE, rows), min((s + 1) * nt // n_split * ROW_TILE, rows)


def grad_rel_err(G, G64) -> np.ndarray:
    """Per class: ||G - G64||_2 / ||G64||_2."""
    G, G64 = np.asarray(G, f64), np.asarray(G64, f64)
    return np.sqrt(((G - G64) ** 2).sum(axis=1)) / np.sqrt((G64 ** 2).sum(axis=1))


def loss_bound(loss64: float, rows: int, n_cls: int, n_split: int, n_parts: int, z_err: float, inv_norm: float) -> float:
    """|kernel loss - float64| for chunks of at most ``rows`` rows.  Summation: every term is positive, so no partial sum exceeds
    the loss itself, and each level of a sum costs at most one rounding of a partial sum: the sequential fp32 chain of
    16 * ceil(ceil(rows / 128) / n_split) terms per lane (the header), 6 + 3 tree levels, wd_tune_update's chain of
    ceil(n_parts / 256) terms and its 6 + 3 levels, and 8 more for the few-ulp evaluation of a term and the final scaling.
    Logits: |d bce / dz| <= 1, so an fp32 logit that is off by at most ``z_err`` (the caller: max_r a_r * ||E_r|| * 101 * 2^-24:
    eight fmaf chains of 96 dimensions of a unit row, three tree levels, then scale and bias) moves the loss by at most rows * K * z_err / norm per
    chunk; ``rows`` is then the total over the chunks."""
    tiles = -(-(-(-rows // ROW_TILE)) // n_split)
    levels = 16 * tiles + 9 + -(-n_parts // 256) + 9 + 8
    return levels * 2.0 ** -24 * abs(loss64) + rows * n_cls * z_err * inv_norm
