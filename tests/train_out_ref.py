"""A float64 numpy restatement of include/c4a0_hip.h's "training: the output layers and the loss": the forward (out, dz, losses) and the
backward (dx, dW, db) of the heads' output layers and `train_common.loss`, with the reductions over rows chunked as the header says --
per chunk of CHUNK rows one sum in ascending row order, then the second stage over the chunks (eight groups, then the groups in
order).  In float64 the orders change nothing a test could see; they are written down so that the structure is the kernels'."""
import numpy as np

CHUNK = 64     # C4_TRAIN_OUT_CHUNK_ROWS
GROUPS = 8
EPS = 1e-8


def work_bytes(m: int, k: int) -> int:
    """the header's formula for c4_train_out_work_bytes"""
    n_chunks = (m + CHUNK - 1) // CHUNK
    return 4 * max(4 * m + 4 * n_chunks, n_chunks * (9 * k + 12))


def chunk_sums(rows: np.ndarray) -> np.ndarray:
    """rows [m, ...] -> [n_chunks, ...]: each chunk's rows added in ascending order from 0"""
    m = rows.shape[0]
    out = []
    for r0 in range(0, m, CHUNK):
        s = np.zeros(rows.shape[1:], dtype=np.float64)
        for r in range(r0, min(m, r0 + CHUNK)):
            s = s + rows[r]
        out.append(s)
    return np.stack(out)


def second_stage(part: np.ndarray) -> np.ndarray:
    """part [n_chunks, ...]: group g adds the chunks g, g + 8, .. in order from its first chunk; then ((G_0 + G_1) + ..)"""
    n = part.shape[0]
    total = None
    for g in range(min(GROUPS, n)):
        s = part[g]
        for c in range(g + GROUPS, n, GROUPS):
            s = s + part[c]
        total = s if total is None else total + s
    return total


def row_sum(rows: np.ndarray) -> np.ndarray:
    return second_stage(chunk_sums(np.asarray(rows, dtype=np.float64)))


def forward(xp, xv, wp, bp, wv, bv, t, tp, tn):
    """-> out [m, 9], dz [m, 9] (the gradient of total at the pre-activations for an upstream gradient of 1), losses [4]"""
    xp, xv, wp, bp, wv, bv, t, tp, tn = (np.asarray(a, dtype=np.float64) for a in (xp, xv, wp, bp, wv, bv, t, tp, tn))
    m = xp.shape[0]
    z = xp @ wp.T + bp
    u = xv @ wv.T + bv
    zs = z - z.max(axis=1, keepdims=True)
    logp = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
    q = np.tanh(u)
    t1 = t + EPS
    kl_rows = (t1 * (np.log(t1) - logp)).sum(axis=1)
    d = q - np.stack([tp, tn], axis=1)
    kl, pen, nopen = row_sum(kl_rows) / m, row_sum(d[:, 0] ** 2) / m, row_sum(d[:, 1] ** 2) / m
    losses = np.array([(kl + pen) + nopen, kl, pen, nopen])
    dz = np.empty((m, 9))
    dz[:, :7] = (np.exp(logp) * t1.sum(axis=1, keepdims=True) - t1) / m
    dz[:, 7:] = 2.0 * d * (1.0 - q * q) / m
    return np.concatenate([logp, q], axis=1), dz, losses


def backward(dz, scale, xp, xv, wp, wv):
    """-> dxp, dxv, dwp, dbp, dwv, dbv"""
    dz, xp, xv, wp, wv = (np.asarray(a, dtype=np.float64) for a in (dz, xp, xv, wp, wv))
    scale = float(scale)
    gp, gv = dz[:, :7], dz[:, 7:]
    dxp, dxv = (gp @ wp) * scale, (gv @ wv) * scale
    dwp = row_sum(gp[:, :, None] * xp[:, None, :]) * scale
    dwv = row_sum(gv[:, :, None] * xv[:, None, :]) * scale
    return dxp, dxv, dwp, row_sum(gp) * scale, dwv, row_sum(gv) * scale
