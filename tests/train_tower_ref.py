"""A float64 numpy restatement of the four operations of the training tower (c4a0_amd/csrc/c4_train_tower.hip, include/c4a0_hip.h
"training the convolution tower") in the kernels' own layout: activations cell-major [42 B][C], weights packed as pack_f32_weights
packs them (w0 [C][32] with k = 2 tap + ci, w [C][9 C] with k = tap C + ci, tap = 3 (dr + 1) + (dc + 1)), dgrad as the forward
convolution with the tap-flipped weights.  tests/test_train_tower_ref.py pins it to float64 F.conv2d / F.batch_norm and their
autograd; the GPU tests hold the kernels to it.  No GPU, no torch."""
import numpy as np

ROWS, COLS, CELLS = 6, 7, 42


def im2col3x3(x: np.ndarray) -> np.ndarray:
    """x [42 B][C] -> X [42 B][9 C]: X[(b, cell)][tap C + ci] = x at the neighbour (row + tap // 3 - 1, col + tap % 3 - 1), 0 off the board"""
    c = x.shape[1]
    b = x.shape[0] // CELLS
    pad = np.zeros((b, ROWS + 2, COLS + 2, c), dtype=x.dtype)
    pad[:, 1:-1, 1:-1] = x.reshape(b, ROWS, COLS, c)
    taps = [pad[:, tap // 3:tap // 3 + ROWS, tap % 3:tap % 3 + COLS] for tap in range(9)]
    return np.stack(taps, axis=3).reshape(b * CELLS, 9 * c)


def im2col0(planes: np.ndarray) -> np.ndarray:
    """planes [B][2][6][7] -> X [42 B][32]: X[(b, cell)][2 tap + ci], columns 18..31 zero"""
    b = planes.shape[0]
    x = im2col3x3(planes.transpose(0, 2, 3, 1).reshape(b * CELLS, 2))
    return np.concatenate([x, np.zeros((b * CELLS, 14), dtype=planes.dtype)], axis=1)


def pack_conv0(weight: np.ndarray) -> np.ndarray:
    """[C][2][3][3] -> w0 [C][32]"""
    c = weight.shape[0]
    w0 = np.zeros((c, 32), dtype=weight.dtype)
    w0[:, :18] = weight.reshape(c, 2, 9).transpose(0, 2, 1).reshape(c, 18)
    return w0


def unpack_conv0(w0: np.ndarray) -> np.ndarray:
    c = w0.shape[0]
    return w0[:, :18].reshape(c, 9, 2).transpose(0, 2, 1).reshape(c, 2, 3, 3)


def pack_conv3x3(weight: np.ndarray) -> np.ndarray:
    """[co][ci][3][3] -> w [co][tap C + ci]"""
    co, ci = weight.shape[:2]
    return np.ascontiguousarray(weight.reshape(co, ci, 9).transpose(0, 2, 1).reshape(co, 9 * ci))


def unpack_conv3x3(w: np.ndarray) -> np.ndarray:
    c = w.shape[0]
    return w.reshape(c, 9, c).transpose(0, 2, 1).reshape(c, c, 3, 3)


def flip_for_dgrad(w: np.ndarray) -> np.ndarray:
    """packed w [co][tap C + ci] -> W'[ci][(8 - tap) C + co]"""
    c = w.shape[0]
    return np.ascontiguousarray(w.reshape(c, 9, c)[:, ::-1, :].transpose(2, 1, 0).reshape(c, 9 * c))


def conv0(planes, w0, bias):
    return im2col0(planes) @ w0.T + bias


def conv3x3(x, w, bias):
    return im2col3x3(x) @ w.T + bias


def dgrad(dz, w):
    """da[cell][ci] = sum_tap sum_co dz[cell - offset(tap)][co] W[co][tap][ci]"""
    return im2col3x3(dz) @ flip_for_dgrad(w).T


def wgrad(dz, cols):
    """(dW [C][K], db [C]) from dz [m][C] and the im2col matrix [m][K] of the convolution's input"""
    return dz.T @ cols, dz.sum(0)


def bn2d_relu_res(z, a, gamma, beta, eps, dy=None):
    """y = a + relu(bn(z)) over the rows with batch statistics; with dy also dz, dgamma, dbeta (the gradient of a is dy)"""
    m = z.shape[0]
    mean, var = z.mean(0), z.var(0)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (z - mean) * rstd
    pre = xh * gamma + beta
    out = {"mean": mean, "var": var, "pre": pre, "y": a + np.maximum(pre, 0.0)}
    if dy is not None:
        g = np.where(pre > 0, dy, 0.0)
        out["dbeta"], out["dgamma"] = g.sum(0), (g * xh).sum(0)
        out["dz"] = gamma * rstd * (g - out["dbeta"] / m - xh * out["dgamma"] / m)
    return out


def to_nchw(x: np.ndarray) -> np.ndarray:
    """cell-major [42 B][C] -> [B][C][6][7]"""
    b = x.shape[0] // CELLS
    return np.ascontiguousarray(x.reshape(b, ROWS, COLS, -1).transpose(0, 3, 1, 2))


def from_nchw(x: np.ndarray) -> np.ndarray:
    b, c = x.shape[:2]
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1).reshape(b * CELLS, c))
