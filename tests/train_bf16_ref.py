"""The numerics contract of bf16 mixed-precision training of a hidden block (include/c4a0_hip.h, "bf16 mixed-precision training"),
restated in float64 numpy (test infrastructure).  `bf16_round` is round to nearest, ties to even, in integer arithmetic on the f32 bit
pattern; it is applied at exactly the points the contract lists and nowhere else.  Every other operation is float64: the reference
does not model the f32 accumulation, so it equals the kernels bit for bit only where every partial sum is exact in f32 (the
exact-integer tests) and is otherwise what their error is measured against."""
import numpy as np


def bf16_round(a) -> np.ndarray:
    """f32 values -> the bf16 value each rounds to (nearest, ties to even), as f32.  Integer arithmetic on the bit pattern: the low
    16 bits are dropped after adding 0x7FFF plus the lowest kept bit; a value past the largest finite bf16 becomes an infinity, an
    infinity stays, a NaN becomes a quiet NaN of its sign."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    r = np.where(nan, (u & 0x80000000) | 0x7FC00000, r)
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def bf16_bits(a) -> np.ndarray:
    """the 16-bit pattern of bf16_round(a)"""
    return (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


def r64(a) -> np.ndarray:
    """float64 -> bf16 (through f32, as the kernels round an f32 value), as float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        return bf16_round(np.asarray(a, dtype=np.float64).astype(np.float32)).astype(np.float64)


def passes(pre: np.ndarray) -> np.ndarray:
    """ReLU's predicate !(pre <= 0): a NaN passes"""
    with np.errstate(invalid="ignore"):
        return ~(pre <= 0)


def linear(xb, wb, bias=None) -> np.ndarray:
    """bf16(sum_k xb[r][k] wb[j][k] + bias[j]) of bf16-valued operands"""
    acc = np.asarray(xb, dtype=np.float64) @ np.asarray(wb, dtype=np.float64).T
    return r64(acc if bias is None else acc + np.asarray(bias, dtype=np.float64))


def bn_forward(z, gamma, beta, eps: float) -> dict:
    """steps 4-6 of the forward on bf16-valued z; `y32` is relu(pre) before the rounding"""
    z, gamma, beta = (np.asarray(t, dtype=np.float64) for t in (z, gamma, beta))
    with np.errstate(over="ignore", invalid="ignore"):
        mean = z.mean(0)
        var = ((z - mean) ** 2).mean(0)
        rstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
        xh = (z - mean) * rstd
        pre = xh * gamma + beta
        y32 = np.where(passes(pre), pre, 0.0)
    return {"mean": mean, "var": var, "rstd": rstd, "xh": xh, "pre": pre, "y32": y32, "y": r64(y32)}


def bn_backward(dy, z, gamma, beta, eps: float) -> dict:
    """steps 1-5 of the backward from bf16-valued dy and z"""
    f = bn_forward(z, gamma, beta, eps)
    gamma, m = np.asarray(gamma, dtype=np.float64), np.shape(z)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(passes(f["pre"]), np.asarray(dy, dtype=np.float64), 0.0)
        dbeta, dgamma = g.sum(0), (g * f["xh"]).sum(0)
        dz32 = gamma * f["rstd"] * ((g - dbeta / m) - f["xh"] * (dgamma / m))
        out = {"g": g, "dbeta": dbeta, "dgamma": dgamma, "dz32": dz32, "db": dz32.sum(0), "dz": r64(dz32)}
    out.update(f)
    return out


def block(x, w, b, gamma, beta, eps: float, dy=None, x_is_bf16: bool = False) -> dict:
    """The whole block: forward, and from dy (rounded once if it is not bf16-valued) the backward."""
    xb = np.asarray(x, dtype=np.float64) if x_is_bf16 else r64(x)
    wb = r64(w)
    z = linear(xb, wb, b)
    out = {"xb": xb, "wb": wb, "z": z}
    if dy is None:
        out.update(bn_forward(z, gamma, beta, eps))
        return out
    out.update(bn_backward(r64(dy), z, gamma, beta, eps))
    out["dx"] = r64(out["dz"] @ wb)
    out["dw"] = r64(out["dz"].T @ xb)
    return out
