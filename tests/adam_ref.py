"""include/c4a0_hip.h's "training: the optimiser" restated in float64 numpy (test infrastructure): Adam with coupled L2 as
`c4_train_adam_f32` computes it, every operation in real-number order and none of the f32 roundings.  tests/test_train_adam_ref.py
pins it to `torch.optim.Adam` in float64; tests/test_gpu_train_adam.py judges the kernel against it."""
import numpy as np


def pow_u32(b: float, e: int) -> float:
    """b^e by square-and-multiply from the lowest bit, as the kernel takes it"""
    r = 1.0
    while e:
        if e & 1:
            r *= b
        b *= b
        e >>= 1
    return r


def adam_step(p, g, m, v, t_before: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0):
    """One call on one segment: (p', m', v') in float64 from the state (p, m, v), the gradient g and the device's step count BEFORE
    the call; the call computes step t = t_before + 1."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    t = t_before + 1
    bc1, bc2 = 1.0 - pow_u32(beta1, t), 1.0 - pow_u32(beta2, t)
    step_size, sqrt_bc2 = lr / bc1, np.sqrt(bc2)
    with np.errstate(all="ignore"):
        g2 = g + weight_decay * p if weight_decay != 0.0 else g
        m2 = m + (1.0 - beta1) * (g2 - m)
        v2 = ((1.0 - beta2) * g2) * g2 + beta2 * v
        p2 = p - step_size * (m2 / (np.sqrt(v2) / sqrt_bc2 + eps))
    return p2, m2, v2


def adam_steps(p, grads, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0):
    """len(grads) calls from a fresh state (m = v = 0, count 0): (p, m, v) after the last"""
    p = np.asarray(p, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads):
        p, m, v = adam_step(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay)
    return p, m, v
