"""The plain-C reference of the f32 evaluator (tests/f32_net_ref.c, built here with gcc -ffp-contract=off) and a forward
pass composed from it: every intermediate the GPU chain exposes, in the same padded layouts."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import torch

from c4a0_amd.nn import InferenceNet, pack_f32_weights

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="f32ref"), "libf32ref.so")
        cmd = ["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-shared", "-fPIC",
               os.path.join(HERE, "f32_net_ref.c"), "-o", out, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = C.CDLL(out)
        fp, i = C.c_void_p, C.c_int
        L.f32ref_linear.argtypes = [fp, i, fp, fp, fp, i, i, i, i, i]
        L.f32ref_conv0.argtypes = [fp, i, i, fp, fp, fp]
        L.f32ref_conv.argtypes = [fp, i, i, fp, fp, fp, fp]
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def pack_on_cpu(model) -> dict:
    """pack_f32_weights of the BN-folded model (folded by InferenceNet on the CPU, the PyTorch path), as numpy arrays."""
    net = InferenceNet(model, torch.device("cpu"), dtype=torch.float32)
    pk = pack_f32_weights([w.contiguous() for w in net.conv_w], net.conv_b, net.pol_w, net.pol_b, net.val_w, net.val_b, net.channels)
    out = {k: (v.numpy() if isinstance(v, torch.Tensor) else ([t.numpy() for t in v] if isinstance(v, list) else v)) for k, v in pk.items()}
    out["n_blocks"] = net.n_blocks
    return out


def linear(x, w, b, act):
    x, w, b = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, b))
    y = np.empty((x.shape[0], w.shape[0]), np.float32)
    ref_lib().f32ref_linear(_p(x), x.shape[1], _p(w), _p(b), _p(y), y.shape[1], x.shape[0], w.shape[0], w.shape[1], int(act))
    return y


def forward(pk: dict, planes: np.ndarray) -> dict:
    """planes f32 [G, 2, 6, 7] -> {"features" [G, 42 Cp], "policy_hidden" / "value_hidden" [list of [G, Hp]], "preact" [G, 9]}."""
    L = ref_lib()
    planes = np.ascontiguousarray(planes, dtype=np.float32)
    g, cp = planes.shape[0], pk["cp"]
    x = np.empty((g, 42 * cp), np.float32)
    L.f32ref_conv0(_p(planes), g, cp, _p(pk["w0"]), _p(pk["bias"][0]), _p(x))
    t = np.empty_like(x)
    for i in range(pk["n_blocks"]):
        L.f32ref_conv(_p(x), g, cp, _p(np.ascontiguousarray(pk["w"][2 * i])), _p(np.ascontiguousarray(pk["bias"][1 + 2 * i])), _p(t), None)
        L.f32ref_conv(_p(t), g, cp, _p(np.ascontiguousarray(pk["w"][2 * i + 1])), _p(np.ascontiguousarray(pk["bias"][2 + 2 * i])), _p(x), _p(x))
    res = {"features": x}
    for name, key in (("policy", "pol"), ("value", "val")):
        h, hidden = x, []
        for w, b in zip(pk[key + "_w"][:-1], pk[key + "_b"][:-1]):
            h = linear(h, w, b, 1)
            hidden.append(h)
        res[name + "_hidden"] = hidden
        res[name + "_out"] = linear(h, pk[key + "_w"][-1], pk[key + "_b"][-1], 0)
    res["preact"] = np.concatenate([res["policy_out"], res["value_out"]], axis=1)
    return res


def log_softmax_documented(v: np.ndarray, expf, logf) -> np.ndarray:
    """The documented log-softmax on f32 pre-activations [G, 7] with the given expf / logf (arrays in, arrays out)."""
    v = v.astype(np.float32)
    mx = v[:, 0].copy()
    for o in range(1, 7):
        mx = np.maximum(mx, v[:, o])
    e = expf(np.ascontiguousarray(v - mx[:, None]).reshape(-1)).reshape(v.shape)
    sm = np.zeros(v.shape[0], np.float32)
    for o in range(7):
        sm = (sm + e[:, o]).astype(np.float32)
    lse = (mx + logf(sm)).astype(np.float32)
    return (v - lse[:, None]).astype(np.float32)
