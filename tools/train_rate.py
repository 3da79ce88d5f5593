"""The training kernels of the heads' hidden blocks beside the stock PyTorch ops, on the GPU -> profiles/train_rate.json.

    python tools/train_rate.py [out.json] [--no-generation] [--max-epochs E] [--bf16 | --graph | --tower | --outputs]

(a) At m = 2 000 rows, F = 1 344 (the default network's heads at the reference's training batch): every kernel of c4_train.hip and
    the forward c4_linear_f32 beside the PyTorch op that does the same job on the same tensors -- F.linear, dz @ W, dz.T @ x (+ the
    column sum for db), F.batch_norm(training=True) + ReLU forward and their autograd backward.  Device events round 20 launches,
    warmed up, the two sides ALTERNATING, medians of 7 pairs with their spreads.
(b) The whole optimiser step (forward_train, loss, backward, Adam) of the default network ModelConfig(1, 32, 4, 2) at batch 2 000 with
    heads="hip" against heads="torch", same timing scheme round 5 steps.  `c4a0_amd.train_heads.AUTO_HEADS` (what heads="auto" means)
    is the faster of the two in the recorded file.
(c) One default-shaped generation through train_single_gen (1 700 games, n = 1 400, batch 2 000; --max-epochs, default 10, instead
    of the reference's 100 so that the run stays short: train_s scales with the epochs run): wall seconds of play / split / train.
(d) --bf16: the opt-in heads="bf16" path alone -> profiles/train_rate_bf16.json.  At the same shape every kernel of c4_train_bf16.hip
    and each of the three c4_linear_bf16 products (forward, dgrad, wgrad) beside the stock op on the same tensors; one hidden block
    forward + backward and the whole optimiser step with heads="bf16", heads="torch" and torch.autocast(bfloat16) on the stock module
    (autocast also runs the tower's convolutions in bf16, which heads="bf16" does not), each callable timed in turn, medians of 7 rounds.
(e) --graph: training from a captured HIP graph -> profiles/train_rate_graph.json.  c4_train_adam_f32 on the default network's parameters
    beside torch.optim.Adam.step() on the same parameters, with the bytes a second it reaches against the 28 bytes a parameter it must
    move; the whole step for heads in {torch, hip, bf16} x {eager torch.optim.Adam (the stock loop), eager HipAdam, graph replay}, all
    nine callables timed in turn; and the default-shaped generation of (c) with graph=True beside graph=False for each head path.
(f) --tower: the opt-in tower="hip" path -> profiles/train_rate_tower.json.  At ModelConfig(1, 32, 4, 2), batch 2 000 (84 000 rows of 32
    channels): each call of c4_train_tower.hip beside the stock op it replaces on the same values (the stock side in its own NCHW layout);
    the tower's forward + backward alone, stock against train_tower.tower_forward; and the whole step for heads in {torch, bf16} x
    tower in {torch, hip}, eager with HipAdam and as a graph replay, beside the stock loop (torch.optim.Adam), all timed in turn.
(g) --outputs: the opt-in outputs="hip" path -> profiles/train_rate_outputs.json.  At m = 2 000, k = 1 344, from f32 and from bf16
    activations: the forward and the backward call of c4_train_out.hip beside the stock ops they replace on the same values, timed as one
    group (F.linear x 2, log_softmax, tanh, loss and their autograd); and the whole step for heads in {torch, bf16} x outputs in
    {torch, hip}, as a graph replay and eager with HipAdam, all timed in turn.
Speed is recorded here, never asserted in a test."""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c4a0_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")
p = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
M, FEAT, EPS = 2000, 1344, 1e-5


def time_us(fn, launches=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


def ab(fa, fb, pairs=7, launches=20):
    """medians (us per call) of `pairs` alternating timings of two callables, and their spreads"""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(pairs):
        ta.append(time_us(fa, launches))
        tb.append(time_us(fb, launches))
    return {"hip_us": statistics.median(ta), "torch_us": statistics.median(tb), "hip_range_us": [min(ta), max(ta)], "torch_range_us": [min(tb), max(tb)]}


def kernels():
    L = _lib.lib()
    g = torch.Generator().manual_seed(0)
    m, n, k = M, FEAT, FEAT
    x, dz, dy = (torch.randn(m, FEAT, generator=g).to(dev) for _ in range(3))
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(dev)
    b, gamma, beta = torch.randn(n, generator=g).to(dev), (torch.rand(n, generator=g) + 0.5).to(dev), torch.randn(n, generator=g).to(dev)
    z, y, dx, dzo = (torch.empty((m, n), device=dev) for _ in range(4))
    dw = torch.empty((n, k), device=dev)
    mean, var, db, dgamma, dbeta = (torch.empty(n, device=dev) for _ in range(5))
    ck = _lib.check
    out = {}
    flop = 2.0 * m * n * k
    out["linear_fwd"] = ab(lambda: ck(L.c4_linear_f32(p(x), p(w), p(b), p(z), m, n, k, k, n, 0, stream())), lambda: F.linear(x, w, b))
    out["dgrad"] = ab(lambda: ck(L.c4_train_linear_dgrad_f32(p(dz), p(w), p(dx), m, n, k, n, k, stream())), lambda: dz @ w)
    out["wgrad"] = ab(lambda: ck(L.c4_train_linear_wgrad_f32(p(dz), p(x), p(dw), p(db), m, n, k, n, k, stream())), lambda: (dz.t() @ x, dz.sum(0)))
    for name in ("linear_fwd", "dgrad", "wgrad"):
        out[name]["hip_tflops"] = flop / out[name]["hip_us"] * 1e-6
        out[name]["torch_tflops"] = flop / out[name]["torch_us"] * 1e-6
    ck(L.c4_linear_f32(p(x), p(w), p(b), p(z), m, n, k, k, n, 0, stream()))
    out["bn_relu_fwd"] = ab(lambda: ck(L.c4_train_bn_relu_fwd_f32(p(z), p(gamma), p(beta), EPS, m, n, n, n, p(y), p(mean), p(var), stream())),
                            lambda: torch.relu(F.batch_norm(z, None, None, gamma, beta, True, 0.1, EPS)))
    zt, gt, bt = z.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    yt = torch.relu(F.batch_norm(zt, None, None, gt, bt, True, 0.1, EPS))
    out["bn_relu_bwd"] = ab(lambda: ck(L.c4_train_bn_relu_bwd_f32(p(dy), p(z), p(mean), p(var), p(gamma), p(beta), EPS, m, n, n, n, n, p(dzo), p(dgamma),
                                                                 p(dbeta), stream())),
                            lambda: torch.autograd.grad(yt, (zt, gt, bt), dy, retain_graph=True))
    return out


def whole_step():
    from c4a0_amd import training as T
    from c4a0_amd.nn import ConnectFourNet, ModelConfig
    from c4a0_amd.train_heads import forward_train

    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    cell = torch.randint(0, 3, (M, 6, 7), generator=g)
    batch = (torch.stack([cell == 1, cell == 2], 1).float().to(dev), torch.softmax(torch.randn(M, 7, generator=g), 1).to(dev),
             (torch.rand(M, generator=g) * 2 - 1).to(dev), (torch.rand(M, generator=g) * 2 - 1).to(dev))
    steps = {}
    for heads in ("hip", "torch"):
        model = ConnectFourNet(ModelConfig(1, 32, 4, 2)).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=4e-4)

        def step(model=model, opt=opt, heads=heads):
            opt.zero_grad(set_to_none=True)
            T.loss(forward_train(model, batch[0], heads), batch)[0].backward()
            opt.step()

        steps[heads] = step
    r = ab(steps["hip"], steps["torch"], launches=5)
    return {"batch": M, "model": [1, 32, 4, 2], "hip_ms": r["hip_us"] * 1e-3, "torch_ms": r["torch_us"] * 1e-3,
            "hip_range_ms": [v * 1e-3 for v in r["hip_range_us"]], "torch_range_ms": [v * 1e-3 for v in r["torch_range_us"]]}


def alternating(fns: dict, pairs=7, launches=20):
    """medians (us per call) of `pairs` rounds that time every callable of `fns` in turn, and their spreads"""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(pairs):
        for name, fn in fns.items():
            t[name].append(time_us(fn, launches))
    return {name: {"us": statistics.median(v), "range_us": [min(v), max(v)]} for name, v in t.items()}


def bf16_leg():
    """heads="bf16" at m = 2 000, F = 1 344: every kernel of c4_train_bf16.hip and each of the three c4_linear_bf16 products alone (beside
    the stock op that does the same job on the same tensors), one hidden block forward + backward and the whole optimiser step with
    heads="bf16", heads="torch" and torch.autocast(bfloat16) on the stock module."""
    from c4a0_amd import training as T
    from c4a0_amd.nn import ConnectFourNet, ModelConfig
    from c4a0_amd.train_heads import forward_train, hidden_block

    L, ck = _lib.lib(), _lib.check
    g = torch.Generator().manual_seed(0)
    m, n, k = M, FEAT, FEAT
    mp = 64 * ((m + 63) // 64)
    bf = torch.bfloat16
    x, dy32 = (torch.randn(m, FEAT, generator=g).to(dev) for _ in range(2))
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(dev)
    b, gamma, beta = torch.randn(n, generator=g).to(dev), (torch.rand(n, generator=g) + 0.5).to(dev), torch.randn(n, generator=g).to(dev)
    zeros = torch.zeros(n, device=dev)
    xb, wb, z, y, dz, dx, dyb = (torch.empty((m, n), dtype=bf, device=dev) for _ in range(7))
    wb = torch.empty((n, k), dtype=bf, device=dev)
    xb_t, dz_t, y_t = (torch.empty((n, mp), dtype=bf, device=dev) for _ in range(3))
    wb_t, dw = torch.empty((k, n), dtype=bf, device=dev), torch.empty((n, k), dtype=bf, device=dev)
    mean, var, db, dgamma, dbeta = (torch.empty(n, device=dev) for _ in range(5))
    dyb.copy_(dy32)

    def linear(xo, wo, bias, yo, mm, nn, kk):
        ck(L.c4_linear_bf16(p(xo), p(wo), p(bias), p(yo), mm, nn, kk, xo.stride(0), nn, 0, 0, stream()))

    cast_x = lambda: ck(L.c4_train_cast_bf16(p(x), 0, m, k, k, p(xb), k, p(xb_t), mp, stream()))
    cast_w = lambda: ck(L.c4_train_cast_bf16(p(w), 0, n, k, k, p(wb), k, None, 0, stream()))
    cast_wt = lambda: ck(L.c4_train_cast_bf16(p(wb), 1, n, k, k, None, 0, p(wb_t), n, stream()))
    fwd = lambda: linear(xb, wb, b, z, m, n, k)
    bn_fwd = lambda: ck(L.c4_train_bn_relu_fwd_bf16(p(z), p(gamma), p(beta), EPS, m, n, n, n, p(y), p(mean), p(var), p(y_t), mp, stream()))
    bn_bwd = lambda: ck(L.c4_train_bn_relu_bwd_bf16(p(dyb), p(z), p(mean), p(var), p(gamma), p(beta), EPS, m, n, n, n, n, p(dz), p(dz_t), mp, p(dgamma),
                                                    p(dbeta), p(db), stream()))
    for fn in (cast_x, cast_w, cast_wt, fwd, bn_fwd, bn_bwd):      # every operand of the timed calls is a real one
        fn()
    zt, gt, bt = z.float().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    yt = torch.relu(F.batch_norm(zt, None, None, gt, bt, True, 0.1, EPS))
    bb = b.to(bf)
    out = {"kernels": {
        "cast_x_and_transpose": alternating({"hip": cast_x, "torch": lambda: (x.to(bf), x.to(bf).t().contiguous())}),
        "cast_w": alternating({"hip": cast_w, "torch": lambda: w.to(bf)}),
        "transpose_w": alternating({"hip": cast_wt, "torch": lambda: wb.t().contiguous()}),
        "linear_fwd": alternating({"hip": fwd, "torch": lambda: F.linear(xb, wb, bb)}),
        "dgrad": alternating({"hip": lambda: linear(dz, wb_t, zeros, dx, m, k, n), "torch": lambda: dz @ wb}),
        "wgrad": alternating({"hip": lambda: linear(dz_t, xb_t, zeros, dw, n, k, mp), "torch": lambda: dz.t() @ xb}),
        "bn_relu_fwd": alternating({"hip": bn_fwd, "torch_f32": lambda: torch.relu(F.batch_norm(zt.detach(), None, None, gamma, beta, True, 0.1, EPS))}),
        "bn_relu_bwd": alternating({"hip": bn_bwd, "torch_f32": lambda: torch.autograd.grad(yt, (zt, gt, bt), dy32, retain_graph=True)}),
    }}
    flop = 2.0 * m * n * k
    for name in ("linear_fwd", "dgrad", "wgrad"):
        for side in out["kernels"][name].values():
            side["tflops"] = flop / side["us"] * 1e-6

    # one hidden block, forward + backward (dx included), and the whole optimiser step
    def block_fn(kind):
        torch.manual_seed(0)
        block = torch.nn.Sequential(torch.nn.Linear(FEAT, FEAT), torch.nn.BatchNorm1d(FEAT), torch.nn.ReLU()).to(dev).train()
        xin = x.clone().requires_grad_()

        def run():
            xin.grad = None
            block.zero_grad(set_to_none=True)
            if kind == "bf16":
                hidden_block(block, xin, "bf16").backward(dyb)
            elif kind == "torch":
                block(xin).backward(dy32)
            else:
                with torch.autocast("cuda", dtype=bf):
                    yy = block(xin)
                yy.backward(dy32.to(yy.dtype))

        return run

    out["hidden_block_fwd_bwd"] = alternating({kind: block_fn(kind) for kind in ("bf16", "torch", "autocast")}, launches=10)
    g = torch.Generator().manual_seed(1)
    cell = torch.randint(0, 3, (M, 6, 7), generator=g)
    batch = (torch.stack([cell == 1, cell == 2], 1).float().to(dev), torch.softmax(torch.randn(M, 7, generator=g), 1).to(dev),
             (torch.rand(M, generator=g) * 2 - 1).to(dev), (torch.rand(M, generator=g) * 2 - 1).to(dev))

    def step_fn(kind):
        torch.manual_seed(0)
        model = ConnectFourNet(ModelConfig(1, 32, 4, 2)).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=4e-4)

        def run():
            opt.zero_grad(set_to_none=True)
            if kind == "autocast":
                with torch.autocast("cuda", dtype=bf):
                    res = model(batch[0])
                res = tuple(t.float() for t in res)
            else:
                res = forward_train(model, batch[0], kind)
            T.loss(res, batch)[0].backward()
            opt.step()

        return run

    out["step"] = alternating({kind: step_fn(kind) for kind in ("bf16", "torch", "autocast")}, launches=5)
    out["step"].update(batch=M, model=[1, 32, 4, 2])
    return out


def graph_leg():
    """c4_train_adam_f32 beside torch.optim.Adam.step(), and the whole step of ModelConfig(1, 32, 4, 2) at batch 2 000 for every head
    path, eager with torch.optim.Adam, eager with HipAdam and as a graph replay."""
    from c4a0_amd import training as T
    from c4a0_amd.nn import ConnectFourNet, ModelConfig
    from c4a0_amd.train_graph import GraphedTrainStep, HipAdam
    from c4a0_amd.train_heads import forward_train

    g = torch.Generator().manual_seed(1)
    cell = torch.randint(0, 3, (M, 6, 7), generator=g)
    data = (torch.stack([cell == 1, cell == 2], 1).float().to(dev), torch.softmax(torch.randn(M, 7, generator=g), 1).to(dev),
            (torch.rand(M, generator=g) * 2 - 1).to(dev), (torch.rand(M, generator=g) * 2 - 1).to(dev))
    idx = torch.randperm(M, generator=g).to(dev)

    def fresh():
        torch.manual_seed(0)
        return ConnectFourNet(ModelConfig(1, 32, 4, 2)).to(dev).train()

    # the optimiser alone, on gradients that stay where one backward left them
    models = {"hip": fresh(), "torch": fresh()}
    opts = {"hip": HipAdam(models["hip"].parameters(), lr=2e-3, weight_decay=4e-4),
            "torch": torch.optim.Adam(models["torch"].parameters(), lr=2e-3, weight_decay=4e-4)}
    for model in models.values():
        T.loss(model(data[0]), data)[0].backward()
    n_params = sum(q.numel() for q in models["hip"].parameters())
    adam = alternating({name: opt.step for name, opt in opts.items()})
    adam.update(parameters=n_params, tensors=len(opts["hip"].params), bytes_per_parameter=28,
                hip_bytes_per_s=28.0 * n_params / (adam["hip"]["us"] * 1e-6))

    def step_fn(heads, kind):
        model = fresh()
        if kind == "graph":
            graphed = GraphedTrainStep(model, HipAdam(model.parameters(), lr=2e-3, weight_decay=4e-4), heads, M, data)
            return lambda: graphed.run(idx)
        opt = HipAdam(model.parameters(), lr=2e-3, weight_decay=4e-4) if kind == "eager_hip_adam" else \
            torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=4e-4)

        def run():
            b = tuple(t[idx] for t in data)
            if kind == "eager_hip_adam":
                opt.zero_grad()
            else:
                opt.zero_grad(set_to_none=True)
            T.loss(forward_train(model, b[0], heads), b)[0].backward()
            opt.step()

        return run

    fns = {f"{heads}/{kind}": step_fn(heads, kind) for heads in ("torch", "hip", "bf16") for kind in ("eager_torch_adam", "eager_hip_adam", "graph")}
    step = alternating(fns, launches=5)
    base = step["torch/eager_torch_adam"]["us"]
    for v in step.values():
        v["ms"] = v["us"] * 1e-3
        v["speedup_over_eager_torch"] = base / v["us"]
    return {"adam": adam, "step": dict(step, batch=M, model=[1, 32, 4, 2])}


def tower_leg():
    from c4a0_amd import train_tower as TT
    from c4a0_amd import training as T
    from c4a0_amd.nn import ConnectFourNet, ModelConfig
    from c4a0_amd.train_graph import GraphedTrainStep, HipAdam
    from c4a0_amd.train_heads import forward_train

    L, ck = _lib.lib(), _lib.check
    g = torch.Generator().manual_seed(0)
    b, c = M, 32
    m = 42 * b
    cell = torch.randint(0, 3, (b, 6, 7), generator=g)
    planes = torch.stack([cell == 1, cell == 2], 1).float().to(dev)
    w0_t, w_t = (torch.randn(c, 2, 3, 3, generator=g) / 18 ** 0.5).to(dev), (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).to(dev)
    bias, gamma, beta = torch.randn(c, generator=g).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    zero = torch.zeros(c, device=dev)
    x, dz, dy, a = (torch.randn(m, c, generator=g).to(dev) for _ in range(4))            # cell-major [42 B][C]
    nchw = lambda t: t.reshape(b, 6, 7, c).permute(0, 3, 1, 2).contiguous()
    x_n, dz_n, dy_n, a_n = nchw(x), nchw(dz), nchw(dy), nchw(a)
    w0, w, wd = TT.pack_conv0(w0_t), TT.pack_conv3x3(w_t), TT.pack_conv3x3_dgrad(w_t)
    z, y, dx = (torch.empty((m, c), device=dev) for _ in range(3))
    dw, dw0 = torch.empty((c, 9 * c), device=dev), torch.empty((c, 32), device=dev)
    mean, var, db, dgamma, dbeta = (torch.empty(c, device=dev) for _ in range(5))
    work = torch.empty(TT.work_bytes(b, c) // 4, device=dev)
    ck(L.c4_train_conv3x3_f32(p(x), p(w), p(bias), p(z), b, c, stream()))
    ck(L.c4_train_bn2d_relu_res_fwd_f32(p(z), p(a), p(gamma), p(beta), EPS, b, c, p(y), p(mean), p(var), p(work), stream()))
    z_n = nchw(z)
    zt, gt, bt = z_n.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    yt = a_n + torch.relu(F.batch_norm(zt, None, None, gt, bt, True, 0.1, EPS))
    grad = torch.nn.grad
    kernels = {
        "conv0_fwd": {"hip": lambda: ck(L.c4_train_conv0_f32(p(planes), p(w0), p(bias), p(z), b, c, stream())),
                      "torch": lambda: F.conv2d(planes, w0_t, bias, padding=1)},
        "conv3x3_fwd": {"hip": lambda: ck(L.c4_train_conv3x3_f32(p(x), p(w), p(bias), p(y), b, c, stream())),
                        "torch": lambda: F.conv2d(x_n, w_t, bias, padding=1)},
        "conv3x3_dgrad": {"hip": lambda: ck(L.c4_train_conv3x3_f32(p(dz), p(wd), p(zero), p(dx), b, c, stream())),
                          "torch": lambda: grad.conv2d_input(x_n.shape, w_t, dz_n, padding=1)},
        "conv3x3_wgrad": {"hip": lambda: ck(L.c4_train_conv3x3_wgrad_f32(p(dz), p(x), p(dw), p(db), b, c, p(work), stream())),
                          "torch": lambda: (grad.conv2d_weight(x_n, w_t.shape, dz_n, padding=1), dz_n.sum((0, 2, 3)))},
        "conv0_wgrad": {"hip": lambda: ck(L.c4_train_conv0_wgrad_f32(p(dz), p(planes), p(dw0), p(db), b, c, p(work), stream())),
                        "torch": lambda: (grad.conv2d_weight(planes, w0_t.shape, dz_n, padding=1), dz_n.sum((0, 2, 3)))},
        "bn2d_relu_res_fwd": {"hip": lambda: ck(L.c4_train_bn2d_relu_res_fwd_f32(p(z), p(a), p(gamma), p(beta), EPS, b, c, p(y), p(mean), p(var), p(work),
                                                                                 stream())),
                              "torch": lambda: a_n + torch.relu(F.batch_norm(z_n, None, None, gamma, beta, True, 0.1, EPS))},
        "bn2d_relu_res_bwd": {"hip": lambda: ck(L.c4_train_bn2d_relu_res_bwd_f32(p(dy), p(z), p(mean), p(var), p(gamma), p(beta), EPS, b, c, p(dx),
                                                                                 p(dgamma), p(dbeta), p(work), stream())),
                              "torch": lambda: torch.autograd.grad(yt, (zt, gt, bt), dy_n, retain_graph=True)},
    }
    out = {"shape": {"batch": b, "channels": c, "rows": m, "chunk_boards": _lib.TOWER_CHUNK_BOARDS}, "kernels": {k: alternating(v) for k, v in kernels.items()}}
    flops = {"conv0_fwd": 2.0 * m * c * 18, "conv0_wgrad": 2.0 * m * c * 18, "conv3x3_fwd": 2.0 * m * c * 9 * c, "conv3x3_dgrad": 2.0 * m * c * 9 * c,
             "conv3x3_wgrad": 2.0 * m * c * 9 * c}
    for name, flop in flops.items():
        for side in out["kernels"][name].values():
            side["tflops"] = flop / side["us"] * 1e-6

    def fresh():
        torch.manual_seed(0)
        return ConnectFourNet(ModelConfig(1, 32, 4, 2)).to(dev).train()

    # the tower alone, forward + backward from a given gradient of its features
    dfeat = torch.randn(b, 42 * c, generator=g).to(dev)

    def tower_fn(kind):
        model = fresh()

        def run():
            model.conv.zero_grad(set_to_none=True)
            feat = TT.tower_forward(model.conv, planes) if kind == "hip" else model.conv(planes).reshape(b, -1)
            feat.backward(dfeat)

        return run

    out["tower_fwd_bwd"] = alternating({kind: tower_fn(kind) for kind in ("hip", "torch")}, launches=10)
    data = (planes, torch.softmax(torch.randn(b, 7, generator=g), 1).to(dev), (torch.rand(b, generator=g) * 2 - 1).to(dev),
            (torch.rand(b, generator=g) * 2 - 1).to(dev))
    idx = torch.randperm(b, generator=g).to(dev)

    def step_fn(heads, tower, kind):
        model = fresh()
        if kind == "graph":
            graphed = GraphedTrainStep(model, HipAdam(model.parameters(), lr=2e-3, weight_decay=4e-4), heads, b, data, tower_path=tower)
            return lambda: graphed.run(idx)
        opt = HipAdam(model.parameters(), lr=2e-3, weight_decay=4e-4) if kind == "eager_hip_adam" else \
            torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=4e-4)

        def run():
            bt_ = tuple(t[idx] for t in data)
            if kind == "eager_hip_adam":
                opt.zero_grad()
            else:
                opt.zero_grad(set_to_none=True)
            T.loss(forward_train(model, bt_[0], heads, tower), bt_)[0].backward()
            opt.step()

        return run

    fns = {"heads=torch/tower=torch/eager_torch_adam": step_fn("torch", "torch", "eager_torch_adam")}
    for heads in ("torch", "bf16"):
        for tower in ("torch", "hip"):
            for kind in ("eager_hip_adam", "graph"):
                fns[f"heads={heads}/tower={tower}/{kind}"] = step_fn(heads, tower, kind)
    step = alternating(fns, launches=5)
    for v in step.values():
        v["ms"] = v["us"] * 1e-3
    out["step"] = dict(step, batch=b, model=[1, 32, 4, 2])
    return out


def outputs_leg():
    """The opt-in outputs="hip" path.  (a) At m = 2 000, k = 1 344, from f32 and from bf16 activations: c4_train_out_loss_fwd and
    c4_train_out_loss_bwd alone, the autograd Function over them forward + backward, and the stock ops they replace on the same values
    as one group (F.linear x 2, log_softmax, tanh, loss; then with their autograd).  (b) The whole step of ModelConfig(1, 32, 4, 2) at
    batch 2 000 for heads in {torch, bf16} x outputs in {torch, hip}, eager with HipAdam and as a graph replay, all timed in turn."""
    from c4a0_amd import train_out as TO
    from c4a0_amd import training as T
    from c4a0_amd.nn import ConnectFourNet, ModelConfig
    from c4a0_amd.train_graph import GraphedTrainStep, HipAdam, train_step

    L, ck = _lib.lib(), _lib.check
    g = torch.Generator().manual_seed(0)
    m, k = M, FEAT
    wp, wv = ((torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5 for n in (7, 2))
    bp, bv = ((torch.rand(n, generator=g) * 2 - 1) / k ** 0.5 for n in (7, 2))
    wp, bp, wv, bv = (t.to(dev) for t in (wp, bp, wv, bv))
    tgt = (torch.softmax(torch.randn(m, 7, generator=g), 1).to(dev), (torch.rand(m, generator=g) * 2 - 1).to(dev),
           (torch.rand(m, generator=g) * 2 - 1).to(dev))
    out, dz = torch.empty((m, 9), device=dev), torch.empty((m, 9), device=dev)
    losses, one = torch.empty(4, device=dev), torch.ones(4, device=dev)
    dwp, dbp, dwv, dbv = torch.empty_like(wp), torch.empty_like(bp), torch.empty_like(wv), torch.empty_like(bv)
    work = torch.empty(TO.work_bytes(m, k) // 4, device=dev)
    res = {"shape": {"m": m, "k": k, "chunk_rows": _lib.OUT_CHUNK_ROWS, "work_bytes": TO.work_bytes(m, k)}, "calls": {}}
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        # relu of a normal variable: what a hidden block hands over
        xp, xv = (torch.relu(torch.randn(m, k, generator=g)).to(dev).to(dtype) for _ in range(2))
        dxp, dxv = torch.empty_like(xp), torch.empty_like(xv)
        is_bf16 = int(dtype == torch.bfloat16)
        leaves = [t.clone().requires_grad_() for t in (xp, xv, wp, bp, wv, bv)]

        def hip_fwd():
            ck(L.c4_train_out_loss_fwd(p(xp), p(xv), is_bf16, k, k, p(wp), p(bp), p(wv), p(bv), p(tgt[0]), p(tgt[1]), p(tgt[2]), m, k, p(out), p(dz),
                                       p(losses), p(work), stream()))

        def hip_bwd():
            ck(L.c4_train_out_loss_bwd(p(dz), p(one), p(xp), p(xv), is_bf16, k, k, p(wp), p(wv), m, k, p(dxp), p(dxv), k, k, p(dwp), p(dbp), p(dwv),
                                       p(dbv), p(work), stream()))

        def stock_losses():
            # the bf16 path's f32 output layer reads x.float(); autograd rounds its dx back to bf16
            logp = F.log_softmax(F.linear(leaves[0].float(), leaves[2], leaves[3]), dim=1)
            q = torch.tanh(F.linear(leaves[1].float(), leaves[4], leaves[5]))
            return T.loss((logp, q[:, 0], q[:, 1]), (None,) + tgt)

        def torch_fwd():
            stock_losses()

        def torch_fwd_bwd():
            torch.autograd.grad(stock_losses()[0], leaves)

        def hip_function_fwd_bwd():
            torch.autograd.grad(TO.OutLossFunction.apply(*leaves, *tgt)[0], leaves)

        hip_fwd()
        res["calls"][name] = alternating({"hip_fwd": hip_fwd, "hip_bwd": hip_bwd, "hip_function_fwd_bwd": hip_function_fwd_bwd,
                                          "torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd})
        c = res["calls"][name]
        c["hip_fwd_plus_bwd_us"] = c["hip_fwd"]["us"] + c["hip_bwd"]["us"]
        c["x_bytes_read_per_call"] = 2 * m * k * xp.element_size()
        c["hip_fwd_bytes_per_s"] = c["x_bytes_read_per_call"] / (c["hip_fwd"]["us"] * 1e-6)
        c["hip_bwd_bytes_per_s"] = 2 * c["x_bytes_read_per_call"] / (c["hip_bwd"]["us"] * 1e-6)      # reads x, writes dx

    cell = torch.randint(0, 3, (M, 6, 7), generator=g)
    data = (torch.stack([cell == 1, cell == 2], 1).float().to(dev), torch.softmax(torch.randn(M, 7, generator=g), 1).to(dev),
            (torch.rand(M, generator=g) * 2 - 1).to(dev), (torch.rand(M, generator=g) * 2 - 1).to(dev))
    idx = torch.randperm(M, generator=g).to(dev)

    def step_fn(heads, outputs, kind):
        torch.manual_seed(0)
        model = ConnectFourNet(ModelConfig(1, 32, 4, 2)).to(dev).train()
        opt = HipAdam(model.parameters(), lr=2e-3, weight_decay=4e-4)
        if kind == "graph":
            graphed = GraphedTrainStep(model, opt, heads, M, data, outputs_path=outputs)
            return lambda: graphed.run(idx)
        return lambda: train_step(model, opt, tuple(t[idx] for t in data), heads, "torch", outputs)

    fns = {f"heads={heads}/outputs={outputs}/{kind}": step_fn(heads, outputs, kind)
           for kind in ("graph", "eager_hip_adam") for heads in ("torch", "bf16") for outputs in ("torch", "hip")}
    step = alternating(fns, launches=5)
    for v in step.values():
        v["ms"] = v["us"] * 1e-3
    res["step"] = dict(step, batch=M, model=[1, 32, 4, 2])
    return res


def generation(max_epochs: int, heads: str, graph: bool = False):
    from c4a0_amd import training as T
    from c4a0_amd.nn import ModelConfig

    with tempfile.TemporaryDirectory() as base:
        torch.manual_seed(0)
        parent = T.TrainingGen.load_latest_with_default(base, 1400, 6.6, 0.01, 2000, 2000, ModelConfig(1, 32, 4, 2), T.TrainConfig({0: 2e-3}, 4e-4))
        timings = {}
        gen = T.train_single_gen(base, dev, parent, 1700, 1400, 6.6, 0.01, 2000, 2000, heads=heads, max_epochs=max_epochs, timings=timings,
                                 graph=graph)
        timings.update(heads=heads, graph=graph, max_epochs=max_epochs, val_loss=gen.val_loss, games=1700, n_mcts_iterations=1400, batch=2000)
        return timings


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "train_rate.json"))
    ap.add_argument("--no-generation", action="store_true")
    ap.add_argument("--max-epochs", type=int, default=10)
    ap.add_argument("--bf16", action="store_true", help='the heads="bf16" leg alone -> profiles/train_rate_bf16.json')
    ap.add_argument("--graph", action="store_true", help="the graphed-step leg alone -> profiles/train_rate_graph.json")
    ap.add_argument("--tower", action="store_true", help='the tower="hip" leg alone -> profiles/train_rate_tower.json')
    ap.add_argument("--outputs", action="store_true", help='the outputs="hip" leg alone -> profiles/train_rate_outputs.json')
    a = ap.parse_args()
    out_path, max_epochs = a.out, a.max_epochs
    if a.outputs:
        if out_path == ap.get_default("out"):
            out_path = os.path.join(ROOT, "profiles", "train_rate_outputs.json")
        res = {"device": torch.cuda.get_device_name(0)}
        res.update(outputs_leg())
        print(json.dumps(res, indent=1), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if a.tower:
        if out_path == ap.get_default("out"):
            out_path = os.path.join(ROOT, "profiles", "train_rate_tower.json")
        res = {"device": torch.cuda.get_device_name(0)}
        res.update(tower_leg())
        print(json.dumps(res, indent=1), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if a.graph:
        if out_path == ap.get_default("out"):
            out_path = os.path.join(ROOT, "profiles", "train_rate_graph.json")
        res = {"device": torch.cuda.get_device_name(0)}
        res.update(graph_leg())
        print(json.dumps(res, indent=1), flush=True)
        if not a.no_generation:
            generation(1, "torch")   # not recorded: the process's first generation pays the libraries' one-time initialisation
            res["generation"] = []
            for heads in ("torch", "hip", "bf16"):
                for graph in (False, True):
                    res["generation"].append(generation(max_epochs, heads, graph))
                    print(json.dumps(res["generation"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if a.bf16:
        if out_path == ap.get_default("out"):
            out_path = os.path.join(ROOT, "profiles", "train_rate_bf16.json")
        res = {"device": torch.cuda.get_device_name(0), "shape": {"m": M, "n": FEAT, "k": FEAT}}
        res.update(bf16_leg())
        print(json.dumps(res, indent=1), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    res = {"device": torch.cuda.get_device_name(0), "shape": {"m": M, "n": FEAT, "k": FEAT}, "kernels": kernels(), "step": whole_step()}
    print(json.dumps(res, indent=1), flush=True)
    if not a.no_generation:
        faster = "hip" if res["step"]["hip_ms"] < res["step"]["torch_ms"] else "torch"
        res["generation"] = generation(max_epochs, faster)
        print(json.dumps(res["generation"], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
