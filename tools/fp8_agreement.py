"""What the fp8 hidden layers change in the evaluator's answers -> profiles/fp8_agreement.json.

    python tools/fp8_agreement.py [out.json]

The fp8-head InferenceNet against the bf16 one on 4 096 random positions (tests.helpers.random_positions), for the default-initialised
4 x 32 and 8 x 64 networks and tests.helpers.sharp_model: top-1 move agreement over the legal moves, mean and max |delta log p| over
the legal moves, mean and max |delta q|, and per fp8 tensor the share of activations that saturated (|code| = 448).  No trained network
is available: what FP8 costs in playing strength is NOT measured by this."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig  # noqa: E402
from tests.helpers import SHARP_MODEL_K, pos_to_planes_np, random_positions, sharp_model  # noqa: E402

dev = torch.device("cuda:0")


def compare(name, model, planes, legal):
    bf = InferenceNet(model, dev)
    f8 = InferenceNet(model, dev, head_dtype=torch.float8_e4m3fn)
    sat = {}
    ch = f8.chain
    run_layer, quantize = ch.run_layer, ch.quantize

    def seen(tag, y):
        if y.dtype == torch.uint8:
            sat[tag] = float(((y & 0x7F) == 0x7E).float().mean())
        return y

    ch.run_layer = lambda ly, x8, *a, **k: seen(ly["name"] + " output", run_layer(ly, x8, *a, **k))
    ch.quantize = lambda x, e: seen("tower output (first layer's input)", quantize(x, e))
    lp8, q8 = f8.forward(planes)
    del ch.run_layer, ch.quantize
    lpb, qb = bf.forward(planes)
    torch.cuda.synchronize()
    neg = torch.full_like(lpb, -float("inf"))
    top_b, top_8 = torch.where(legal, lpb, neg).argmax(1), torch.where(legal, lp8, neg).argmax(1)
    dlp = (lp8 - lpb).abs()[legal]
    dq = (q8 - qb).abs()
    return {"network": name, "positions": int(planes.shape[0]), "top1_agreement": float((top_b == top_8).float().mean()),
            "abs_delta_logp_mean": float(dlp.mean()), "abs_delta_logp_max": float(dlp.max()), "abs_delta_q_mean": float(dq.mean()),
            "abs_delta_q_max": float(dq.max()), "fp8_scales": f8.fp8_scales, "saturated_share": sat}


if __name__ == "__main__":
    pos = np.array(random_positions(4096), dtype=np.uint64)
    planes = torch.from_numpy(pos_to_planes_np(pos[:, 0], pos[:, 1])).to(dev, torch.bfloat16)
    legal = torch.from_numpy(np.stack([((pos[:, 0] >> np.uint64(35 + c)) & np.uint64(1)) == 0 for c in range(7)], axis=1)).to(dev)
    out = []
    for blocks, channels in ((4, 32), (8, 64)):
        torch.manual_seed(1337)
        out.append(compare(f"default-initialised {blocks} x {channels}", ConnectFourNet(ModelConfig(blocks, channels, 4, 2)).eval(), planes, legal))
        print(out[-1], flush=True)
    out.append(compare(f"tests.helpers.sharp_model(4, 32, {SHARP_MODEL_K})", sharp_model(4, 32, SHARP_MODEL_K), planes, legal))
    print(out[-1], flush=True)
    res = {"note": "randomly initialised / constructed networks only: playing strength under FP8 is unmeasured", "results": out}
    json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "profiles/fp8_agreement.json", "w"), indent=1)
