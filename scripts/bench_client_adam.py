"""One local iteration's "step + weight bookkeeping" with Adam: step="torch"
(torch.optim.Adam's multi-tensor step, then ClientStepStats.after_step's
fused weight pass) against step="fused" (ClientStepStats.adam_step: one
kernel), scripts/bench_client_step.py's method.

    python scripts/bench_client_adam.py [--dtypes f32,bf16] [--out profiles/client_adam/bench.json]

Per shape and dtype: medians of 30 timed iterations after 5 warm-ups, torch
and fused three times each, alternating, in one process; times are host wall
clock around a synchronised iteration, in microseconds.  The gradients are
fixed tensors (no forward / backward): only the step and the bookkeeping run.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mfl_amd import client_stats  # noqa: E402

ADAM = dict(lr=0.001, weight_decay=0.001, amsgrad=True)


def _resnet_like(n_layers, width):
    shapes = [(16, 3, 3, 3), (16,), (16,)]
    for _ in range(n_layers):
        shapes += [(width, width, 3, 3), (width,), (width,)]
    return shapes + [(10, width), (10,)]


SHAPES = {
    "mnist_lr": [(10, 784), (10,)],
    "femnist_cnn": [(32, 1, 5, 5), (32,), (64, 32, 5, 5), (64,), (2048, 3136), (2048,), (62, 2048), (62,)],
    "resnet56": _resnet_like(55, 32),
    "resnet18_gn": _resnet_like(17, 256),
    "one_25m": [(25_000_000,)],
}


def _params(shapes, dt, dev):
    g = torch.Generator(device="cpu").manual_seed(7)
    params = []
    for s in shapes:
        p = torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(dt).to(dev))
        p.grad = torch.randn(s, generator=g).to(dt).to(dev)
        params.append(p)
    return params


def _median_us(shapes, dt, dev, mode, iters=30, warm=5):
    params = _params(shapes, dt, dev)
    stats = client_stats.ClientStepStats(params, stats="hip", step=mode, optimizer="adam", adam=ADAM)
    opt = None if mode == "fused" else torch.optim.Adam(params, lr=ADAM["lr"], weight_decay=ADAM["weight_decay"],
                                                        amsgrad=True)
    stats.begin(1.0)
    times = []
    for i in range(warm + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if opt is None:
            stats.adam_step(0.5, 1.0)
        else:
            opt.step()
            stats.after_step(0.5, 1.0)
        torch.cuda.synchronize()
        if i >= warm:
            times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "client_adam" / "bench.json"))
    ap.add_argument("--dtypes", default="f32,bf16")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    names = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
    rows = []
    for key in args.dtypes.split(","):
        dt = names[key]
        if client_stats.adam_form(dev, dt) is None:
            rows.append({"dtype": key, "skipped": "adam_form has no mask for this dtype: step='fused' is refused"})
            print(rows[-1], flush=True)
            continue
        for name, shapes in SHAPES.items():
            runs = {"torch": [], "fused": []}
            for _ in range(3):
                for mode in ("torch", "fused"):
                    runs[mode].append(_median_us(shapes, dt, dev, mode))
            n = sum(int(torch.Size(s).numel()) for s in shapes)
            row = {"dtype": key, "shape": name, "params": n, "keys": len(shapes),
                   "torch_us": [round(v, 1) for v in runs["torch"]], "fused_us": [round(v, 1) for v in runs["fused"]]}
            row["torch_spread_us"] = round(max(runs["torch"]) - min(runs["torch"]), 1)
            row["speedup"] = round(statistics.median(runs["torch"]) / statistics.median(runs["fused"]), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"torch": torch.__version__, "device": torch.cuda.get_device_name(0),
                                          "adam": ADAM, "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
