"""Time a whole local loop of Client.train on the GPU (the prologue's forward
and backward, then --iters iterations of forward, backward and bookkeeping,
then the last read), with real models, under three kinds of bookkeeping:

  torch   : step="torch"  -- optimizer.step(), the fused statistics passes, one
            host sync per iteration (the :71 guard);
  fused   : step="fused"  -- the fused SGD / Adam step, still one sync per
            iteration;
  device  : step="fused", guard="device" at ahead in --ahead -- the guard
            decided on the device, the step gated on it, one sync per loop.

    python scripts/bench_client_loop.py [--models ...] [--dtypes f32,bf16] [--reps 30] [--out-dir profiles/client_loop]

The time is the host's wall clock around client_stats.client_train() between
two device synchronisations: the loop is launch- and latency-bound, so the
host's time is the quantity of interest.  Every repetition starts from the
same weights.  The arms alternate within every repetition (arm A, B, C, ...,
then again), so drift of the machine falls on all of them alike; the figure
is the median over --reps repetitions.  No threshold: "vs_fused" is an arm's
median over the fused arm's of the same run, whatever it comes to.

The models are the public architectures the reference trains, written here
for the benchmark: logistic regression on 784 inputs, the LEAF FEMNIST CNN,
CIFAR ResNet-56 (BatchNorm) and ResNet-18 with GroupNorm, at batch 32.
"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
import types
from pathlib import Path

import torch
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import mfl_amd  # noqa: E402
from mfl_amd import client_stats  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
BATCH = 32


class Flatten784(nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = nn.Linear(784, 10)

    def forward(self, x):
        return self.linear(x.flatten(1))


class FemnistCNN(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(1, 32, 5, padding=2), nn.Conv2d(32, 64, 5, padding=2)
        self.fc1, self.fc2 = nn.Linear(64 * 7 * 7, 2048), nn.Linear(2048, 62)

    def forward(self, x):
        x = torch.max_pool2d(torch.relu(self.conv1(x)), 2)
        x = torch.max_pool2d(torch.relu(self.conv2(x)), 2)
        return self.fc2(torch.relu(self.fc1(x.flatten(1))))


class Block(nn.Module):
    def __init__(self, cin, cout, stride, norm):
        super().__init__()
        self.c1, self.n1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False), norm(cout)
        self.c2, self.n2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False), norm(cout)
        self.short = None
        if stride != 1 or cin != cout:
            self.short = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), norm(cout))

    def forward(self, x):
        y = self.n2(self.c2(torch.relu(self.n1(self.c1(x)))))
        return torch.relu(y + (x if self.short is None else self.short(x)))


class ResNet(nn.Module):
    def __init__(self, widths, blocks, norm, classes=10):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, widths[0], 3, 1, 1, bias=False), norm(widths[0]), nn.ReLU())
        layers, cin = [], widths[0]
        for i, (w, n) in enumerate(zip(widths, blocks)):
            for j in range(n):
                layers.append(Block(cin, w, 2 if (i and j == 0) else 1, norm))
                cin = w
        self.layers = nn.Sequential(*layers)
        self.fc = nn.Linear(cin, classes)

    def forward(self, x):
        return self.fc(self.layers(self.stem(x)).mean((2, 3)))


MODELS = {
    "mnist_lr": (Flatten784, (1, 28, 28), 10),
    "femnist_cnn": (FemnistCNN, (1, 28, 28), 62),
    "resnet56": (lambda: ResNet((16, 32, 64), (9, 9, 9), nn.BatchNorm2d), (3, 32, 32), 10),
    "resnet18_gn": (lambda: ResNet((64, 128, 256, 512), (2, 2, 2, 2), lambda c: nn.GroupNorm(2, c)), (3, 32, 32), 10),
}


def make_client(x, labels, dev, optimizer):
    """A stand-in for the reference's Client and its module: what client_train reads."""
    name = "_bench_client_loop_module"
    mod = sys.modules.get(name)
    if mod is None:
        mod = types.ModuleType(name)
        mod.count = mod.count_end = time.perf_counter_ns
        mod.THRESHOLD_GRADS_RATIO = 1e12  # the guard never trips: every arm runs every iteration

        class Client:
            pass

        Client.__module__ = name
        mod.Client = Client
        sys.modules[name] = mod
    c = mod.Client()
    c.local_training_data = [(x, labels)]
    c.device = dev
    c.criterion = nn.CrossEntropyLoss().to(dev)
    c.args = types.SimpleNamespace(client_optimizer=optimizer, lr=0.01 if optimizer == "sgd" else 0.001, wd=0.001,
                                   clip=10.0)
    return c


def one_loop(client, net, start, iters, arm):
    """Wall-clock microseconds of one local loop from the weights ``start``."""
    net.load_state_dict(start)
    kw = dict(step="torch") if arm == "torch" else dict(step="fused")
    if arm.startswith("device"):
        kw["guard"] = "device"
        client_stats.DEFAULT_AHEAD = int(arm.split("_")[1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = client_stats.client_train(client, net, iters, keep_on_device=True, stats="hip", **kw)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    assert out[1] is not None, "the guard tripped: the arms would not do the same work"
    return (t1 - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--optimizers", default="sgd,adam")
    ap.add_argument("--ahead", default="1,2,4,8")
    ap.add_argument("--out-dir", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    default_ahead = client_stats.DEFAULT_AHEAD
    arms = ["torch", "fused"] + [f"device_{a}" for a in args.ahead.split(",")]
    lines = []
    for name in args.models.split(","):
        make, shape, classes = MODELS[name]
        for key in args.dtypes.split(","):
            dt = DTYPES[key]
            torch.manual_seed(0)
            net = make().to(dev).to(dt)
            x = torch.randn(BATCH, *shape, device=dev).to(dt)
            labels = torch.randint(0, classes, (BATCH,), device=dev)
            start = copy.deepcopy(net.state_dict())
            P = sum(p.numel() for p in net.parameters())
            for optimizer in args.optimizers.split(","):
                client = make_client(x, labels, dev, optimizer)
                times = {arm: [] for arm in arms}
                for rep in range(args.warmup + args.reps):
                    for arm in arms:
                        t = one_loop(client, net, start, args.iters, arm)
                        if rep >= args.warmup:
                            times[arm].append(t)
                med = {arm: statistics.median(ts) for arm, ts in times.items()}
                line = {"model": name, "dtype": key, "optimizer": optimizer, "P": P,
                        "keys": len(list(net.parameters())), "batch": BATCH, "iters": args.iters, "reps": args.reps,
                        "us_median": {arm: round(m, 1) for arm, m in med.items()},
                        "us_min": {arm: round(min(ts), 1) for arm, ts in times.items()},
                        "vs_fused": {arm: round(m / med["fused"], 3) for arm, m in med.items()},
                        "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
                print(json.dumps(line), flush=True)
                lines.append(line)
            del net
            torch.cuda.empty_cache()
    client_stats.DEFAULT_AHEAD = default_ahead
    if args.out_dir:
        out = Path(args.out_dir) / "mi355x_client_loop.jsonl"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
