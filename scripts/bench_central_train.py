"""central_train for a linear model: ``chain_train``, one launch and batch-split, against the torch loop of fedavg_trainer.py:361-371.

    python scripts/bench_central_train.py                   # every configuration, one child process each
    python scripts/bench_central_train.py --one 64 sgd 1000 # one configuration, one JSON line

Workload: MNIST-LR shapes (D = 784, C = 10), K in 100, 1000 clients of B = 64 and B = 600 samples, SGD and Adam,
3 central rounds: 3 K optimizer steps of one model.  The three arms (the torch loop, ``chain_train``, and
``chain_train(split=True)``) run in the same process on batches that are resident on the GPU, rotated (loop, chain,
split, loop, ...), 3 warm-up rounds of arms and then 30 timed ones.  The loop arm is the
reference's: per step ``zero_grad``, forward, ``CrossEntropyLoss``, backward, ``loss.item()`` and ``optimizer.step()``,
with a fresh optimizer per run as central_train makes one.  A time is host wall clock around the arm including its
host syncs; the line holds the three medians, the extremes and whether one arm was below another in EVERY round of
arms (``all_below``: chain below loop; ``split_below_loop_every_pair``; ``split_below_chain_every_pair``; without the
flag nothing is called faster).  ``x_gbps`` is the bytes of x the chain reads (every batch once
per round) over the chain's median time: a rate over the whole call, host time included, not a counter reading.

The driver runs each configuration as a child process under its own time limit and stops at the first that fails;
lines go to profiles/central_train/mi355x_central_split.jsonl (mi355x_central_train.jsonl beside it is the two-arm
run from before the split arm existed).
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]
OUT = ROOT / "profiles" / "central_train" / "mi355x_central_split.jsonl"
D, C, ROUNDS, WARMUP, REPEATS = 784, 10, 3, 3, 30
KS, BS, OPTIMIZERS = (100, 1000), (64, 600), ("sgd", "adam")
HYPER = {"sgd": dict(lr=0.05, wd=0.0), "adam": dict(lr=0.001, wd=0.001)}
LIMIT_S = 400  # per child


def one(B, optimizer, K):
    import torch

    import mfl_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(B + K)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(D, C)).to(dev)
    w0, b0 = net[1].weight.detach().clone(), net[1].bias.detach().clone()
    batches = [((0.25 * torch.randn(B, D, generator=g)).to(dev), torch.randint(0, C, (B,), generator=g).to(dev))
               for _ in range(K)]
    h, criterion = HYPER[optimizer], torch.nn.CrossEntropyLoss().to(dev)

    def restore():
        with torch.no_grad():
            net[1].weight.copy_(w0)
            net[1].bias.copy_(b0)

    def loop():
        opt = torch.optim.SGD(net.parameters(), lr=h["lr"]) if optimizer == "sgd" else \
            torch.optim.Adam(net.parameters(), lr=h["lr"], weight_decay=h["wd"], amsgrad=True)
        for _ in range(ROUNDS):
            for x, labels in batches:
                net.train()
                net.zero_grad()
                loss = criterion(net(x), labels)
                loss.backward()
                loss = loss.item()
                opt.step()
        return loss

    def chain():
        return mfl_amd.chain_train(net, batches, ROUNDS, optimizer=optimizer, **h)[-1]

    def split():
        return mfl_amd.chain_train(net, batches, ROUNDS, optimizer=optimizer, split=True, **h)[-1]

    def timed(fn):
        restore()
        torch.cuda.synchronize()
        t = time.perf_counter()
        loss = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, loss

    runs = [(timed(loop), timed(chain), timed(split)) for _ in range(WARMUP + REPEATS)][WARMUP:]
    lo, ch, sp = ([r[arm][0] for r in runs] for arm in range(3))
    line = dict(workload="mnist_lr_central_train", B=B, D=D, C=C, rounds=ROUNDS, optimizer=optimizer, K=K,
                repeats=REPEATS, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                loop_ms=statistics.median(lo), chain_ms=statistics.median(ch), split_ms=statistics.median(sp),
                loop_min_max=[min(lo), max(lo)], chain_min_max=[min(ch), max(ch)], split_min_max=[min(sp), max(sp)],
                all_below=all(c < s for s, c in zip(lo, ch)),
                split_below_loop_every_pair=all(p < s for s, p in zip(lo, sp)),
                split_below_chain_every_pair=all(p < c for c, p in zip(ch, sp)),
                x_gbps=ROUNDS * K * B * D * 4 / (statistics.median(ch) * 1e-3) / 1e9,
                last_loss=dict(loop=runs[-1][0][1], chain=runs[-1][1][1], split=runs[-1][2][1]))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--one", nargs=3, metavar=("B", "OPTIMIZER", "K"))
    ap.add_argument("--out", type=Path, default=OUT)
    a = ap.parse_args()
    if a.one:
        return one(int(a.one[0]), a.one[1], int(a.one[2]))
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with a.out.open("w") as f:
        for K in KS:
            for B in BS:
                for optimizer in OPTIMIZERS:
                    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--one", str(B), optimizer, str(K)]
                    proc = subprocess.run(cmd, capture_output=True, text=True)
                    if proc.returncode != 0:  # nothing more is started on the GPU after a failure
                        sys.exit(f"{' '.join(cmd[4:])} ended with {proc.returncode}:\n{proc.stdout}\n{proc.stderr[-2000:]}")
                    f.write(proc.stdout.strip().splitlines()[-1] + "\n")
                    f.flush()
                    print(proc.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
