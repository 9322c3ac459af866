"""A round's wide linear clients: one ``cohort_train(wide=True)`` call against K sequential torch loops.

    python scripts/bench_cohort_wide.py                       # every configuration, one child process each
    python scripts/bench_cohort_wide.py --one 784 62 64 10    # one configuration (D C B K), one JSON line

Workload: FEMNIST-LR (D = 784, C = 62) and fed_cifar100-LR (D = 3072, C = 100) shapes, B = 64 and B = 600 samples per
client, 10 local iterations, SGD, K = 10 and K = 100 clients that all start from the same global model, batches
resident on the GPU.  Both arms run in the same process, alternated (loop, wide, loop, ...), 3 warm-up pairs and then
30 timed pairs; a time is host wall clock around the arm including its host syncs, and the line holds the medians, the
extremes and whether wide was below the loop in EVERY pair (``all_below``; without it nothing is called faster).  The
loop arm is what such a round runs without the wide cohort: ``client_train(loop="torch")`` per client, the model
restored from the global parameters before each (two device copies).

The driver runs each configuration as a child process under its own time limit and stops at the first that fails;
lines go to profiles/client_cohort/mi355x_cohort_wide.jsonl.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
OUT = ROOT / "profiles" / "client_cohort" / "mi355x_cohort_wide.jsonl"
ITERS, WARMUP, REPEATS = 10, 3, 30
SHAPES, BS, KS = ((784, 62), (3072, 100)), (64, 600), (10, 100)
HYPER = dict(lr=0.05, wd=0.0)
LIMIT_S = 300  # per child


def one(D, C, B, K):
    import torch

    import mfl_amd
    from linear_loop_ref import make_client
    from mfl_amd.client_passes import wide_default_slices

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(B + K + D)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(D, C)).to(dev)
    w0, b0 = net[1].weight.detach().clone(), net[1].bias.detach().clone()
    scale = 0.25 * min(1.0, (784 / D) ** 0.5)
    clients = [make_client((scale * torch.randn(B, D, generator=g)).to(dev), torch.randint(0, C, (B,), generator=g).to(dev),
                           dev, "sgd", ratio=1e4, **HYPER) for _ in range(K)]
    P = C * D + C
    rows = torch.zeros(K, -(-P // mfl_amd.ALIGN_ELEMS) * mfl_amd.ALIGN_ELEMS, device=dev)

    def restore():
        with torch.no_grad():
            net[1].weight.copy_(w0)
            net[1].bias.copy_(b0)

    def loop():
        for c in clients:
            restore()
            mfl_amd.client_train(c, net, ITERS, loop="torch", keep_on_device=True)

    def wide():
        restore()
        mfl_amd.cohort_train(clients, net, ITERS, rows=rows, wide=True)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    pairs = [(timed(loop), timed(wide)) for _ in range(WARMUP + REPEATS)][WARMUP:]
    seq, wid = [p[0] for p in pairs], [p[1] for p in pairs]
    print(json.dumps(dict(
        workload="linear_wide", D=D, C=C, B=B, K=K, iters=ITERS, optimizer="sgd", repeats=REPEATS,
        slices_per_group=wide_default_slices([B] * K, C), device=torch.cuda.get_device_name(0), torch=torch.__version__,
        loop_ms=statistics.median(seq), wide_ms=statistics.median(wid), loop_min_max=[min(seq), max(seq)],
        wide_min_max=[min(wid), max(wid)], all_below=all(w < s for s, w in pairs))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--one", nargs=4, type=int, metavar=("D", "C", "B", "K"))
    ap.add_argument("--out", type=Path, default=OUT)
    a = ap.parse_args()
    if a.one:
        return one(*a.one)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with a.out.open("w") as f:
        for D, C in SHAPES:
            for B in BS:
                for K in KS:
                    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--one", *map(str, (D, C, B, K))]
                    proc = subprocess.run(cmd, capture_output=True, text=True)
                    if proc.returncode != 0:  # nothing more is started on the GPU after a failure
                        sys.exit(f"{' '.join(cmd[4:])} ended with {proc.returncode}:\n{proc.stdout}\n{proc.stderr[-2000:]}")
                    f.write(proc.stdout.strip().splitlines()[-1] + "\n")
                    f.flush()
                    print(proc.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
