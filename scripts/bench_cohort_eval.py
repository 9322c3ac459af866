"""Every client's evaluation: one ``cohort_test`` call against K sequential ``Client.local_test`` bodies.

    python scripts/bench_cohort_eval.py                # every configuration, one child process each
    python scripts/bench_cohort_eval.py --one 600 2000 # one configuration, one JSON line

Workload: MNIST-LR shapes (D = 784, C = 10, sigmoid), K in 100, 1000, 2000 clients (2000: a test and a train table of
1000 clients in one set), B = 64, B = 600 and a mixed table (B = "mixed": sizes 10 to 1000, seeded).  The baseline is
what the parent commit offers for this call: the reference's loop, K times the torch expressions of client.py:110-118
(forward, criterion, ``torch.max``, two ``.item()`` syncs) on the same GPU with every batch already resident.  Both
arms run in the same process, alternated (loop, cohort_test, loop, ...), 3 warm-up pairs and then 30 timed pairs; a time
is host wall clock around the arm including its host syncs, and the line holds the medians, the extremes and whether
``cohort_test`` was below the loop in EVERY pair (``all_below``; without it nothing is called faster).  The ``EvalSet``
is built once outside the timed region (``build_ms``: drawing, uploading, the table and the workspace).  ``device_ms``
is the median of the call's time on the stream between two events, and ``x_gb_per_s`` the bytes of x over it, against
the 8 TB/s HBM peak of the MI355X.

The driver runs each configuration as a child process under its own time limit and stops at the first that fails;
lines go to profiles/client_eval/mi355x_cohort_eval.jsonl.
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
OUT = ROOT / "profiles" / "client_eval" / "mi355x_cohort_eval.jsonl"
D, C, WARMUP, REPEATS = 784, 10, 3, 30
KS, BS = (100, 1000, 2000), ("64", "600", "mixed")
HBM_PEAK_GB_S = 8000.0
LIMIT_S = 240  # per child


def one(B, K):
    import torch

    import mfl_amd

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(K)
    sizes = torch.randint(10, 1001, (K,), generator=g).tolist() if B == "mixed" else [int(B)] * K
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(D, C), torch.nn.Sigmoid()).to(dev)
    criterion = torch.nn.CrossEntropyLoss().to(dev)
    batches = [(torch.randn(n, D, generator=g).to(dev), torch.randint(0, C, (n,), generator=g).to(dev)) for n in sizes]
    torch.cuda.synchronize()
    t = time.perf_counter()
    evalset = mfl_amd.EvalSet([[batch] for batch in batches], dev, criterion)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t) * 1e3

    def loop():
        out = []
        net.eval()
        with torch.no_grad():
            for x, target in batches:  # client.py:110-118
                pred = net(x)
                loss = criterion(pred, target)
                _, predicted = torch.max(pred, -1)
                correct = predicted.eq(target).sum()
                out.append({"test_correct": correct.item(), "test_loss": loss.item() * target.size(0),
                            "test_total": target.size(0)})
        return out

    def cohort():
        return mfl_amd.cohort_test(net, evalset, loop="linear_sigmoid")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    want, got = loop(), cohort()
    assert [m["test_correct"] for m in want] == [m["test_correct"] for m in got]  # the arms compute the same thing
    pairs = [(timed(loop), timed(cohort)) for _ in range(WARMUP + REPEATS)][WARMUP:]
    device = []
    for _ in range(REPEATS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        cohort()
        stop.record()
        stop.synchronize()
        device.append(start.elapsed_time(stop))
    seq, coh = [p[0] for p in pairs], [p[1] for p in pairs]
    device_ms, x_bytes = statistics.median(device), 4 * D * sum(sizes)
    print(json.dumps(dict(
        workload="mnist_lr_eval", B=B, D=D, C=C, K=K, rows=sum(sizes), repeats=REPEATS, build_ms=build_ms,
        loop_ms=statistics.median(seq), cohort_test_ms=statistics.median(coh), loop_min_max=[min(seq), max(seq)],
        cohort_test_min_max=[min(coh), max(coh)], all_below=all(c < s for s, c in pairs), device_ms=device_ms,
        x_gb_per_s=x_bytes / device_ms / 1e6, hbm_peak_fraction=x_bytes / device_ms / 1e6 / HBM_PEAK_GB_S,
        device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--one", nargs=2, metavar=("B", "K"))
    ap.add_argument("--out", type=Path, default=OUT)
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], int(a.one[1]))
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with a.out.open("w") as f:
        for B in BS:
            for K in KS:
                cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--one", B, str(K)]
                proc = subprocess.run(cmd, capture_output=True, text=True)
                if proc.returncode != 0:  # nothing more is started on the GPU after a failure
                    sys.exit(f"{' '.join(cmd[4:])} ended with {proc.returncode}:\n{proc.stdout}\n{proc.stderr[-2000:]}")
                f.write(proc.stdout.strip().splitlines()[-1] + "\n")
                f.flush()
                print(proc.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
