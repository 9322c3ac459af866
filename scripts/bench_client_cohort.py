"""A round's linear clients: one ``cohort_train`` launch against K sequential ``client_train(loop="linear")`` calls.

    python scripts/bench_client_cohort.py                  # every configuration, one child process each
    python scripts/bench_client_cohort.py --one 64 sgd 100 # one configuration, one JSON line

Workload: MNIST-LR shapes (D = 784, C = 10), B = 64 and B = 600 samples per client, 10 local iterations, SGD and
Adam, K in 1, 10, 100, 256, 512 clients that all start from the same global model.  Both arms run in the same
process, alternated (sequential, cohort, sequential, ...), 3 warm-up pairs and then 30 timed pairs; a time is host
wall clock around the arm including its host syncs, and the line holds the medians, the extremes and whether the
cohort was below the sequential arm in EVERY pair (``all_below``; without it nothing is called faster).  The
sequential arm restores the model from the global parameters before each client (two device copies), as every client
of a round starts from the global model.  For K = 100 a second pair of arms adds the round's aggregate: cohort +
``reduce_with_sqdist`` on its rows against sequential + packing the K results into rows + the same reduce.

The driver runs each configuration as a child process under its own time limit and stops at the first that fails;
lines go to profiles/client_cohort/mi355x_client_cohort.jsonl.

    python scripts/bench_client_cohort.py --split                  # the same grid with a third arm
    python scripts/bench_client_cohort.py --split --one 600 sgd 10

``--split`` rotates a third arm with the two, ``cohort_train(split=True)`` at its default ``slices_per_group``
(sequential, cohort, split, sequential, ...), and at B = 600 four more, the sweep ``slices_per_group`` = 1, 2, 4, 8.
A line holds every arm's median and extremes, the default and, per split arm, ``split_below_cohort_every_pair``:
whether that arm was below the one-workgroup cohort of the same rotation in EVERY rotation.  No round arms; lines go
to profiles/client_cohort/mi355x_cohort_split.jsonl.
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
OUT = ROOT / "profiles" / "client_cohort" / "mi355x_client_cohort.jsonl"
SPLIT_OUT = ROOT / "profiles" / "client_cohort" / "mi355x_cohort_split.jsonl"
SWEEP_B, SWEEP_Q = 600, (1, 2, 4, 8)
D, C, ITERS, WARMUP, REPEATS = 784, 10, 10, 3, 30
KS, BS, OPTIMIZERS = (1, 10, 100, 256, 512), (64, 600), ("sgd", "adam")
HYPER = {"sgd": dict(lr=0.05, wd=0.0), "adam": dict(lr=0.001, wd=0.001)}
LIMIT_S = 240  # per child


def one(B, optimizer, K, split=False):
    import torch

    import mfl_amd
    from linear_loop_ref import make_client

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(B + K)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(D, C)).to(dev)
    w0, b0 = net[1].weight.detach().clone(), net[1].bias.detach().clone()
    clients = [make_client(torch.randn(B, D, generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev), dev,
                           optimizer, ratio=1e4, **HYPER[optimizer]) for _ in range(K)]
    weights = mfl_amd.weights_tensor(mfl_amd.sample_weights([B] * K), torch.float32, dev)
    P = C * D + C
    rows = torch.zeros(K, -(-P // mfl_amd.ALIGN_ELEMS) * mfl_amd.ALIGN_ELEMS, device=dev)
    packed = torch.zeros_like(rows)

    def sequential(pack):
        for k, c in enumerate(clients):
            with torch.no_grad():
                net[1].weight.copy_(w0)
                net[1].bias.copy_(b0)
            sd = mfl_amd.client_train(c, net, ITERS, loop="linear", keep_on_device=True)[0]
            if pack:
                packed[k, :P] = torch.cat([sd["1.weight"].reshape(-1), sd["1.bias"]])
        if pack:
            mfl_amd.reduce_with_sqdist(packed, weights, P)
            torch.cuda.synchronize()

    def cohort(reduce):
        with torch.no_grad():
            net[1].weight.copy_(w0)
            net[1].bias.copy_(b0)
        res = mfl_amd.cohort_train(clients, net, ITERS, rows=rows)
        if reduce:
            mfl_amd.reduce_with_sqdist(res.rows, weights, res.P)
            torch.cuda.synchronize()

    def timed(fn, arg):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(arg)
        return (time.perf_counter() - t) * 1e3

    line = dict(workload="mnist_lr", B=B, D=D, C=C, iters=ITERS, optimizer=optimizer, K=K, repeats=REPEATS,
                device=torch.cuda.get_device_name(0), torch=torch.__version__)
    if split:
        from mfl_amd.client_passes import cosplit_default_slices, cosplit_groups

        def split_arm(q):
            with torch.no_grad():
                net[1].weight.copy_(w0)
                net[1].bias.copy_(b0)
            mfl_amd.cohort_train(clients, net, ITERS, rows=rows, split=True, slices_per_group=q)

        qs = [None] + (list(SWEEP_Q) if B == SWEEP_B else [])
        turns = [(timed(sequential, False), timed(cohort, False), [timed(split_arm, q) for q in qs])
                 for _ in range(WARMUP + REPEATS)][WARMUP:]
        seq, coh = [t[0] for t in turns], [t[1] for t in turns]

        def arm(i):
            ms = [t[2][i] for t in turns]
            q = qs[i] or cosplit_default_slices([B] * K, D)
            return dict(slices_per_group=q, groups=cosplit_groups([B] * K, D, q), split_ms=statistics.median(ms),
                        split_min_max=[min(ms), max(ms)], split_below_cohort_every_pair=all(m < c for m, c in zip(ms, coh)))

        line["train"] = dict(sequential_ms=statistics.median(seq), cohort_ms=statistics.median(coh),
                             sequential_min_max=[min(seq), max(seq)], cohort_min_max=[min(coh), max(coh)], **arm(0))
        line["split_below_cohort_every_pair"] = line["train"]["split_below_cohort_every_pair"]
        line["sweep"] = [arm(i) for i in range(1, len(qs))]
        print(json.dumps(line), flush=True)
        return
    for tag, arg in (("train", False), ("round", True)) if K == 100 else (("train", False),):
        pairs = [(timed(sequential, arg), timed(cohort, arg)) for _ in range(WARMUP + REPEATS)][WARMUP:]
        seq, coh = [p[0] for p in pairs], [p[1] for p in pairs]
        line[tag] = dict(sequential_ms=statistics.median(seq), cohort_ms=statistics.median(coh),
                         sequential_min_max=[min(seq), max(seq)], cohort_min_max=[min(coh), max(coh)],
                         all_below=all(c < s for s, c in pairs))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--one", nargs=3, metavar=("B", "OPTIMIZER", "K"))
    ap.add_argument("--split", action="store_true", help="rotate cohort_train(split=True) with the two arms")
    ap.add_argument("--out", type=Path)
    a = ap.parse_args()
    if a.one:
        return one(int(a.one[0]), a.one[1], int(a.one[2]), a.split)
    out = a.out or (SPLIT_OUT if a.split else OUT)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as f:
        for B in BS:
            for optimizer in OPTIMIZERS:
                for K in KS:
                    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--one", str(B), optimizer, str(K)]
                    cmd += ["--split"] if a.split else []
                    proc = subprocess.run(cmd, capture_output=True, text=True)
                    if proc.returncode != 0:  # nothing more is started on the GPU after a failure
                        sys.exit(f"{' '.join(cmd[4:])} ended with {proc.returncode}:\n{proc.stdout}\n{proc.stderr[-2000:]}")
                    f.write(proc.stdout.strip().splitlines()[-1] + "\n")
                    f.flush()
                    print(proc.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
