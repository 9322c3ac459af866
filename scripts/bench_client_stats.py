"""Time one local iteration's client statistics (client.py:69-86) on the GPU,
two ways on the same device and tensors:

  torch : the reference's own expression sequence (ClientStepStats(stats="torch"):
          torch.cat, isnan().sum(), norms, tensor truth tests) -- the baseline;
  hip   : the fused passes (fedavg_client_stats_f32 twice + fedavg_client_track,
          or their bf16 / fp16 / fp64 forms of libfedavg_amd_clientvec.so)
          with their one sync.

    python scripts/bench_client_stats.py [--dtype f32|bf16|f16|f64] [--reps 30]
                                         [--out profiles/client_stats/NAME.jsonl]

Per shape: the median over --reps repetitions (after warm-up) of the hipEvent
time around after_backward() + after_step(), the host syncs per iteration,
and for the fused pass alone the median time of one pass (10 back-to-back
passes between two events, table staging and finalize included) with the
achieved bytes/s on the algorithmic bytes per element (read cur, read snap,
write snap: 12 B for fp32, 6 B for bf16 / fp16, 24 B for fp64) against 8 TB/s.
A pass whose tensors and snapshot (two elements' bytes per element) fit the
256 MB Infinity Cache is labelled cache-resident; larger models rotate over
several parameter sets so that every pass reads from HBM.
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import mfl_amd  # noqa: E402
from model_shapes import CONFIGS  # noqa: E402

PEAK = 8.0e12
MALL = 256 << 20
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


def param_shapes(name):
    """The model's parameters (what net.parameters() yields): no BatchNorm statistics."""
    _, shapes = CONFIGS[name]
    return [s for k, s in shapes if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


SHAPES = {
    "mnist_lr": lambda: param_shapes("mnist_lr"),
    "femnist_cnn": lambda: param_shapes("femnist_cnn"),
    "resnet56": lambda: param_shapes("resnet56"),
    "resnet18_gn": lambda: param_shapes("resnet18_gn"),
    "flat_25m": lambda: [(25_000_000,)],
}


def make_params(shapes, dev, seed, dtype=torch.float32):
    g = torch.Generator(device=dev).manual_seed(seed)
    params = []
    for s in shapes:
        p = torch.nn.Parameter((torch.randn(s, device=dev, generator=g) * 0.05).to(dtype))
        p.grad = (torch.randn(s, device=dev, generator=g) * 1e-3).to(dtype)
        params.append(p)
    return params


def step(params, scale=1e-3):
    """What a local iteration changes between two statistics calls (not timed)."""
    with torch.no_grad():
        for p in params:
            p.add_(p.grad, alpha=-scale)
            p.grad.mul_(0.999)


def time_iteration(stats, params, reps, warmup):
    loss = torch.tensor(1.25, device=params[0].device)
    stats.begin(1.3)
    times, syncs = [], []
    for i in range(warmup + reps):
        step(params)
        torch.cuda.synchronize()
        s0 = stats.host_syncs
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        trip = stats.after_backward(loss, 0.03, 1e9)
        assert not trip
        stats.after_step(1.25, 1.3)
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b) * 1e3)
            syncs.append(stats.host_syncs - s0)
    return statistics.median(times), min(times), max(syncs)


def time_pass(sets, reps, warmup, inner=10):
    """One fused pass (weights against their snapshot), rotating over the parameter sets."""
    times = []
    k = 0
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            sets[k % len(sets)]._pass("w", 1)
            k += 1
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dtype = DTYPES[args.dtype]
    es = torch.empty((), dtype=dtype).element_size()
    assert args.reps >= 20, "medians of at least 20 repetitions"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    for name in args.shapes.split(","):
        shapes = SHAPES[name]()
        P = sum(math.prod(s) for s in shapes)
        params = make_params(shapes, dev, 0, dtype)
        t_torch, t_torch_min, _ = time_iteration(mfl_amd.ClientStepStats(params, stats="torch"), params, args.reps,
                                                 args.warmup)
        fused = mfl_amd.ClientStepStats(params, stats="hip")
        t_hip, t_hip_min, syncs = time_iteration(fused, params, args.reps, args.warmup)
        resident = 2 * es * P <= MALL
        n_sets = 1 if 2 * es * P < (32 << 20) else max(2, math.ceil((512 << 20) / (2 * es * P)))
        sets = [fused]
        for r in range(1, n_sets):
            extra = mfl_amd.ClientStepStats(make_params(shapes, dev, r, dtype), stats="hip")
            extra.begin(1.3)
            sets.append(extra)
        t_pass, t_pass_min = time_pass(sets, args.reps, args.warmup)
        line = {
            "shape": name, "dtype": args.dtype, "P": P, "keys": len(shapes), "reps": args.reps,
            "torch_us_median": round(t_torch, 2), "torch_us_min": round(t_torch_min, 2),
            # :71 isnan().sum() > 0, isnan(loss), the norm test; :75 item(); :79 and :83 one or two truth tests each
            "torch_host_syncs": "6-8",
            "hip_us_median": round(t_hip, 2), "hip_us_min": round(t_hip_min, 2), "hip_host_syncs": syncs,
            "speedup": round(t_torch / t_hip, 3),
            "pass_us_median": round(t_pass, 2), "pass_us_min": round(t_pass_min, 2),
            "pass_bytes": 3 * es * P, "pass_gbps": round(3 * es * P / (t_pass * 1e-6) / 1e9, 1),
            "pass_frac_of_8tbps": round(3 * es * P / (t_pass * 1e-6) / PEAK, 4),
            "pass_parameter_sets": n_sets,
            "memory": ("cache-resident" if n_sets == 1 else f"rotating over {n_sets} sets of {2 * es * P >> 20} MB"
                       + (" (one set fits the Infinity Cache)" if resident else "")),
            "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
        }
        print(json.dumps(line), flush=True)
        lines.append(line)
        del sets, fused, params
        torch.cuda.empty_cache()
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
