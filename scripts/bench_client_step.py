"""Time one local iteration's "step + weight bookkeeping" (client.py:74-86) on
the GPU, three ways on the same device and tensors:

  ref    : the reference's torch expressions (optimizer.step(), then
           ClientStepStats(stats="torch").after_step(): torch.cat, w - last_w,
           norms, tensor truth tests);
  torch  : step="torch" -- optimizer.step(), then the fused weight pass
           (fedavg_client_stats_*) and fedavg_client_track*;
  fused  : step="fused" -- one fedavg_client_sgd_step_* and fedavg_client_track*.

    python scripts/bench_client_step.py [--dtypes f32,bf16] [--reps 30] [--out-dir profiles/client_step]

Per shape and dtype: the median over --reps repetitions (after warm-up) of the
hipEvent time around exactly those calls; the gradient pass and the guard's
sync (after_backward) run before each repetition, untimed, as the loop has
them.  "torch" and "fused" are measured three times each, alternating, in the
same process: the figures are the medians of the three medians, and the spread
is the min-max of the three "torch" medians.  "ok" says that fused is not
slower than torch beyond that spread (fused <= the largest torch median).
The algorithmic bytes per element: torch 6 elements' bytes (step: read w, read
g, write w; pass: read w, read snapshot, write snapshot), fused 3.
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
from bench_client_stats import DTYPES, SHAPES, make_params  # noqa: E402

LR = 0.03


def time_variant(params, reps, warmup, **kw):
    """Median and minimum us of the step + weight bookkeeping of one iteration."""
    stats = mfl_amd.ClientStepStats(params, **kw)
    opt = torch.optim.SGD(params, lr=LR)
    fused = stats.step_mode == "fused"
    loss = torch.tensor(1.25, device=params[0].device)
    stats.begin(1.3)
    times = []
    for i in range(warmup + reps):
        assert not stats.after_backward(loss, LR, 1e9)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if fused:
            stats.sgd_step(LR, 1.25, 1.3)
        else:
            opt.step()
            stats.after_step(1.25, 1.3)
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--out-dir", default="")
    args = ap.parse_args()
    assert args.reps >= 20, "medians of at least 20 repetitions"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for key in args.dtypes.split(","):
        dtype = DTYPES[key]
        es = torch.empty((), dtype=dtype).element_size()
        form = mfl_amd.client_stats.sgd_form(dev, dtype)
        lines = []
        for name in args.shapes.split(","):
            shapes = SHAPES[name]()
            P = sum(math.prod(s) for s in shapes)
            # gradients of 1e-3 * N(0, 1): the weights stay model-like over the run's steps
            params = make_params(shapes, dev, 0, dtype)
            ref, ref_min = time_variant(params, args.reps, args.warmup, stats="torch")
            runs = {"torch": [], "fused": []}
            for _ in range(3):
                for mode in ("torch", "fused"):
                    runs[mode].append(time_variant(params, args.reps, args.warmup, stats="hip", step=mode)[0])
            t_torch, t_fused = statistics.median(runs["torch"]), statistics.median(runs["fused"])
            line = {
                "shape": name, "dtype": key, "P": P, "keys": len(shapes), "reps": args.reps, "lr": LR, "form": form,
                "ref_us_median": round(ref, 2), "ref_us_min": round(ref_min, 2),
                "torch_us_median": round(t_torch, 2), "torch_us_repeats": [round(t, 2) for t in runs["torch"]],
                "fused_us_median": round(t_fused, 2), "fused_us_repeats": [round(t, 2) for t in runs["fused"]],
                "speedup_over_torch": round(t_torch / t_fused, 3), "speedup_over_ref": round(ref / t_fused, 3),
                "ok": bool(t_fused <= max(runs["torch"])),
                "torch_bytes": 6 * es * P, "fused_bytes": 3 * es * P,
                "fused_gbps": round(3 * es * P / (t_fused * 1e-6) / 1e9, 1),
                "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
            }
            print(json.dumps(line), flush=True)
            lines.append(line)
            del params
            torch.cuda.empty_cache()
        if args.out_dir:
            out = Path(args.out_dir) / f"mi355x_step_{key}.jsonl"
            out.parent.mkdir(parents=True, exist_ok=True)
            out.write_text("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
