"""Aggregate + :291 sums for bf16 / fp16 / fp64 rows: two passes against one.

    python scripts/bench_fused_vec.py [--out profiles/fused_vec/bench.jsonl]
                                      [--dtypes bf16,fp16,fp64] [--K 10,32,64,100,128]
                                      [--P 1200000,11200000,25000000]

For every dtype x K x P, in one process: (a) fedavg_reduce_* then
fedavg_client_sqdist_* (the two passes) and (b) fedavg_reduce_sqdist_* (the
entry of libfedavg_amd_fusedvec.so; the plan says whether it fuses).  Both
are called through the C ABI on buffers and workspaces allocated once, so the
events bracket the launches and nothing else.  hipEvents, 5 warm-ups, then 30
repetitions that ALTERNATE the two routes (a, b, a, b, ...), the median of
each.  Before a cell is timed its two routes' outputs are compared: `out` bit
for bit, `sumsq` within 2 (P + 1) 2^-53 relative; a cell that differs ends
the run.  One JSON line per cell: both times, their ratio and the one call's
share of 8 TB/s on its algorithmic bytes, elem_size * (K * P + P).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import mfl_amd  # noqa: E402
from mfl_amd import _lib  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp64": torch.float64}
SUFFIX = {"bf16": "bf16", "fp16": "f16", "fp64": "f64"}
PEAK_BYTES_PER_S = 8e12


def timed_pair(fa, fb, warmup=5, reps=30):
    """Median (and minimum) of ``reps`` timings of each route, alternating."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return statistics.median(ta), min(ta), statistics.median(tb), min(tb)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--dtypes", default="bf16,fp16,fp64")
    ap.add_argument("--K", default="10,32,64,100,128")
    ap.add_argument("--P", default="1200000,11200000,25000000")
    ap.add_argument("--max-bytes", type=float, default=40e9, help="skip cells whose rows exceed this")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib, fv = _lib.load(), _lib.load_fusedvec()
    lines = []
    for name in args.dtypes.split(","):
        dtype = DTYPES[name]
        es = torch.empty((), dtype=dtype).element_size()
        for P in (int(v) for v in args.P.split(",")):
            for K in (int(v) for v in args.K.split(",")):
                ld = (P + 63) // 64 * 64
                if K * ld * es > args.max_bytes:
                    continue
                x = (torch.randn((K, ld), device=dev, dtype=torch.float32) * 0.05).to(dtype)
                w = mfl_amd.weights_tensor([1.0 / K] * K, dtype, dev)
                red, sq, fused = (getattr(lib, f"fedavg_reduce_{SUFFIX[name]}"),
                                  getattr(lib, f"fedavg_client_sqdist_{SUFFIX[name]}"),
                                  getattr(fv, f"fedavg_reduce_sqdist_{SUFFIX[name]}"))
                n2 = lib.fedavg_client_sqdist_workspace_elems(K, P, es)
                n1 = fv.fedavg_reduce_sqdist_vec_workspace(K, P, es)
                ws2 = torch.empty(n2, dtype=torch.float64, device=dev)
                ws1 = torch.empty(n1, dtype=torch.float64, device=dev)
                out2, out1 = (torch.empty(P, dtype=dtype, device=dev) for _ in range(2))
                s2, s1 = (torch.empty(K, dtype=torch.float64, device=dev) for _ in range(2))
                st = torch.cuda.current_stream(dev).cuda_stream
                xp, wp = x.data_ptr(), w.data_ptr()

                def two():
                    _lib.check(red(xp, K, P, ld, wp, out2.data_ptr(), st), "reduce")
                    _lib.check(sq(xp, K, P, ld, out2.data_ptr(), ws2.data_ptr(), n2, s2.data_ptr(), st), "client_sqdist")

                def one():
                    _lib.check_fusedvec(fused(xp, K, P, ld, wp, out1.data_ptr(), ws1.data_ptr(), n1, s1.data_ptr(), st),
                                        "reduce_sqdist")

                two()
                one()
                torch.cuda.synchronize()
                ibits = torch.int64 if es == 8 else torch.int16
                if not torch.equal(out1.view(ibits), out2.view(ibits)):
                    raise SystemExit(f"{name} K={K} P={P}: the routes' averages differ")
                rel = float(((s1 - s2).abs() / s2.abs().clamp_min(1e-300)).max())
                if not rel <= 2 * (P + 1) * 2.0 ** -53:
                    raise SystemExit(f"{name} K={K} P={P}: the routes' sums differ by {rel:.3e} relative")
                t2, t2min, t1, t1min = timed_pair(two, one)
                plan = fv.fedavg_fused_vec_plan_of(K, P, es, int(dtype == torch.bfloat16))
                row = {"dtype": name, "K": K, "P": P, "plan": plan, "two_pass_ms": round(t2, 4),
                       "fused_ms": round(t1, 4), "two_pass_min_ms": round(t2min, 4), "fused_min_ms": round(t1min, 4),
                       "ratio": round(t2 / t1, 3), "sumsq_rel_diff": rel,
                       "fused_share_of_8TBs": round(es * (K * P + P) / (t1 * 1e-3) / PEAK_BYTES_PER_S, 3)}
                print(json.dumps(row), flush=True)
                lines.append(row)
                del x, out1, out2, ws1, ws2
                torch.cuda.empty_cache()
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(r) + "\n" for r in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
