"""A device-resident round's bf16 / fp16 / fp64 group: packed rows against zero-copy.

    python scripts/bench_device_round_vec.py [--out profiles/device_round_vec/bench.jsonl]
                                             [--dtypes bf16,fp16,fp64] [--K 10,32,64,100,128]
                                             [--shapes resnet18_gn,flat_25m]

For every dtype x shape x K, in one process, on K clients whose keys are
separately allocated device tensors: (a) today's route, fedavg_pack_rows_device
into [K, ld] staging rows followed by fedavg_reduce_sqdist_{f64,f16,bf16}
(libfedavg_amd_fusedvec.so), and (b) fedavg_device_round_{f64,f16,bf16}
(libfedavg_amd_segvec.so), straight from the clients' tensors.  Both go
through the C ABI on buffers, tables and workspaces allocated once, so the
events bracket the calls (their table staging and H2D included) and nothing
else.  hipEvents, 5 warm-ups, then 30 repetitions that ALTERNATE the two
routes (a, b, a, b, ...), the median of each.  Before a cell is timed (b)'s
`out` is compared with (a)'s bit for bit and `sumsq` within 2 (P + 1) 2^-53
relative; a cell that differs ends the run.  One JSON line per cell: both
times, their ratio and each route's share of 8 TB/s on the algorithmic bytes,
elem_size * (K * P + P).  fp64 stops at 64 clients (the library's bands).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from mfl_amd import _lib  # noqa: E402
from model_shapes import resnet18_gn_shapes  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp64": torch.float64}
SUFFIX = {"bf16": "bf16", "fp16": "f16", "fp64": "f64"}
SHAPES = {"resnet18_gn": [int(np.prod(s)) for _, s in resnet18_gn_shapes()], "flat_25m": [25_000_000]}
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
    ap.add_argument("--shapes", default="resnet18_gn,flat_25m")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib, fv, sv = _lib.load(), _lib.load_fusedvec(), _lib.load_segvec()
    st = torch.cuda.current_stream(dev).cuda_stream
    lines = []
    for name in args.dtypes.split(","):
        dtype = DTYPES[name]
        es = torch.empty((), dtype=dtype).element_size()
        for shape in args.shapes.split(","):
            numel = np.array(SHAPES[shape], dtype=np.int64)
            n, P = len(numel), int(numel.sum())
            offset = np.concatenate([[0], np.cumsum(numel)[:-1]]).astype(np.int64)
            ld = (P + 63) // 64 * 64
            for K in (int(v) for v in args.K.split(",")):
                plan = sv.fedavg_device_round_vec_plan_of(K, es, int(dtype == torch.bfloat16))
                if not plan:
                    continue
                # the clients: one allocation per key and client, as separately trained models hold them
                clients = [[(torch.randn(int(m), device=dev, dtype=torch.float32) * 0.05).to(dtype) for m in numel]
                           for _ in range(K)]
                ptrs = np.array([[t.data_ptr() for t in c] for c in clients], dtype=np.int64)
                w64 = np.full(K, 1.0 / K)
                w_dev = torch.tensor(w64, dtype=torch.float64 if es == 8 else torch.float32, device=dev)
                # (a) pack + the one-read rows kernel
                items = np.empty((K, n, 4), dtype=np.int64)
                items[:, :, 0] = ptrs
                items[:, :, 1] = numel
                items[:, :, 2] = (np.arange(K, dtype=np.int64) * ld)[:, None] + offset[None, :]
                items[:, :, 3] = 0
                items = items.reshape(K * n, 4)
                rows = torch.empty((K, ld), dtype=dtype, device=dev)
                pk_need = lib.fedavg_pack_rows_device_workspace(K * n)
                pk_h = torch.empty(pk_need, dtype=torch.uint8, pin_memory=True)
                pk_d = torch.empty(pk_need, dtype=torch.uint8, device=dev)
                na = fv.fedavg_reduce_sqdist_vec_workspace(K, P, es)
                ws_a = torch.empty(na, dtype=torch.float64, device=dev)
                out_a, out_b = (torch.empty(P, dtype=dtype, device=dev) for _ in range(2))
                s_a, s_b = (torch.empty(K, dtype=torch.float64, device=dev) for _ in range(2))
                pack = lib.fedavg_pack_rows_device
                fused = getattr(fv, f"fedavg_reduce_sqdist_{SUFFIX[name]}")
                # (b) the zero-copy call
                nb = sv.fedavg_device_round_vec_partials(K, es)
                ws_b = torch.empty(nb, dtype=torch.float64, device=dev)
                tb_need = sv.fedavg_device_round_vec_workspace(K, n)
                tb_h = torch.empty(tb_need, dtype=torch.uint8, pin_memory=True)
                tb_d = torch.empty(tb_need, dtype=torch.uint8, device=dev)
                zero = getattr(sv, f"fedavg_device_round_{SUFFIX[name]}")

                def route_a():
                    _lib.check(pack(items.ctypes.data, K * n, rows.data_ptr(), es, pk_h.data_ptr(), pk_d.data_ptr(),
                                    pk_need, st), "fedavg_pack_rows_device")
                    _lib.check_fusedvec(fused(rows.data_ptr(), K, P, ld, w_dev.data_ptr(), out_a.data_ptr(),
                                              ws_a.data_ptr(), na, s_a.data_ptr(), st), "fedavg_reduce_sqdist")

                def route_b():
                    _lib.check_segvec(zero(ptrs.ctypes.data, n, None, numel.ctypes.data, offset.ctypes.data, n, K,
                                           w64.ctypes.data, out_b.data_ptr(), ws_b.data_ptr(), nb, s_b.data_ptr(),
                                           tb_h.data_ptr(), tb_d.data_ptr(), tb_need, st), "fedavg_device_round")

                route_a()
                torch.cuda.synchronize()  # the pinned tables are rewritten per call: each call's H2D has run
                route_b()
                torch.cuda.synchronize()
                ibits = torch.int64 if es == 8 else torch.int16
                if not torch.equal(out_a.view(ibits), out_b.view(ibits)):
                    raise SystemExit(f"{name} {shape} K={K}: the routes' averages differ")
                rel = float(((s_b - s_a).abs() / s_a.abs().clamp_min(1e-300)).max())
                if not rel <= 2 * (P + 1) * 2.0 ** -53:
                    raise SystemExit(f"{name} {shape} K={K}: the routes' sums differ by {rel:.3e} relative")
                ta, ta_min, tb, tb_min = timed_pair(route_a, route_b)
                alg = es * (K * P + P)
                row = {"dtype": name, "shape": shape, "keys": n, "K": K, "P": P, "plan": plan,
                       "pack_ms": round(ta, 4), "zero_copy_ms": round(tb, 4), "pack_min_ms": round(ta_min, 4),
                       "zero_copy_min_ms": round(tb_min, 4), "ratio": round(ta / tb, 3), "sumsq_rel_diff": rel,
                       "pack_share_of_8TBs": round(alg / (ta * 1e-3) / PEAK_BYTES_PER_S, 3),
                       "zero_copy_share_of_8TBs": round(alg / (tb * 1e-3) / PEAK_BYTES_PER_S, 3)}
                print(json.dumps(row), flush=True)
                lines.append(row)
                del clients, rows, out_a, out_b, ws_a, ws_b
                torch.cuda.empty_cache()
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(r) + "\n" for r in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
