"""Host time of one native call of the fused passes, for comparing two builds.

    python scripts/host_call_cost.py [--lib-dir DIR] [--reps 200] [--warmup 30]

Loads DIR/libfedavg_amd.so (default: the package's lib/) and times, per call
and on the host alone (the stream is synchronized outside the timed region),
fedavg_reduce_sqdist_f32 at 10 x 7850 and 100 x 600372,
fedavg_client_sqdist_f32 and fedavg_client_sqdist_workspace at 100 x 600372
and fedavg_device_round_f32 at resnet56 x 100.  These rounds are launch-bound:
the figures are the cost of the plan, the occupancy lookups, the workspace
check and the launches.  One JSON line with the medians in microseconds.
Compare builds by alternating processes on one machine (A, B, A): the spread
of the two A runs is the noise floor.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import numpy as np
import torch

from mfl_amd import _lib
from model_shapes import resnet56_shapes


def typed(path):
    lib = ctypes.CDLL(str(path))
    for name in ("fedavg_reduce_sqdist_workspace", "fedavg_reduce_sqdist_f32", "fedavg_client_sqdist_workspace",
                 "fedavg_client_sqdist_f32", "fedavg_reduce_sqdist_segments_partials",
                 "fedavg_device_round_scratch", "fedavg_device_round_workspace", "fedavg_device_round_f32"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def median_us(call, reps, warmup):
    for _ in range(warmup):
        assert call() == 0
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
    return round(float(np.median(ts)), 2)


def rows_call(lib, dev, K, P):
    ld = (P + 63) // 64 * 64
    x = torch.zeros((K, ld), device=dev)
    w = torch.full((K,), 1.0 / K, device=dev)
    out = torch.empty(P, device=dev)
    sumsq = torch.empty(K, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.fedavg_reduce_sqdist_workspace(K, P), dtype=torch.float64, device=dev)
    return lambda: lib.fedavg_reduce_sqdist_f32(x.data_ptr(), K, P, ld, w.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                ws.numel(), sumsq.data_ptr(), None)


def dist_call(lib, dev, K, P):
    ld = (P + 63) // 64 * 64
    x = torch.zeros((K, ld), device=dev)
    glob = torch.zeros(ld, device=dev)
    sumsq = torch.empty(K, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.fedavg_client_sqdist_workspace(K, P), dtype=torch.float64, device=dev)
    return lambda: lib.fedavg_client_sqdist_f32(x.data_ptr(), K, P, ld, glob.data_ptr(), ws.data_ptr(), ws.numel(),
                                                sumsq.data_ptr(), None)


def round_call(lib, dev, K):
    shapes = resnet56_shapes()
    numel = np.array([int(np.prod(s, dtype=np.int64)) for _, s in shapes], dtype=np.int64)
    kind = np.array([1 if n.endswith("num_batches_tracked") else 0 for n, _ in shapes], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(numel)[:-1]]).astype(np.int64)
    n = len(numel)
    # client k's key j: row k of keys[j], rows 16-B aligned
    keys = [torch.zeros((K, 2), dtype=torch.int64, device=dev) if kd else
            torch.zeros((K, (int(m) + 3) // 4 * 4), device=dev) for m, kd in zip(numel, kind)]
    ptrs = np.array([[keys[j][k].data_ptr() for j in range(n)] for k in range(K)], dtype=np.int64)
    w64 = np.full(K, 1.0 / K, dtype=np.float64)
    out = torch.empty(int(numel.sum()), device=dev)
    sumsq = torch.empty(K, dtype=torch.float64, device=dev)
    partials = torch.empty(lib.fedavg_reduce_sqdist_segments_partials(K), dtype=torch.float64, device=dev)
    scr = torch.empty(max(1, lib.fedavg_device_round_scratch(numel.ctypes.data, kind.ctypes.data, n, K)), device=dev)
    nws = lib.fedavg_device_round_workspace(K, n)
    ws_h = torch.empty(nws, dtype=torch.uint8, pin_memory=True)
    ws_d = torch.empty(nws, dtype=torch.uint8, device=dev)
    return lambda _alive=keys: lib.fedavg_device_round_f32(ptrs.ctypes.data, n, None, numel.ctypes.data, offset.ctypes.data,
                                               kind.ctypes.data, n, K, w64.ctypes.data, out.data_ptr(),
                                               partials.data_ptr(), partials.numel(), sumsq.data_ptr(), scr.data_ptr(),
                                               scr.numel(), ws_h.data_ptr(), ws_d.data_ptr(), nws, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-dir", type=Path, default=_lib.LIB_PATH.parent)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = typed(args.lib_dir / _lib.LIB_PATH.name)
    res = {"label": args.label, "lib_dir": str(args.lib_dir), "reps": args.reps}
    for name, call in (("reduce_sqdist_f32_10x7850_us", rows_call(lib, dev, 10, 7850)),
                       ("reduce_sqdist_f32_100x600372_us", rows_call(lib, dev, 100, 600372)),
                       ("client_sqdist_f32_100x600372_us", dist_call(lib, dev, 100, 600372)),
                       ("client_sqdist_workspace_100x600372_us",
                        lambda: 0 * lib.fedavg_client_sqdist_workspace(100, 600372)),
                       ("device_round_f32_resnet56x100_us", round_call(lib, dev, 100))):
        res[name] = median_us(call, args.reps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
