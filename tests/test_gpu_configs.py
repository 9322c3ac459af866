"""GPU parity at the BASELINE configurations that need the whole card, and the
RCCL exchange itself.

* cfg4 (fed_cifar100 + resnet18_gn, K = 500 x P = 11,227,812; 22.5 GB of
  rows) and cfg5's per-GPU slice at 8 GPUs (K = 1000 x P = 12,500,000;
  50 GB): the clients are generated on the device by ``mfl_amd.synthetic``
  (a pure function of (client, global column)), reduced by the production
  kernel, and >= 16 windows plus the first and last columns are compared bit
  for bit with the oracle (``oracle/fedavg_oracle.py:reduce_f32``,
  fedavg_trainer.py:450-457) applied to the same inputs regenerated on the
  host by numpy.  A full-length fp64 linearity check bounds the whole vector.
  The same model is then reduced again in the 8-GPU geometry -- every rank's
  block-cyclic chunks on this one GPU, the short-row schedules the N = 8
  pipeline runs -- and each rank's columns must carry the oracle's bits too.
* RCCL: a real ``nccl`` process group at world size 1 on cuda:0 (the
  ``device_id=`` path bench.py uses), ``ShardedReducer`` with the gather
  forced on, 8 chunks: every chunk goes through ``all_gather_into_tensor`` on
  device tensors, ordered after the HIP kernel on the compute stream.  The
  reassembled ``full[:P]`` must be bit-exact against the oracle, and
  ``gather_only`` must rebuild it from ``local_out``.  What this does NOT
  prove: xGMI transport and multi-rank ordering (8-GPU runs are the
  driver's); the gloo tests cover the multi-rank layout.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import fedavg_oracle as O
import mfl_amd
from mfl_amd import synthetic
from mfl_amd.distributed import ShardedReducer, plan_shards

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_available):
    mfl_amd._lib.load()
    torch.cuda.set_device(DEV)
    yield
    torch.cuda.empty_cache()


def _bits(a: np.ndarray, b: np.ndarray, what: str):
    if a.tobytes() != b.tobytes():
        d = np.nonzero(a.view(np.int32) != b.view(np.int32))[0]
        raise AssertionError(f"{what}: {len(d)} mismatches, first {d[:5]}: {a[d[:5]]} vs {b[d[:5]]}")


def _windows(P, n=16, width=4099, seed=0):
    rng = np.random.default_rng(seed)
    starts = [int(s) for s in rng.integers(0, P - width, size=n)] + [0, P - width]
    return [(s, width) for s in starts]


def _linearity(rows, w32, P, out):
    ref = torch.zeros(P, dtype=torch.float64, device=DEV)
    for k in range(rows.shape[0]):
        ref += rows[k, :P].double() * float(w32[k])
    return float((out[:P].double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("K,P,world,chunks", [(500, 11_227_812, 8, 2), (1000, 12_500_000, 1, 8)],
                         ids=["cfg4_resnet18_gn", "cfg5_slice"])
def test_baseline_config_sampled_parity(K, P, world, chunks):
    """(world, chunks): the N = 8 pipeline geometry -- cfg4's 11.2M model over
    8 ranks in 2 chunks each (bench.auto_chunks); the cfg5 slice IS one
    rank's 12.5M-column shard at N = 8, in 8 chunks."""
    ld = (P + 63) // 64 * 64
    rows = torch.empty((K, ld), device=DEV)
    synthetic.fill_rows(rows, [(0, 0, P)])
    weights = mfl_amd.sample_weights(synthetic.sample_counts(K))
    w = mfl_amd.weights_tensor(weights, torch.float32, DEV)
    out = mfl_amd.reduce_packed(rows, w, P)
    torch.cuda.synchronize()
    for s, n in _windows(P):
        exp = O.reduce_f32(synthetic.client_columns_numpy(K, s, n), weights)
        _bits(out[s:s + n].cpu().numpy(), exp, f"K={K} window {s}")
    w32 = np.array(weights, np.float64).astype(np.float32)
    assert _linearity(rows, w32, P, out) < 1e-6

    # the same model in the 8-GPU pipeline geometry: each rank's block-cyclic
    # chunks of the strong-scaled shard, reduced chunk by chunk on this GPU
    for r in sorted({0, world - 1}):
        plan = plan_shards(P, world, r, chunks)
        shard = torch.zeros((K, plan.local_cols), device=DEV)
        for l, g, n in plan.local_segments():
            shard[:, l:l + n] = rows[:, g:g + n]
        local = torch.empty(plan.local_cols, device=DEV)
        S = plan.block
        for c in range(plan.chunks):
            mfl_amd.reduce_packed(shard[:, c * S:(c + 1) * S], w, S, local[c * S:(c + 1) * S])
        torch.cuda.synchronize()
        for l, g, n in plan.local_segments():
            assert torch.equal(local[l:l + n].view(torch.int32), out[g:g + n].view(torch.int32)), (r, g)
            m = min(n, 2048)
            exp = O.reduce_f32(synthetic.client_columns_numpy(K, g + n - m, m), weights)
            _bits(local[l + n - m:l + n].cpu().numpy(), exp, f"rank {r} chunk end {g + n}")
        del shard, local
    del rows, out
    torch.cuda.empty_cache()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def rccl_group():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    assert dist.get_backend() == "nccl"
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("K,P,chunks", [(37, 1_000_003, 8), (100, 3_125_000, 4), (5, 4_099, 3)])
def test_rccl_allgather_world1_bit_exact(rccl_group, K, P, chunks):
    red = ShardedReducer(K, P, chunks=chunks, device=DEV, gather=True)
    assert red.gather and red.full is not None
    synthetic.fill_rows(red.clients, red.plan.local_segments())
    weights = mfl_amd.sample_weights(synthetic.sample_counts(K))
    w = mfl_amd.weights_tensor(weights, torch.float32, DEV)
    red.full.fill_(float("nan"))
    full = red.step(w)
    torch.cuda.synchronize()
    assert full.data_ptr() == red.full.data_ptr() and full.numel() == P
    exp = O.reduce_f32(synthetic.client_columns_numpy(K, 0, P), weights)
    _bits(full.cpu().numpy(), exp, "reassembled model vs oracle")
    # the exchange step alone rebuilds the same model from local_out
    red.full.zero_()
    red.gather_only()
    torch.cuda.synchronize()
    _bits(red.full[:P].cpu().numpy(), exp, "gather_only")
    # back-to-back steps (the bench's timed loop) stay correct
    for _ in range(3):
        red.step(w)
    torch.cuda.synchronize()
    _bits(red.full[:P].cpu().numpy(), exp, "repeated steps")


def test_cfg5_full_size_single_gpu_passes():
    """cfg5 at its full N = 1 size (1000 x 100M fp32 = 400 GB of rows, more than
    one GPU holds) as the bench runs it: two P-chunked passes over one resident
    1000 x 50M buffer (200 GB), every pass's sampled windows bit-exact vs the
    oracle on host-regenerated inputs (bench.sampled_parity).  Run as a child
    process so that this process's cached allocations do not count against the
    200 GB (fedavg_trainer.py:441-458 at BASELINE.json configs[4])."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    if torch.cuda.get_device_properties(0).total_memory < 240 * 2**30:
        pytest.skip("needs a GPU with >= 240 GiB of HBM")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--workload", "synthetic_1000x100m", "--steps", "1",
                        "--warmup", "0", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=110,
                       env=dict(os.environ), cwd=str(root))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["config"]["passes"] == 2 and line["config"]["P_per_gpu"] == 100_000_000, line["config"]
    assert line["parity"]["ok"], line["parity"]
    assert line["parity"]["columns_checked"] >= 2 * 3 * 2048


def test_bench_plain_run_dumps_the_timed_model(tmp_path):
    """A plain ``bench.py`` run (cfg2: 10 x 1,206,590, the whole model fits the
    dump) carries none of the ``--full`` side measurements, times exactly
    ``--steps`` steps, and ``--dump-outputs`` writes the averaged model of the
    last timed step: float32, bit for bit the oracle's on host-regenerated
    inputs."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--workload", "femnist_cnn",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True,
                       text=True, timeout=110, env=dict(os.environ), cwd=str(root))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    K, P = 10, 1_206_590
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32" and line["unit"] == "GB/s"
    # value and ms_per_step are one measurement (ms_per_step is rounded to 1e-4 ms, value to 0.01 GB/s)
    assert line["value"] == pytest.approx((4 * K * P + 4 * P + 4 * K) / line["ms_per_step"] / 1e6,
                                          rel=1e-3 + 0.5e-4 / line["ms_per_step"], abs=0.006)
    for key in ("cpu_baseline", "parity", "round_with_distances", "clock_mhz"):
        assert key not in line, key
    got = np.load(tmp_path / "model.npy")
    assert got.dtype == np.float32 and got.shape == (P,)
    w = mfl_amd.sample_weights(synthetic.sample_counts(K))
    _bits(got, O.reduce_f32(synthetic.client_columns_numpy(K, 0, P), w), "bench.py --dump-outputs model")
