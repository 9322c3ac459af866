"""The fused client statistics on the MI355X: fedavg_client_stats_f32 /
fedavg_client_track against the numpy fp64 oracle (tests/client_stats_oracle.py)
and, through ClientStepStats and client_train, against what the reference's
own Client.train recorded (tests/golden/client)."""
import math

import numpy as np
import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import _lib, client_stats

pytestmark = pytest.mark.gpu

# numels from {1, 3, 4, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5}: unit edges (4,096) and 16-B tails
SHAPES = {
    "k1_one": [1],
    "k1_units": [3 * 4096 + 5],
    "k3": [4097, 1, 63],
    "k7": [4096, 3, 65, 4095, 64, 4, 3 * 4096 + 5],
    "k7_rev": [3 * 4096 + 5, 4, 64, 4095, 65, 3, 4096],
}
# any fp64 summation order of P non-negative terms is within P * 2^-53 (< 3e-12 here) of the exact sum
SUM_RTOL = 1e-11
PAD = 123.0  # sentinel in the snapshot's padding: the pass must leave it alone


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    return _lib.load()


def _data(numels, seed):
    """Model-like weights N(0, 0.05^2) and the same one 1e-3 step later."""
    rng = np.random.default_rng(seed)
    prev = [rng.normal(0.0, 0.05, n).astype(np.float32) for n in numels]
    cur = [(p + 1e-3 * rng.normal(0.0, 1.0, p.size)).astype(np.float32) for p in prev]
    return prev, cur


def _to_dev(arr, dev, misaligned=False):
    """A device tensor of arr; misaligned: a view at storage offset 1 (4-B, not 16-B aligned)."""
    if not misaligned:
        t = torch.from_numpy(arr.copy()).to(dev)
        assert t.data_ptr() % 16 == 0
        return t
    base = torch.zeros(arr.size + 1, dtype=torch.float32, device=dev)
    view = base[1:]
    view.copy_(torch.from_numpy(arr.copy()))
    assert view.data_ptr() % 16 == 4
    return view


class Pass:
    """One fedavg_client_stats_f32 call over a list of device tensors."""

    def __init__(self, lib, dev, numels):
        self.lib, self.dev = lib, dev
        self.numel = np.array(numels, dtype=np.int64)
        padded = (self.numel + 3) // 4 * 4
        self.offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self.P = int(padded.sum())
        n = len(numels)
        self.nparts = int(lib.fedavg_client_stats_partials(self.numel.ctypes.data, n))
        self.ws = int(lib.fedavg_client_stats_workspace(n))
        self.host_ws = torch.empty(max(self.ws, 16), dtype=torch.uint8, pin_memory=True)
        self.dev_ws = torch.empty(max(self.ws, 16), dtype=torch.uint8, device=dev)
        self.partials = torch.empty(max(self.nparts, 1), dtype=torch.float64, device=dev)
        self.snap = torch.full((self.P,), PAD, dtype=torch.float32, device=dev)

    def set_snap(self, arrays):
        host = np.full(self.P, PAD, dtype=np.float32)
        for a, off in zip(arrays, self.offset):
            host[off:off + a.size] = a
        self.snap.copy_(torch.from_numpy(host))

    def snap_bits(self):
        return self.snap.cpu().numpy().view(np.int32)

    def expected_bits(self, arrays):
        host = np.full(self.P, PAD, dtype=np.float32)
        for a, off in zip(arrays, self.offset):
            host[off:off + a.size] = a
        return host.view(np.int32)

    def run(self, tensors, has_snap):
        ptrs = np.array([t.data_ptr() for t in tensors], dtype=np.int64)
        stats = torch.full((4,), -7.0, dtype=torch.float64, device=self.dev)
        rc = self.lib.fedavg_client_stats_f32(
            ptrs.ctypes.data, self.numel.ctypes.data, self.offset.ctypes.data, len(tensors), self.snap.data_ptr(),
            self.P, has_snap, self.partials.data_ptr(), self.partials.numel(), stats.data_ptr(),
            self.host_ws.data_ptr(), self.dev_ws.data_ptr(), self.host_ws.numel(),
            torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "fedavg_client_stats_f32", self.lib)
        torch.cuda.synchronize()
        return stats.cpu().numpy()


def _oracle(prev, cur, has_snap):
    c = np.concatenate(cur)
    return O.record(c, np.concatenate(prev) if has_snap else None)


def _close(got, want):
    return got == want or abs(got - want) <= SUM_RTOL * abs(want)


@pytest.mark.parametrize("has_snap", [0, 1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_record_and_snapshot(lib, dev, shape, has_snap):
    numels = SHAPES[shape]
    prev, cur = _data(numels, seed=len(numels) * 100 + has_snap)
    p = Pass(lib, dev, numels)
    p.set_snap(prev)
    tensors = [_to_dev(a, dev) for a in cur]
    stats = p.run(tensors, has_snap)
    nan_count, s_cur, s_d = _oracle(prev, cur, has_snap)
    print(f"{shape} has_snap={has_snap}: got {stats.tolist()} want {(nan_count, s_cur, s_d)}")
    assert stats[0] == nan_count == 0 and stats[3] == 0.0
    assert _close(stats[1], s_cur)
    assert _close(stats[2], s_d) and (has_snap or stats[2] == 0.0)
    assert np.array_equal(p.snap_bits(), p.expected_bits(cur))  # snap = cur bit for bit, padding untouched
    # determinism: the same call again, from the same snapshot
    p.set_snap(prev)
    again = p.run(tensors, has_snap)
    assert again.tobytes() == stats.tobytes()


@pytest.mark.parametrize("which", [0, 1, 2, "all"])
@pytest.mark.parametrize("shape", ["k3", "k7"])
def test_misaligned_key_takes_the_scalar_path_with_the_same_result(lib, dev, shape, which):
    numels = SHAPES[shape]
    prev, cur = _data(numels, seed=7)
    p = Pass(lib, dev, numels)
    p.set_snap(prev)
    aligned = p.run([_to_dev(a, dev) for a in cur], 1)
    p.set_snap(prev)
    tensors = [_to_dev(a, dev, misaligned=(which == "all" or j == which)) for j, a in enumerate(cur)]
    got = p.run(tensors, 1)
    assert got.tobytes() == aligned.tobytes()
    assert np.array_equal(p.snap_bits(), p.expected_bits(cur))


@pytest.mark.parametrize("misaligned", [False, True])
def test_nan_count_is_exact_and_snapshot_keeps_nan_bits(lib, dev, misaligned):
    numels = SHAPES["k7"]
    prev, cur = _data(numels, seed=11)
    cur[0][0] = np.nan                     # the first element
    cur[3][-1] = np.nan                    # the last element of a key (4,095: a 3-element tail)
    cur[2][64] = np.nan                    # inside a scalar tail (65 = 16 slices + 1)
    cur[6][3 * 4096 + 2] = np.float32(np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0])  # a payload
    cur[1][1] = np.nan                     # a key shorter than one slice
    p = Pass(lib, dev, numels)
    p.set_snap(prev)
    stats = p.run([_to_dev(a, dev, misaligned) for a in cur], 1)
    assert stats[0] == 5.0
    assert math.isnan(stats[1]) and math.isnan(stats[2])
    assert np.array_equal(p.snap_bits(), p.expected_bits(cur))


def test_inf_is_not_a_nan_and_gives_an_infinite_sum(lib, dev):
    numels = SHAPES["k3"]
    prev, cur = _data(numels, seed=13)
    cur[0][5] = np.inf
    cur[2][62] = -np.inf
    p = Pass(lib, dev, numels)
    p.set_snap(prev)
    stats = p.run([_to_dev(a, dev) for a in cur], 1)
    assert stats[0] == 0.0 and stats[1] == math.inf and stats[2] == math.inf
    assert np.array_equal(p.snap_bits(), p.expected_bits(cur))


def test_zero_difference_and_empty_models(lib, dev):
    numels = SHAPES["k7"]
    prev, cur = _data(numels, seed=17)
    p = Pass(lib, dev, numels)
    p.set_snap(cur)
    stats = p.run([_to_dev(a, dev) for a in cur], 1)
    assert stats[2] == 0.0 and _close(stats[1], O.record(np.concatenate(cur))[1])
    # P == 0: a no-op that writes zero stats
    stats_t = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    rc = lib.fedavg_client_stats_f32(None, None, None, 0, None, 0, 1, None, 0, stats_t.data_ptr(), None, None, 0,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert stats_t.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    # keys without elements: the same
    e = Pass(lib, dev, [0, 0])
    e.snap = torch.full((4,), PAD, dtype=torch.float32, device=dev)
    e.P = 4
    assert e.run([torch.empty(0, device=dev), torch.empty(0, device=dev)], 1).tolist() == [0.0] * 4
    assert e.snap.cpu().tolist() == [PAD] * 4


def test_track_update_rule_on_device(lib, dev):
    """fedavg_client_track against the oracle's rule: a first zero is replaced,
    NaN after a set value is ignored, NaN first (or after a zero) is sticky."""
    sequences = {
        "zero_then_smaller": [(1.0, 0.0, 0.0), (2.0, 0.5, 0.25)],
        "max_stays": [(1.0, 2.0, 2.0), (3.0, 0.5, 0.25), (0.7, 1.1, 0.3)],
        "nan_after_set": [(1.0, 2.0, 3.0), (1.0, float("nan"), float("nan")), (1.0, 1.0, 1.0)],
        "nan_first": [(1.0, float("nan"), float("nan")), (1.0, 5.0, 5.0)],
        "nan_after_zero": [(1.0, 0.0, 0.0), (1.0, float("nan"), float("nan")), (1.0, 5.0, 5.0)],
        "zero_step": [(0.0, 1.0, 1.0)],  # norm(w - last_w) == 0: inf
    }
    for name, seq in sequences.items():
        state = torch.zeros(4, dtype=torch.float64, device=dev)
        track = O.Track()
        for n_w, n_g, dl in seq:
            sw, sg = float(n_w) ** 2 * 1.37, float(n_g) ** 2 * 0.91
            w = torch.tensor([0.0, 1.0, sw, 0.0], dtype=torch.float64, device=dev)
            g = torch.tensor([0.0, 1.0, sg, 0.0], dtype=torch.float64, device=dev)
            rc = lib.fedavg_client_track(state.data_ptr(), w.data_ptr(), g.data_ptr(), dl,
                                         torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "fedavg_client_track", lib)
            torch.cuda.synchronize()
            track.step(sw, sg, dl)
        rho, beta, has_rho, has_beta = state.cpu().tolist()
        assert has_rho == 1.0 and has_beta == 1.0
        for got, want in ((rho, float(track.rho)), (beta, float(track.beta))):
            assert (math.isnan(got) and math.isnan(want)) or got == want, (name, got, want)


def _cuda_model(case, dev):
    net = O.build_model(case["meta"]["model"]).to(dev)
    return net, list(net.parameters())


def _set(params, flat, grads):
    off = 0
    with torch.no_grad():
        for p in params:
            n = p.numel()
            t = torch.from_numpy(np.array(flat[off:off + n])).view_as(p).to(p.device)
            if grads:
                p.grad = t.contiguous()  # a new tensor every step, as backward after zero_grad() leaves it
            else:
                p.copy_(t)
            off += n


@pytest.mark.parametrize("name", O.client_case_names())
def test_tracking_on_recorded_sequences(dev, name):
    """The reference's recorded (w_t, g_t, loss_t) fed into parameter and grad
    tensors: guard decisions, rho and beta."""
    case = O.load_client_case(name)
    meta, w, g, loss = case["meta"], case["w"], case["g"], case["loss"]
    net, params = _cuda_model(case, dev)
    _set(params, w[0], False)
    _set(params, g[0], True)
    stats = mfl_amd.ClientStepStats(params, stats="hip")
    assert stats.mode == "hip"
    stats.begin(float(loss[0]))
    tripped_at = None
    for t in range(1, len(g)):
        _set(params, g[t], True)
        trip = stats.after_backward(torch.tensor(loss[t], device=dev), meta["lr"], meta["ratio"])
        if not math.isnan(float(loss[t])):
            assert stats.loss == float(loss[t])
        if trip:
            tripped_at = t - 1
            break
        _set(params, w[t], False)
        stats.after_step(float(loss[t]), float(loss[t - 1]))
    syncs = stats.host_syncs
    beta, rho = stats.result()
    assert syncs == (len(g) - 1) and stats.host_syncs == syncs + 1  # one per iteration, one for the result
    o_trip, o_beta, o_rho = O.replay(w, g, loss, meta["lr"], meta["ratio"])
    assert tripped_at == o_trip
    assert (tripped_at is not None) == meta["tripped"]
    if meta["tripped"]:
        assert beta is None and rho is None
        return
    print(f"{name}: beta {beta!r} oracle {o_beta!r} ref {case['ret'][1]!r}; rho {rho!r} oracle {o_rho!r} "
          f"ref {case['ret'][2]!r}")
    # three fp32 roundings of 2^-24 each on exactly rounded norms
    assert O.rel(beta, o_beta) <= 1e-6 and O.rel(rho, o_rho) <= 1e-6
    bound = O.ref_bound(meta)
    assert O.rel(beta, float(case["ret"][1])) <= bound and O.rel(rho, float(case["ret"][2])) <= bound


def _train(case, dev, stats, keep_on_device=False):
    client, net = O.case_client(case, dev)
    seen = []
    out = client_stats.client_train(client, net, case["meta"]["local_iteration"], stats=stats,
                                    keep_on_device=keep_on_device,
                                    trace=lambda stage, w, g, loss: seen.append((stage, w.cpu().numpy(),
                                                                                 None if g is None else g.cpu().numpy(),
                                                                                 loss)))
    return out, seen


def test_client_train_end_to_end(dev):
    """client_train on the GPU on the small MLP: rho and beta equal the oracle
    applied to the tensors the run itself produced (independent of how forward
    and backward round); hip and torch statistics take the same guard decisions."""
    case = O.load_client_case("mlp_16x24x4_it4")
    meta = case["meta"]
    (sd, loss, beta, rho, acc, cycles), seen = _train(case, dev, "hip")
    assert loss is not None and all(v.device.type == "cpu" for v in sd.values())
    w = [s[1] for s in seen if s[0] in ("begin", "after_step")]
    g = [s[2] for s in seen if s[0] in ("begin", "after_backward")]
    losses = [s[3] for s in seen if s[0] in ("begin", "after_backward")]
    assert len(w) == len(g) == meta["local_iteration"] + 1
    o_trip, o_beta, o_rho = O.replay(w, g, np.array(losses, dtype=np.float32), meta["lr"], meta["ratio"])
    assert o_trip is None
    print(f"end to end: beta {beta!r} oracle {o_beta!r}; rho {rho!r} oracle {o_rho!r}")
    assert O.rel(beta, o_beta) <= 1e-6 and O.rel(rho, o_rho) <= 1e-6
    assert 0.0 <= acc <= 1.0 and cycles > 0
    (_, t_loss, t_beta, t_rho, _, _), _ = _train(case, dev, "torch")
    assert t_loss is not None and t_beta is not None and t_rho is not None
    for name in ("nan_input_trips", "tiny_weights_trip"):
        trips = O.load_client_case(name)
        for mode in ("hip", "torch"):
            out, seen = _train(trips, dev, mode)
            assert out[1:] == (None,) * 5, (name, mode)
            assert [s[0] for s in seen] == ["begin", "after_backward"]


def test_keep_on_device_feeds_the_device_round(dev):
    case = O.load_client_case("mlp_16x24x4_it4")
    w_locals = []
    for n in (8, 24):
        (sd, loss, beta, rho, acc, cycles), _ = _train(case, dev, "hip", keep_on_device=True)
        assert all(v.is_cuda for v in sd.values())
        w_locals.append((n, sd))
    out = mfl_amd.aggregate(w_locals, device=dev)
    for k, v in out.items():
        assert v.is_cuda and bool(torch.isfinite(v).all()), k


def _reuse_run(dev, w0, grads, fresh, optimizer, guard):
    """Three iterations on a two-key model of 5 and 3 elements; ``fresh``: every
    p.grad is a new tensor each time (the old ones kept alive, so the addresses
    differ), else the values are copied into fixed grad tensors.  Returns the
    weights, the record and, in the fresh run, the waits the reuse rule made."""
    flat = torch.cat(w0)
    params = [torch.nn.Parameter(flat[:5]), torch.nn.Parameter(flat[5:])]
    assert params[1].data_ptr() % 16 == 4  # not 16-B aligned
    kw = dict(optimizer="adam", adam=dict(lr=0.01, weight_decay=0.001)) if optimizer == "adam" else {}
    t = mfl_amd.ClientStepStats(params, stats="hip", step="fused", guard=guard, ahead=1 if guard == "device" else None,
                                **kw)
    assert (t.step_mode, t.guard_mode, t._offset.tolist()) == ("fused", guard, [0, 8])  # the second offset is padded
    kept, waits = [], []

    def give(gs):
        for p, g in zip(params, gs):
            if fresh or p.grad is None:
                kept.append(p.grad)
                p.grad = g.clone()
            else:
                p.grad.copy_(g)
        waits.append(t._passes["g"].stage(t._grad_ptrs().tobytes()))  # the pass below ships this very table
        waits.append(t._passes["g"].stage(t._grad_ptrs().tobytes()))  # and the same addresses again never wait

    losses = [torch.tensor(v, device=dev) for v in (2.5, 2.25, 1.75, 1.5)]
    give(grads[0])
    if guard == "device":
        t.begin(losses[0])
        for i in range(3):
            give(grads[i + 1])
            t.guarded_step(losses[i + 1], 0.05, 1000.0)
        assert t.finish()[0] is None
    else:
        t.begin(2.5)
        last = 2.5
        for i in range(3):
            give(grads[i + 1])
            assert not t.after_backward(losses[i + 1], 0.05, 1000.0)
            t.adam_step(t.loss, last) if optimizer == "adam" else t.sgd_step(0.05, t.loss, last)
            last = t.loss
        t.result()
    state = t._step.state.clone() if optimizer == "adam" else torch.zeros(0, device=dev)
    return [x.view(torch.int64 if x.dtype == torch.float64 else torch.int32).cpu()
            for x in (flat.detach(), t._rec, state)], waits


@pytest.mark.parametrize("optimizer,guard", [("sgd", "host"), ("adam", "host"), ("sgd", "device"), ("adam", "device")])
def test_key_table_reuse_rule_and_fresh_grads_equal_fixed_grads(dev, optimizer, guard):
    """The pinned key table's reuse rule (_KeyPass.stage): no wait before the
    first call nor for the same addresses, one wait when every grad is a new
    tensor, none when those addresses come again; and the weights, the record
    and Adam's state after three iterations are the same bits whether the
    gradients arrive in new tensors or in fixed ones."""
    rng = np.random.default_rng(53)
    w0, *grads = [[torch.from_numpy(rng.normal(0.0, scale, n).astype(np.float32)).to(dev) for n in (5, 3)]
                  for scale in (0.3, 1.0, 1.0, 1.0, 1.0)]
    moved, waits = _reuse_run(dev, w0, grads, True, optimizer, guard)
    assert waits == [False, False] + [True, False] * 3
    fixed, waits = _reuse_run(dev, w0, grads, False, optimizer, guard)
    assert waits == [False] * 8
    for a, b, what in zip(moved, fixed, ("weights", "record", "adam state")):
        assert torch.equal(a, b), what
    assert not torch.equal(moved[0], torch.cat(w0).view(torch.int32).cpu())  # the steps were taken
