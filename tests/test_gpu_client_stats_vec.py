"""The fused client statistics for bf16, fp16 and fp64 models on the MI355X:
fedavg_client_stats_{bf16,f16,f64} / fedavg_client_track_{bf16,f16,f64}
(include/fedavg_amd_clientvec.h) against the dtype oracle
(tests/client_stats_vec_oracle.py) and, through ClientStepStats and
client_train, on the recorded sequences of tests/golden/client cast to each
dtype."""
import math
import types

import numpy as np
import pytest
import torch

import client_stats_oracle as O
import client_stats_vec_oracle as V
import mfl_amd
from mfl_amd import _lib, client_stats

pytestmark = pytest.mark.gpu

KEYS = sorted(V.DTYPES)
ES = {"bf16": 2, "f16": 2, "f64": 8}
BITS = {2: torch.int16, 8: torch.int64}
# key sizes at the unit edge (16 KiB: 8,192 / 2,048 elements) and the 16-B tails (8 / 2 elements)
SHAPES = {
    2: {"k1_one": [1], "k1_units": [3 * 8192 + 5], "k3": [8193, 1, 127],
        "k7": [8192, 7, 129, 8191, 8, 9, 3 * 8192 + 5], "k7_rev": [3 * 8192 + 5, 9, 8, 8191, 129, 7, 8192]},
    8: {"k1_one": [1], "k1_units": [3 * 2048 + 1], "k3": [2049, 2, 31],
        "k7": [2048, 1, 33, 2047, 3, 31, 3 * 2048 + 1], "k7_rev": [3 * 2048 + 1, 31, 3, 2047, 33, 1, 2048]},
}
SHAPE_NAMES = sorted(SHAPES[2])
# any fp64 summation order of P <= 25k non-negative terms is within P * 2^-53 (< 3e-12) of the exact sum; for fp64
# inputs each rounded square adds 2^-53
SUM_RTOL = 1e-11
PAD = 123.0  # sentinel in the snapshot's padding (exact in every dtype): the pass must leave it alone
# payload NaNs per dtype
PAYLOAD = {"bf16": 0x7FC5, "f16": 0x7E05, "f64": 0x7FF8000000012345}


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    return _lib.load_clientvec()


def _data(numels, seed, dt):
    """Model-like weights N(0, 0.05^2) and the same one 1e-3 step later, as CPU tensors of type T."""
    rng = np.random.default_rng(seed)
    prev64 = [rng.normal(0.0, 0.05, n) for n in numels]
    cur64 = [p + 1e-3 * rng.normal(0.0, 1.0, p.size) for p in prev64]
    return [torch.from_numpy(a).to(dt) for a in prev64], [torch.from_numpy(a).to(dt) for a in cur64]


def _to_dev(t, dev, offset=0):
    """A device tensor of t; offset > 0: a view at that storage offset of a 16-B aligned allocation."""
    if not offset:
        d = t.clone().to(dev)
        assert d.data_ptr() % 16 == 0
        return d
    base = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    view = base[offset:]
    view.copy_(t)
    assert view.data_ptr() % 16 == (offset * t.element_size()) % 16 != 0
    return view


class Pass:
    """One fedavg_client_stats_{bf16,f16,f64} call over a list of device tensors."""

    def __init__(self, lib, dev, numels, key):
        self.lib, self.dev, self.key, self.dt, self.es = lib, dev, key, V.DTYPES[key], ES[key]
        self.fn = getattr(lib, f"fedavg_client_stats_{key}")
        per16 = 16 // self.es
        self.numel = np.array(numels, dtype=np.int64)
        padded = (self.numel + per16 - 1) // per16 * per16
        self.offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self.P = int(padded.sum())
        n = len(numels)
        self.nparts = int(lib.fedavg_client_stats_vec_partials(self.numel.ctypes.data, n, self.es))
        self.ws = int(lib.fedavg_client_stats_vec_workspace(n))
        self.host_ws = torch.empty(max(self.ws, 16), dtype=torch.uint8, pin_memory=True)
        self.dev_ws = torch.empty(max(self.ws, 16), dtype=torch.uint8, device=dev)
        self.partials = torch.empty(max(self.nparts, 1), dtype=torch.float64, device=dev)
        self.snap = torch.full((max(self.P, per16),), PAD, dtype=self.dt, device=dev)
        self.stats = torch.full((4,), -7.0, dtype=torch.float64, device=dev)

    def _flat(self, tensors):
        host = torch.full((self.snap.numel(),), PAD, dtype=self.dt)
        for a, off in zip(tensors, self.offset):
            host[off:off + a.numel()] = a
        return host

    def set_snap(self, tensors):
        self.snap.copy_(self._flat(tensors))

    def snap_bits(self):
        return self.snap.cpu().view(BITS[self.es])

    def expected_bits(self, tensors):
        return self._flat(tensors).view(BITS[self.es])

    def launch(self, tensors, has_snap, stream=None):
        ptrs = np.array([t.data_ptr() for t in tensors], dtype=np.int64)
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = self.fn(ptrs.ctypes.data, self.numel.ctypes.data, self.offset.ctypes.data, len(tensors),
                     self.snap.data_ptr(), self.P, has_snap, self.partials.data_ptr(), self.partials.numel(),
                     self.stats.data_ptr(), self.host_ws.data_ptr(), self.dev_ws.data_ptr(), self.host_ws.numel(), st)
        _lib.check_clientvec(rc, f"fedavg_client_stats_{self.key}")

    def run(self, tensors, has_snap):
        self.stats.fill_(-7.0)
        self.launch(tensors, has_snap)
        torch.cuda.synchronize()
        return self.stats.cpu().numpy()


def _oracle(prev, cur, has_snap):
    return V.record(torch.cat(cur), torch.cat(prev) if has_snap else None)


def _close(got, want):
    return got == want or abs(got - want) <= SUM_RTOL * abs(want)


# ------------------------------------------------------------ record, snapshot
@pytest.mark.parametrize("has_snap", [0, 1])
@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("key", KEYS)
def test_record_and_snapshot(lib, dev, key, shape, has_snap):
    numels = SHAPES[ES[key]][shape]
    prev, cur = _data(numels, len(numels) * 100 + has_snap, V.DTYPES[key])
    p = Pass(lib, dev, numels, key)
    p.set_snap(prev)
    tensors = [_to_dev(a, dev) for a in cur]
    stats = p.run(tensors, has_snap)
    nan_count, s_cur, s_d = _oracle(prev, cur, has_snap)
    print(f"{key} {shape} has_snap={has_snap}: got {stats.tolist()} want {(nan_count, s_cur, s_d)}")
    assert stats[0] == nan_count == 0 and stats[3] == 0.0
    assert _close(stats[1], s_cur)
    assert _close(stats[2], s_d) and (has_snap or stats[2] == 0.0)
    assert torch.equal(p.snap_bits(), p.expected_bits(cur))  # snap = cur bit for bit, padding untouched
    # determinism: the same call again, from the same snapshot
    p.set_snap(prev)
    again = p.run(tensors, has_snap)
    assert again.tobytes() == stats.tobytes()


@pytest.mark.parametrize("shape", ["k3", "k7"])
@pytest.mark.parametrize("key,offset", [(k, o) for k in KEYS for o in ((1, 4) if ES[k] == 2 else (1,))])
def test_misaligned_tensors_give_the_aligned_bytes(lib, dev, key, shape, offset):
    """Storage offset 1 (2 B / 8 B off) and, for the 16-bit types, 4 (8-B but
    not 16-B aligned): one key at a time and all keys."""
    numels = SHAPES[ES[key]][shape]
    prev, cur = _data(numels, 7, V.DTYPES[key])
    p = Pass(lib, dev, numels, key)
    p.set_snap(prev)
    aligned = p.run([_to_dev(a, dev) for a in cur], 1)
    assert torch.equal(p.snap_bits(), p.expected_bits(cur))
    for which in [*range(len(numels)), "all"]:
        p.set_snap(prev)
        tensors = [_to_dev(a, dev, offset if which in ("all", j) else 0) for j, a in enumerate(cur)]
        got = p.run(tensors, 1)
        assert got.tobytes() == aligned.tobytes(), which
        assert torch.equal(p.snap_bits(), p.expected_bits(cur)), which


def _set_bits(t, idx, bits):
    assert 0 <= bits < 1 << (8 * t.element_size() - 1)  # a positive NaN: the same value as a signed integer
    t.view(BITS[t.element_size()])[idx] = bits


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("key", KEYS)
def test_nan_count_is_exact_and_snapshot_keeps_nan_bits(lib, dev, key, offset):
    es = ES[key]
    numels = SHAPES[es]["k7"]
    prev, cur = _data(numels, 11, V.DTYPES[key])
    cur[0][0] = math.nan                      # the first element
    cur[3][-1] = math.nan                     # the last element of a key with a tail (8,191 / 2,047)
    cur[2][numels[2] - 1] = math.nan          # inside a scalar tail (129 / 33 = 16 slices + 1)
    _set_bits(cur[6], numels[6] - 1, PAYLOAD[key])  # a payload NaN
    cur[1][numels[1] - 1] = math.nan          # a key shorter than one slice (7 / 1 elements)
    assert numels[1] < 16 // es and int(torch.isnan(torch.cat(cur)).sum()) == 5
    p = Pass(lib, dev, numels, key)
    p.set_snap(prev)
    stats = p.run([_to_dev(a, dev, offset) for a in cur], 1)
    assert stats[0] == 5.0
    assert math.isnan(stats[1]) and math.isnan(stats[2])
    assert torch.equal(p.snap_bits(), p.expected_bits(cur))
    assert int(p.snap_bits()[int(p.offset[6]) + numels[6] - 1]) & ((1 << (8 * es)) - 1) == PAYLOAD[key]


@pytest.mark.parametrize("key", KEYS)
def test_inf_is_not_a_nan_and_gives_an_infinite_sum(lib, dev, key):
    numels = SHAPES[ES[key]]["k3"]
    prev, cur = _data(numels, 13, V.DTYPES[key])
    cur[0][5] = math.inf
    cur[2][numels[2] - 1] = -math.inf
    p = Pass(lib, dev, numels, key)
    p.set_snap(prev)
    stats = p.run([_to_dev(a, dev) for a in cur], 1)
    assert stats[0] == 0.0 and stats[1] == math.inf and stats[2] == math.inf
    assert torch.equal(p.snap_bits(), p.expected_bits(cur))


@pytest.mark.parametrize("key", KEYS)
def test_zero_difference_and_empty_models(lib, dev, key):
    dt, es = V.DTYPES[key], ES[key]
    numels = SHAPES[es]["k7"]
    prev, cur = _data(numels, 17, dt)
    p = Pass(lib, dev, numels, key)
    p.set_snap(cur)
    stats = p.run([_to_dev(a, dev) for a in cur], 1)
    assert stats[2] == 0.0 and _close(stats[1], V.record(torch.cat(cur))[1])
    # P == 0: a no-op that writes zero stats
    stats_t = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    rc = p.fn(None, None, None, 0, None, 0, 1, None, 0, stats_t.data_ptr(), None, None, 0,
              torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert stats_t.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    # keys without elements: the same, and the snapshot is left alone
    e = Pass(lib, dev, [0, 0], key)
    e.P = e.snap.numel()
    empty = torch.empty(0, dtype=dt, device=dev)
    assert e.run([empty, empty], 1).tolist() == [0.0] * 4
    assert e.snap.cpu().tolist() == [PAD] * e.snap.numel()


# --------------------------------------------------------------------- tracker
TRACK_SEQUENCES = {
    "zero_then_smaller": [(1.0, 0.0, 0.0), (2.0, 0.5, 0.25)],
    "max_stays": [(1.0, 2.0, 2.0), (3.0, 0.5, 0.25), (0.7, 1.1, 0.3)],
    "nan_after_set": [(1.0, 2.0, 3.0), (1.0, float("nan"), float("nan")), (1.0, 1.0, 1.0)],
    "nan_first": [(1.0, float("nan"), float("nan")), (1.0, 5.0, 5.0)],
    "nan_after_zero": [(1.0, 0.0, 0.0), (1.0, float("nan"), float("nan")), (1.0, 5.0, 5.0)],
    "zero_step": [(0.0, 1.0, 1.0)],  # norm(w - last_w) == 0: inf
}


@pytest.mark.parametrize("key", KEYS)
def test_track_update_rule_on_device(lib, dev, key):
    """The six sequences of the fp32 tracker test through each dtype's entry,
    bit-equal to the oracle's Track fed the same sums."""
    fn = getattr(lib, f"fedavg_client_track_{key}")
    for name, seq in TRACK_SEQUENCES.items():
        state = torch.zeros(4, dtype=torch.float64, device=dev)
        track = V.Track(V.DTYPES[key])
        for n_w, n_g, dl in seq:
            sw, sg = float(n_w) ** 2 * 1.37, float(n_g) ** 2 * 0.91
            w = torch.tensor([0.0, 1.0, sw, 0.0], dtype=torch.float64, device=dev)
            g = torch.tensor([0.0, 1.0, sg, 0.0], dtype=torch.float64, device=dev)
            rc = fn(state.data_ptr(), w.data_ptr(), g.data_ptr(), dl, torch.cuda.current_stream().cuda_stream)
            _lib.check_clientvec(rc, f"fedavg_client_track_{key}")
            torch.cuda.synchronize()
            track.step(sw, sg, dl)
        rho, beta, has_rho, has_beta = state.cpu().tolist()
        assert has_rho == 1.0 and has_beta == 1.0
        assert V.same(rho, track.rho) and V.same(beta, track.beta), (name, rho, track.rho, beta, track.beta)


# ------------------------------------------------------------- ClientStepStats
def _set(params, flat, grads):
    off = 0
    with torch.no_grad():
        for p in params:
            n = p.numel()
            t = flat[off:off + n].view_as(p).to(p.device)
            if grads:
                p.grad = t.contiguous()  # a new tensor every step, as backward after zero_grad() leaves it
            else:
                p.copy_(t)
            off += n


_replays = {}


def _replay(name, key):
    if (name, key) not in _replays:
        dt = V.DTYPES[key]
        case = O.load_client_case(name)
        w, g = V.cast_sequence(case, dt)
        _replays[(name, key)] = (case, w, g, V.replay(w, g, case["loss"], case["meta"]["lr"], case["meta"]["ratio"],
                                                      dt))
    return _replays[(name, key)]


@pytest.mark.parametrize("name", O.client_case_names())
@pytest.mark.parametrize("key", KEYS)
def test_tracking_on_recorded_sequences(dev, key, name):
    """The reference's recorded (w_t, g_t, loss_t), cast to the dtype, fed into
    parameter and grad tensors: mode, guard decisions, host syncs, and rho /
    beta bit-equal to the oracle's Track fed the device's own records."""
    dt = V.DTYPES[key]
    case, w, g, (o_trip, o_beta, o_rho) = _replay(name, key)
    meta, loss = case["meta"], case["loss"]
    net = O.build_model(meta["model"]).to(dt).to(dev)
    params = list(net.parameters())
    _set(params, w[0], False)
    _set(params, g[0], True)
    stats = mfl_amd.ClientStepStats(params, stats="hip")
    assert stats.mode == "hip" and mfl_amd.ClientStepStats(params).mode == "hip"
    stats.begin(float(loss[0]))
    track = V.Track(dt)
    tripped_at = None
    for t in range(1, len(g)):
        _set(params, g[t], True)
        trip = stats.after_backward(torch.tensor(float(loss[t]), device=dev), meta["lr"], meta["ratio"])
        if not math.isnan(float(loss[t])):
            assert stats.loss == float(loss[t])
        if trip:
            tripped_at = t - 1
            break
        _set(params, w[t], False)
        stats.after_step(float(loss[t]), float(loss[t - 1]))
        rec = stats._rec.cpu().numpy()  # the test's own read: not one of the class's syncs
        track.step(float(rec[client_stats._W + 2]), float(rec[client_stats._G + 2]),
                   abs(float(loss[t]) - float(loss[t - 1])))
    syncs = stats.host_syncs
    beta, rho = stats.result()
    assert syncs == (len(g) - 1) and stats.host_syncs == syncs + 1  # one per iteration, one for the result
    assert tripped_at == o_trip
    assert (tripped_at is not None) == meta["tripped"]
    if meta["tripped"]:
        assert beta is None and rho is None
        return
    print(f"{name} {key}: beta {beta!r} track {track.beta!r} oracle {o_beta!r}; rho {rho!r} track {track.rho!r} "
          f"oracle {o_rho!r}")
    assert V.same(beta, track.beta) and V.same(rho, track.rho)


def _client(case, dev, dt):
    """case_client with the model and x cast to the dtype."""
    meta = case["meta"]
    args = types.SimpleNamespace(client_optimizer="sgd", lr=meta["lr"], wd=0.0, clip=meta["clip"], dataset="mnist")
    x = torch.from_numpy(np.array(case["x"])).to(dt)
    labels = torch.from_numpy(np.array(case["labels"]))
    client = O.make_client_class(meta["ratio"])((x, labels), args, dev)
    net = O.load_flat(O.build_model(meta["model"]), case["w"][0]).to(dt).to(dev)
    return client, net


def _train(case, dev, dt, stats, keep_on_device=False):
    client, net = _client(case, dev, dt)
    seen = []
    out = client_stats.client_train(client, net, case["meta"]["local_iteration"], stats=stats,
                                    keep_on_device=keep_on_device,
                                    trace=lambda stage, w, g, loss: seen.append((stage, w.cpu(),
                                                                                 None if g is None else g.cpu(),
                                                                                 loss)))
    return out, seen


@pytest.mark.parametrize("key", KEYS)
def test_client_train_end_to_end(dev, key):
    """client_train on the small MLP in each dtype: rho and beta equal the
    oracle applied to the tensors the run itself produced (fp64: to within the
    bound of the sums' order, see below); the torch statistics
    on the same GPU take the same guard decisions (their rho / beta are
    printed next to the fused ones: agreement reported, not asserted); with
    keep_on_device the result feeds the device round."""
    dt = V.DTYPES[key]
    case = O.load_client_case("mlp_16x24x4_it4")
    meta = case["meta"]
    (sd, loss, beta, rho, acc, cycles), seen = _train(case, dev, dt, "auto")
    assert loss is not None and all(v.device.type == "cpu" and v.dtype == dt for v in sd.values())
    w = [s[1] for s in seen if s[0] in ("begin", "after_step")]
    g = [s[2] for s in seen if s[0] in ("begin", "after_backward")]
    losses = [s[3] for s in seen if s[0] in ("begin", "after_backward")]
    assert len(w) == len(g) == meta["local_iteration"] + 1 and all(t.dtype == dt for t in w + g)
    o_trip, o_beta, o_rho = V.replay(w, g, losses, meta["lr"], meta["ratio"], dt)
    assert o_trip is None
    (_, t_loss, t_beta, t_rho, _, _), t_seen = _train(case, dev, dt, "torch")
    print(f"end to end {key}: beta fused {beta!r} oracle {o_beta!r} torch {t_beta!r}; rho fused {rho!r} "
          f"oracle {o_rho!r} torch {t_rho!r}")
    if dt == torch.float64:
        # fp64 has no coarser type to round the sums' last bits away: the device's fixed-order sums and the oracle's
        # exact ones differ by at most P * 2^-53 relative (P addends >= 0), a norm by half of that plus its own
        # rounding, the quotient (or reciprocal and product) of two norms by P * 2^-53 + 3 * 2^-53
        tol = (w[0].numel() + 3) * 2.0 ** -53
        assert O.rel(beta, o_beta) <= tol and O.rel(rho, o_rho) <= tol, (beta, o_beta, rho, o_rho, tol)
    else:
        assert V.same(beta, o_beta) and V.same(rho, o_rho)
    assert 0.0 <= acc <= 1.0 and cycles > 0
    assert t_loss is not None and [s[0] for s in t_seen] == [s[0] for s in seen]  # the same guard decisions
    w_locals = []
    for n in (8, 24):
        (sd, loss, _, _, _, _), _ = _train(case, dev, dt, "hip", keep_on_device=True)
        assert loss is not None and all(v.is_cuda for v in sd.values())
        w_locals.append((n, sd))
    out = mfl_amd.aggregate(w_locals, device=dev)
    for k, v in out.items():
        assert v.is_cuda and bool(torch.isfinite(v).all()), k


def test_grads_of_another_dtype_raise(dev):
    p = torch.nn.Parameter(torch.zeros(16, dtype=torch.bfloat16, device=dev))
    p.grad = torch.zeros(16, dtype=torch.bfloat16, device=dev)
    stats = mfl_amd.ClientStepStats([p], stats="hip")
    p.grad_dtype = None  # torch itself refuses a grad of another dtype unless the tensor allows any
    p.grad = torch.zeros(16, dtype=torch.float32, device=dev)
    with pytest.raises(TypeError, match="dtype"):
        stats.begin(0.0)
    mixed = [p, torch.nn.Parameter(torch.zeros(16, dtype=torch.float16, device=dev))]
    assert mfl_amd.ClientStepStats(mixed).mode == "torch"
    with pytest.raises(TypeError, match="one dtype"):
        mfl_amd.ClientStepStats(mixed, stats="hip")


# ------------------------------------------------------------- contract checks
@pytest.fixture(scope="module")
def sides(dev):
    return [torch.cuda.Stream(device=dev) for _ in range(2)]


@pytest.fixture(scope="module")
def hold_cycles(dev):
    """About 5 ms of torch.cuda._sleep: far longer than a call sequence's host time."""
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(1_000_000)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0
    return int(5.0 * 1_000_000 / ms)


def _reference_run(lib, dev, key, seed=23):
    numels = SHAPES[ES[key]]["k7"]
    prev, cur = _data(numels, seed, V.DTYPES[key])
    p = Pass(lib, dev, numels, key)
    p.set_snap(prev)
    stats = p.run([_to_dev(a, dev) for a in cur], 1)
    return numels, prev, cur, stats, p.snap_bits().clone()


@pytest.mark.parametrize("key", KEYS)
def test_dirty_workspaces_change_nothing(lib, dev, key):
    numels, prev, cur, want, want_snap = _reference_run(lib, dev, key)
    p = Pass(lib, dev, numels, key)
    p.set_snap(prev)
    p.dev_ws.fill_(0xFF)
    p.partials.view(torch.uint8).fill_(0xFF)  # NaN bytes
    tensors = [_to_dev(a, dev) for a in cur]
    p.stats.view(torch.uint8).fill_(0xFF)
    p.launch(tensors, 1)
    torch.cuda.synchronize()
    assert p.stats.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(p.snap_bits(), want_snap)


def _ordered(p, stream, hold, staged, tensors, prev_dev, result, poison):
    """Behind a hold on `stream`: the real snapshot and tensors in, the call, the record out, poison."""
    with torch.cuda.stream(stream):
        if hold:
            torch.cuda._sleep(hold)
        p.snap.copy_(prev_dev, non_blocking=True)
        for t, s in zip(tensors, staged):
            t.copy_(s, non_blocking=True)
        p.launch(tensors, 1, stream.cuda_stream)
        busy = not stream.query()
        result.copy_(p.stats, non_blocking=True)
        for t in tensors:
            t.copy_(poison[:t.numel()], non_blocking=True)
    return busy


def _stream_case(lib, dev, key, seed):
    numels, prev, cur, want, want_snap = _reference_run(lib, dev, key, seed)
    p = Pass(lib, dev, numels, key)
    staged = [_to_dev(a, dev) for a in cur]
    nan = torch.full((max(numels),), math.nan, dtype=V.DTYPES[key], device=dev)
    tensors = [nan[:n].clone() for n in numels]  # the call must not read these before the stream brings the values
    p.snap.fill_(math.nan)
    prev_dev = p._flat(prev).to(dev)
    result = torch.zeros(4, dtype=torch.float64, device=dev)
    return p, staged, tensors, prev_dev, result, nan, want, want_snap


@pytest.mark.parametrize("key", KEYS)
def test_stats_call_is_ordered_on_its_stream(lib, dev, key, sides, hold_cycles):
    p, staged, tensors, prev_dev, result, nan, want, want_snap = _stream_case(lib, dev, key, 29)
    torch.cuda.synchronize()
    busy = _ordered(p, sides[0], hold_cycles, staged, tensors, prev_dev, result, nan)
    assert busy, "the stream was idle when the call returned: the hold was too short to prove anything"
    sides[0].synchronize()
    assert result.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(p.snap_bits(), want_snap)
    torch.cuda.synchronize()


@pytest.mark.parametrize("key", KEYS)
def test_two_streams_with_separate_buffers(lib, dev, key, sides, hold_cycles):
    cases = [_stream_case(lib, dev, key, seed) for seed in (31, 37)]
    torch.cuda.synchronize()
    for (p, staged, tensors, prev_dev, result, nan, _, _), s in zip(cases, sides):
        _ordered(p, s, hold_cycles // 5, staged, tensors, prev_dev, result, nan)
    for s in sides:
        s.synchronize()
    for p, _, _, _, result, _, want, want_snap in cases:
        assert result.cpu().numpy().tobytes() == want.tobytes()
        assert torch.equal(p.snap_bits(), want_snap)
    torch.cuda.synchronize()


@pytest.mark.parametrize("key", KEYS)
def test_track_call_is_ordered_and_reentrant_across_streams(lib, dev, key, sides, hold_cycles):
    fn = getattr(lib, f"fedavg_client_track_{key}")
    draws = [(3.7, 1.9, 0.41), (0.8, 2.6, 1.3)]
    want = []
    for sw, sg, dl in draws:
        track = V.Track(V.DTYPES[key])
        track.step(sw, sg, dl)
        want.append((track.rho, track.beta))
    bufs = []
    for (sw, sg, dl), s in zip(draws, sides):
        real = torch.tensor([0.0, 1.0, sw, 0.0, 0.0, 1.0, sg, 0.0], dtype=torch.float64, device=dev)
        recs = torch.full((8,), math.nan, dtype=torch.float64, device=dev)
        state = torch.zeros(4, dtype=torch.float64, device=dev)
        out = torch.zeros(4, dtype=torch.float64, device=dev)
        bufs.append((real, recs, state, out))
    nan8 = torch.full((8,), math.nan, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    busy = []
    for (sw, sg, dl), s, (real, recs, state, out) in zip(draws, sides, bufs):
        with torch.cuda.stream(s):
            torch.cuda._sleep(hold_cycles)
            recs.copy_(real, non_blocking=True)
            rc = fn(state.data_ptr(), recs.data_ptr(), recs.data_ptr() + 32, dl, s.cuda_stream)
            _lib.check_clientvec(rc, f"fedavg_client_track_{key}")
            busy.append(not s.query())
            out.copy_(state, non_blocking=True)
            recs.copy_(nan8, non_blocking=True)
    assert all(busy), "a stream was idle when the call returned: the hold was too short to prove anything"
    for s in sides:
        s.synchronize()
    for (rho_w, beta_w), (_, _, _, out) in zip(want, bufs):
        rho, beta, has_rho, has_beta = out.cpu().tolist()
        assert has_rho == 1.0 and has_beta == 1.0 and V.same(rho, rho_w) and V.same(beta, beta_w)
    torch.cuda.synchronize()
