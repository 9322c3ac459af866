"""The fused client SGD step on the MI355X: fedavg_client_sgd_step_{f32,bf16,
f16,f64} (include/fedavg_amd_clientstep.h) against torch.optim.SGD on the same
GPU, bit for bit, its record against numpy fp64 sums of the downloaded
tensors, and, through ClientStepStats and client_train with step="fused", on
the recorded client cases of tests/golden/client."""
import math

import numpy as np
import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import _lib, client_stats

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
# the fused-step dtype tuple: a dtype sgd_form found no form for is not in it
KEYS = [k for k, dt in DTYPES.items() if dt in client_stats.STEP_DTYPES]
UNIT = {"f32": 4096, "bf16": 8192, "f16": 8192, "f64": 2048}  # elements of 16 KiB
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
LRS = (0.03, 0.001)
# any fp64 summation order of P non-negative terms is within P * 2^-53 (< 3e-12 here) of the exact sum
SUM_RTOL = 1e-11
SENTINEL = 123.0  # exact in every dtype
PAD = 8           # sentinel elements on either side of a weight tensor


def shapes(key):
    U = UNIT[key]
    k7 = [U, 3, 65, U - 1, 64, 4, 3 * U + 5]
    return {"k1_one": [1], "k1_units": [3 * U + 5], "k3": [U + 1, 1, 63], "k7": k7, "k7_rev": k7[::-1]}


SHAPE_NAMES = sorted(shapes("f32"))


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    return _lib.load_clientstep()


@pytest.fixture(scope="module")
def forms(dev):
    """The form of each dtype, found once."""
    return {k: client_stats.sgd_form(dev, DTYPES[k]) for k in KEYS}


_data_cache = {}


def _data(numels, seed, dt):
    """test_gpu_client_stats._data's recipe: model-like weights N(0, 0.05^2);
    gradients N(0, 1).  CPU tensors of type T, computed once per case."""
    key = (tuple(numels), seed, dt)
    if key not in _data_cache:
        rng = np.random.default_rng(seed)
        w = [torch.from_numpy(rng.normal(0.0, 0.05, n)).to(dt) for n in numels]
        g = [torch.from_numpy(rng.normal(0.0, 1.0, n)).to(dt) for n in numels]
        _data_cache[key] = (w, g)
    return _data_cache[key]


def _bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def _grad_dev(t, dev, offset=0):
    """A device copy of t at a storage offset of `offset` elements of a 16-B aligned allocation."""
    base = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    view = base[offset:]
    view.copy_(t)
    assert base.data_ptr() % 16 == 0 and (view.data_ptr() - base.data_ptr()) == offset * t.element_size()
    return view


class Weights:
    """Weight tensors as views inside one buffer each, PAD sentinel elements
    before and after (and `offset` more in front: a storage offset that takes
    the tensor off its 16-B alignment)."""

    def __init__(self, tensors, dev, offset=0):
        self.bufs, self.views, self.lead = [], [], PAD + offset  # PAD elements are a multiple of 16 B in every dtype
        for t in tensors:
            buf = torch.full((self.lead + t.numel() + PAD,), SENTINEL, dtype=t.dtype, device=dev)
            assert buf.data_ptr() % 16 == 0
            view = buf[self.lead:self.lead + t.numel()]
            view.copy_(t)
            assert view.data_ptr() % 16 == (offset * t.element_size()) % 16
            self.bufs.append(buf)
            self.views.append(view)

    def sentinels_untouched(self):
        for buf, view in zip(self.bufs, self.views):
            host = buf.cpu()
            edge = torch.cat([host[:self.lead], host[self.lead + view.numel():]])
            if not bool((edge == SENTINEL).all()) or edge.numel() != self.lead + PAD:
                return False
        return True


class Step:
    """One fedavg_client_sgd_step_* call over lists of device tensors."""

    def __init__(self, lib, dev, numels, key):
        self.lib, self.key, self.dt = lib, key, DTYPES[key]
        self.fn = getattr(lib, f"fedavg_client_sgd_step_{key}")
        es = torch.empty(0, dtype=self.dt).element_size()
        self.numel = np.array(numels, dtype=np.int64)
        n = len(numels)
        self.nparts = int(lib.fedavg_client_step_partials(self.numel.ctypes.data, n, es))
        ws = int(lib.fedavg_client_step_workspace(n))
        self.host_ws = torch.empty(max(ws, 16), dtype=torch.uint8, pin_memory=True)
        self.dev_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=dev)
        self.partials = torch.empty(max(self.nparts, 1), dtype=torch.float64, device=dev)
        self.stats = torch.full((4,), -7.0, dtype=torch.float64, device=dev)

    def run(self, w, g, lr, form):
        self.stats.fill_(-7.0)
        w_ptrs = np.array([t.data_ptr() for t in w], dtype=np.int64)
        g_ptrs = np.array([t.data_ptr() for t in g], dtype=np.int64)
        rc = self.fn(w_ptrs.ctypes.data, g_ptrs.ctypes.data, self.numel.ctypes.data, len(self.numel), lr, form,
                     self.partials.data_ptr(), self.partials.numel(), self.stats.data_ptr(), self.host_ws.data_ptr(),
                     self.dev_ws.data_ptr(), self.host_ws.numel(), torch.cuda.current_stream().cuda_stream)
        _lib.check_clientstep(rc, f"fedavg_client_sgd_step_{self.key}")
        torch.cuda.synchronize()
        return self.stats.cpu().numpy()


def _torch_sgd(w, g, lr, dev):
    """What torch.optim.SGD(params, lr=lr).step() leaves on clones on the same GPU."""
    params = [torch.nn.Parameter(t.clone().to(dev)) for t in w]
    for p, t in zip(params, g):
        p.grad = t.clone().to(dev)
    torch.optim.SGD(params, lr=lr).step()
    torch.cuda.synchronize()
    return [p.detach() for p in params]


def _sums(w_new, w_old):
    """numpy fp64 sums from the downloaded w' and rT(w' - w) (the difference formed by torch in the model's type)."""
    if not w_new:
        return 0.0, 0.0
    new, old = torch.cat([t.reshape(-1) for t in w_new]).cpu(), torch.cat([t.reshape(-1) for t in w_old]).cpu()
    d = (new - old).double().numpy()
    n = new.double().numpy()
    with np.errstate(all="ignore"):
        return float(np.sum(n * n)), float(np.sum(d * d))


def _close(got, want):
    return got == want or abs(got - want) <= SUM_RTOL * abs(want)


# ------------------------------------------------------------------- the form
@pytest.mark.parametrize("key", KEYS)
def test_sgd_form_finds_a_form(dev, key):
    found = client_stats.sgd_form_probe(dev, DTYPES[key])
    print(f"sgd_form {key}: {found}")
    assert found["differ"] > 0, "the two forms gave the same bits on the probe: it cannot tell them apart"
    assert found["form"] in (0, 1) and found["match"][found["form"]] and not found["match"][1 - found["form"]]
    assert client_stats.sgd_form(dev, DTYPES[key]) == found["form"]
    assert client_stats.sgd_form_probe(dev, DTYPES[key]) is found  # cached: one probe per (device, dtype)


def test_fp32_is_a_fused_step_dtype():
    assert "f32" in KEYS


# ------------------------------------------------- bits, record, determinism
@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("key", KEYS)
def test_bits_equal_torch_and_the_record(lib, dev, forms, key, shape, lr):
    numels = shapes(key)[shape]
    w, g = _data(numels, len(numels) * 100 + int(lr * 1000), DTYPES[key])
    want = _torch_sgd(w, g, lr, dev)
    step = Step(lib, dev, numels, key)
    ws = Weights(w, dev)
    gs = [_grad_dev(t, dev) for t in g]
    stats = step.run(ws.views, gs, lr, forms[key])
    for j, (got, ref) in enumerate(zip(ws.views, want)):
        assert torch.equal(_bits(got), _bits(ref)), j
    for j, (got, ref) in enumerate(zip(gs, g)):
        assert torch.equal(_bits(got.cpu()), _bits(ref)), j  # g unchanged
    assert ws.sentinels_untouched()
    s_w, s_d = _sums(ws.views, [t.to(dev) for t in w])
    print(f"{key} {shape} lr={lr}: got {stats.tolist()} want {(0, s_w, s_d, 0)}")
    assert stats[0] == 0.0 and stats[3] == 0.0
    assert _close(stats[1], s_w) and _close(stats[2], s_d)
    # the same call again from the same start: the same bytes; then with partials full of NaN
    for dirty in (False, True):
        again = Weights(w, dev)
        if dirty:
            step.partials.fill_(math.nan)
            step.dev_ws.fill_(0xFF)
        assert step.run(again.views, gs, lr, forms[key]).tobytes() == stats.tobytes(), dirty
        for got, ref in zip(again.views, want):
            assert torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("shape", ["k3", "k7"])
@pytest.mark.parametrize("key", KEYS)
def test_misaligned_sides_give_the_aligned_bytes(lib, dev, forms, key, shape):
    """w, g or both at a storage offset of one element: the same w' bits and the same stats bytes."""
    numels = shapes(key)[shape]
    lr = LRS[0]
    w, g = _data(numels, 7, DTYPES[key])
    step = Step(lib, dev, numels, key)
    base = Weights(w, dev)
    aligned = step.run(base.views, [_grad_dev(t, dev) for t in g], lr, forms[key])
    for w_off, g_off in ((1, 0), (0, 1), (1, 1)):
        ws = Weights(w, dev, w_off)
        gs = [_grad_dev(t, dev, g_off) for t in g]
        got = step.run(ws.views, gs, lr, forms[key])
        assert got.tobytes() == aligned.tobytes(), (w_off, g_off)
        for a, b in zip(ws.views, base.views):
            assert torch.equal(_bits(a), _bits(b)), (w_off, g_off)
        for a, b in zip(gs, g):
            assert torch.equal(_bits(a.cpu()), _bits(b)), (w_off, g_off)
        assert ws.sentinels_untouched(), (w_off, g_off)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("key", KEYS)
def test_special_values(lib, dev, forms, key, offset):
    """NaN and +-inf in g, subnormal w and g, -0.0, and |g| large enough to
    overflow fp16, in one [U + 1] key (the last element is a ragged slice)."""
    dt, U = DTYPES[key], UNIT[key]
    n = U + 1
    w, g = _data([n], 41, dt)
    w, g = w[0].clone(), g[0].clone()
    tiny = torch.finfo(dt).smallest_normal
    g[0], g[1], g[2], g[n - 1] = math.nan, math.inf, -math.inf, math.nan
    w[3], g[3] = tiny / 4, 0.0            # subnormal w kept
    w[4], g[4] = tiny / 4, tiny / 2       # subnormal w and g
    w[5], g[5] = 0.0, tiny / 8            # a subnormal (or vanishing) product alone
    w[6], g[6] = -0.0, 0.0                # -0.0 + (-lr * 0.0)
    w[7], g[7] = -0.0, -0.0
    w[8], g[8] = 1.0, 6.0e4               # finite in fp16, w' is not past lr 0.03; the next ones are
    w[9], g[9] = 6.0e4, -6.0e4
    w[10], g[10] = -6.0e4, 6.5e4
    w[n - 2], g[n - 2] = tiny / 2, -tiny  # in the last whole slice
    for lr in (0.03, 40.0):
        want = _torch_sgd([w], [g], lr, dev)[0]
        ws = Weights([w], dev, offset)
        gs = [_grad_dev(g, dev, offset)]
        stats = Step(lib, dev, [n], key).run(ws.views, gs, lr, forms[key])
        got = ws.views[0]
        nan_w, nan_g = torch.isnan(want), torch.isnan(got)
        assert stats[0] == float(nan_w.sum()) and float(nan_w.sum()) >= 2
        assert torch.equal(nan_w, nan_g)  # NaN positions; payload bits are not compared
        assert torch.equal(_bits(got)[~nan_g], _bits(want)[~nan_w])
        assert ws.sentinels_untouched()
        assert math.isnan(stats[1]) and math.isnan(stats[2]) and stats[3] == 0.0
        if key == "f16" and lr == 40.0:
            assert bool(torch.isinf(want[8:11]).any())  # the step overflowed fp16 in torch as well


@pytest.mark.parametrize("key", KEYS)
def test_empty_keys_and_an_empty_model(lib, dev, forms, key):
    dt = DTYPES[key]
    fn = getattr(lib, f"fedavg_client_sgd_step_{key}")
    # no keys at all: every table may be null
    stats_t = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    rc = fn(None, None, None, 0, 0.03, forms[key], None, 0, stats_t.data_ptr(), None, None, 0,
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert stats_t.cpu().tolist() == [0.0] * 4
    # keys without elements
    step = Step(lib, dev, [0, 0], key)
    empty = torch.empty(0, dtype=dt, device=dev)
    assert step.run([empty, empty], [empty, empty], 0.03, forms[key]).tolist() == [0.0] * 4
    # empty keys among others change nothing, and their (dangling) addresses are never used
    numels = [0, UNIT[key] + 1, 0, 5, 0]
    w, g = _data(numels, 43, dt)
    want = _torch_sgd(w, g, 0.03, dev)
    ws = Weights(w, dev)
    stats = Step(lib, dev, numels, key).run(ws.views, [_grad_dev(t, dev) for t in g], 0.03, forms[key])
    for got, ref in zip(ws.views, want):
        assert torch.equal(_bits(got), _bits(ref))
    assert ws.sentinels_untouched() and stats[0] == 0.0
    dense = Weights([w[1], w[3]], dev)
    assert Step(lib, dev, [numels[1], numels[3]], key).run(
        dense.views, [_grad_dev(g[1], dev), _grad_dev(g[3], dev)], 0.03, forms[key]).tobytes() == stats.tobytes()


# ------------------------------------------------------------- ClientStepStats
def test_no_mixing_of_after_step_and_sgd_step(dev):
    p = torch.nn.Parameter(torch.full((16,), 0.5, device=dev))
    p.grad = torch.ones(16, device=dev)
    fused = mfl_amd.ClientStepStats([p], step="fused")
    assert fused.step_mode == "fused" and mfl_amd.ClientStepStats([p], step="auto").step_mode == "fused"
    fused.begin(1.0)
    with pytest.raises(RuntimeError, match="after_step.*fused stepping"):
        fused.after_step(0.5, 1.0)
    plain = mfl_amd.ClientStepStats([p])
    assert plain.step_mode == "torch"
    plain.begin(1.0)
    with pytest.raises(RuntimeError, match="sgd_step.*step='fused'"):
        plain.sgd_step(0.03, 0.5, 1.0)
    version = p._version
    assert not fused.after_backward(torch.tensor(0.5, device=dev), 0.25, 1e9)
    fused.sgd_step(0.25, 0.5, 1.0)
    assert p._version > version and torch.equal(p.detach().cpu(), torch.full((16,), 0.25))


def _client(case, dev, dt):
    client, net = O.case_client(case, dev)
    if dt != torch.float32:
        x, labels = client.local_training_data[0]
        client.local_training_data = [(x.to(dt), labels)]
        net = net.to(dt)
    return client, net


def _train(case, dev, dt, **kw):
    client, net = _client(case, dev, dt)
    seen = []
    out = client_stats.client_train(client, net, case["meta"]["local_iteration"], stats="hip",
                                    trace=lambda stage, w, g, loss: seen.append((stage, w, g, loss)), **kw)
    return out, seen


def test_client_train_with_fused_stepping(dev):
    """mlp_16x24x4_it4 with step="fused": every traced w after the step is
    torch SGD applied on the GPU to the traced w before and the traced g; rho
    and beta are the oracle's on the traced tensors; one sync per iteration
    and one for the result; the tripping cases never step."""
    case = O.load_client_case("mlp_16x24x4_it4")
    meta = case["meta"]
    syncs = []
    real = client_stats.ClientStepStats.result

    def counting(self):
        syncs.append(self.host_syncs)
        out = real(self)
        syncs.append(self.host_syncs)
        return out

    client_stats.ClientStepStats.result = counting
    try:
        (sd, loss, beta, rho, acc, cycles), seen = _train(case, dev, torch.float32, step="fused")
    finally:
        client_stats.ClientStepStats.result = real
    assert syncs == [meta["local_iteration"], meta["local_iteration"] + 1]
    assert loss is not None and all(v.device.type == "cpu" for v in sd.values())
    w = [s[1] for s in seen if s[0] in ("begin", "after_step")]
    g = [s[2] for s in seen if s[0] in ("begin", "after_backward")]
    losses = [s[3] for s in seen if s[0] in ("begin", "after_backward")]
    assert len(w) == len(g) == meta["local_iteration"] + 1
    for t in range(1, len(w)):
        want = _torch_sgd([w[t - 1]], [g[t]], meta["lr"], dev)[0]
        assert torch.equal(_bits(w[t]), _bits(want)), t
    o_trip, o_beta, o_rho = O.replay([t.cpu().numpy() for t in w], [t.cpu().numpy() for t in g],
                                     np.array(losses, dtype=np.float32), meta["lr"], meta["ratio"])
    assert o_trip is None
    print(f"fused stepping: beta {beta!r} oracle {o_beta!r}; rho {rho!r} oracle {o_rho!r}")
    assert O.rel(beta, o_beta) <= 1e-6 and O.rel(rho, o_rho) <= 1e-6
    assert 0.0 <= acc <= 1.0 and cycles > 0
    for name in ("nan_input_trips", "tiny_weights_trip"):
        trips = O.load_client_case(name)
        out, seen = _train(trips, dev, torch.float32, step="fused")
        assert out[1:] == (None,) * 5, name
        assert [s[0] for s in seen] == ["begin", "after_backward"]  # never stepped


@pytest.mark.parametrize("key", [k for k in KEYS if k != "f32"])
def test_client_train_with_fused_stepping_other_dtypes(dev, key):
    """The same run in bf16, fp16 and fp64: the traced steps are torch's bits."""
    dt = DTYPES[key]
    case = O.load_client_case("mlp_16x24x4_it4")
    meta = case["meta"]
    (sd, loss, beta, rho, acc, cycles), seen = _train(case, dev, dt, step="fused")
    assert loss is not None and beta is not None and rho is not None
    w = [s[1] for s in seen if s[0] in ("begin", "after_step")]
    g = [s[2] for s in seen if s[0] in ("begin", "after_backward")]
    assert len(w) == len(g) == meta["local_iteration"] + 1 and all(t.dtype == dt for t in w + g)
    for t in range(1, len(w)):
        want = _torch_sgd([w[t - 1]], [g[t]], meta["lr"], dev)[0]
        assert torch.equal(_bits(w[t]), _bits(want)), t


def test_keep_on_device_with_fused_stepping_feeds_the_device_round(dev):
    case = O.load_client_case("mlp_16x24x4_it4")
    w_locals = []
    for n in (8, 24):
        (sd, loss, beta, rho, acc, cycles), _ = _train(case, dev, torch.float32, step="fused", keep_on_device=True)
        assert loss is not None and all(v.is_cuda for v in sd.values())
        w_locals.append((n, sd))
    out = mfl_amd.aggregate(w_locals, device=dev)
    for k, v in out.items():
        assert v.is_cuda and bool(torch.isfinite(v).all()), k
