"""libfedavg_amd_clientloop.so on the MI355X through its C ABI.

The guard kernel on crafted records, per dtype: the answers are those of the
host expressions ClientStepStats.after_backward evaluates (client_stats.
_norm_of / _guard_bound and its fp32 branch), evaluated here, at the edge
(norm == bound, and the least sum whose norm rounds above the bound), on NaN
and inf sums, a NaN count, a NaN loss and an all-zero model; and the gate is
sticky.

The gated SGD and Adam steps on the smallest key lists that reach the tails
(one element; 4097, 0 and 63 elements; tensors not 16-B aligned): with an
open gate every stored bit equals the ungated entry's and rho / beta equal
fedavg_client_track* fed |loss - last_loss| from the host; with a set gate
nothing that was pre-filled with a dirty pattern changes."""
import math

import numpy as np
import pytest
import torch

from mfl_amd import _lib, client_stats

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
KEYS = tuple(DTYPES)
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
INF, NAN = math.inf, math.nan
# the record, laid out as client_stats lays it out
W, G, STATE, LOSS, LAST, GATE, EPOCH, REC = 0, 4, 8, 12, 13, 14, 15, 16


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ the guard
def host_norm(key, s):
    if key == "f32":  # after_backward's fp32 branch
        return np.float32(math.sqrt(s)) if not math.isnan(s) else np.float32("nan")
    return client_stats._norm_of(float(s), DTYPES[key])


def host_bound(key, n_w, lr_ratio):
    if key == "f32":
        with np.errstate(all="ignore"):
            return np.float32(lr_ratio) * n_w
    return client_stats._guard_bound(n_w, lr_ratio, DTYPES[key])


def host_trip(key, nans, s_g, s_w, loss, lr_ratio):
    n_g, n_w = host_norm(key, s_g), host_norm(key, s_w)
    return bool(nans > 0 or math.isnan(loss) or n_g > host_bound(key, n_w, lr_ratio))


def device_guard(dev, key, nans, s_g, s_w, loss, lr_ratio, epoch, gate=(0.0, 0.0)):
    lib = _lib.load_clientloop()
    rec = torch.tensor([nans, s_g, 0, 0, 0, s_w, 0, 0, loss, 0, gate[0], gate[1]], dtype=torch.float64, device=dev)
    p = rec.data_ptr()
    name = f"fedavg_client_guard_{key}"
    rc = getattr(lib, name)(p, p + 32, p + 64, p + 80, lr_ratio, epoch, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check_clientloop(rc, name)
    out = rec.cpu()
    assert same(out[:10], torch.tensor([nans, s_g, 0, 0, 0, s_w, 0, 0, loss, 0], dtype=torch.float64))  # read only
    return float(out[10]), float(out[11])


def edge_sums(key, s_w, lr_ratio):
    """(a sum whose norm equals the bound, the greatest such sum, the least sum whose norm is above the bound)."""
    bound = float(host_bound(key, host_norm(key, s_w), lr_ratio))
    dt = DTYPES[key]
    above = float((bits(torch.tensor([bound], dtype=dt)) + 1).view(dt))  # the next value of the type (bound > 0)
    equal = bound * bound
    assert float(host_norm(key, equal)) == bound and float(host_norm(key, above * above)) > bound
    # the norm is monotone in the sum: bisect over the doubles between the two, by their bit patterns
    as_int = lambda x: int(np.float64(x).view(np.int64))  # noqa: E731
    as_float = lambda i: float(np.int64(i).view(np.float64))  # noqa: E731
    lo, hi = as_int(equal), as_int(above * above)  # norm(lo) <= bound < norm(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if float(host_norm(key, as_float(mid))) > bound:
            hi = mid
        else:
            lo = mid
    return equal, as_float(lo), as_float(hi)


@pytest.mark.parametrize("key", KEYS)
def test_guard_decides_as_the_host_expressions_do(dev, key):
    s_w, lr_ratio = 2.7182818, 0.001 * 37.0
    equal, last_equal, first_above = edge_sums(key, s_w, lr_ratio)
    assert not host_trip(key, 0, equal, s_w, 1.0, lr_ratio) and not host_trip(key, 0, last_equal, s_w, 1.0, lr_ratio)
    assert host_trip(key, 0, first_above, s_w, 1.0, lr_ratio)
    cases = [
        (0, equal, s_w, 1.0), (0, last_equal, s_w, 1.0), (0, first_above, s_w, 1.0),
        (1, 1e-12, s_w, 1.0),      # one NaN among the gradients, small sums
        (0, 1e-12, s_w, NAN),      # a NaN loss
        (0, NAN, s_w, 1.0),        # a NaN norm compares false
        (0, 1e-12, NAN, 1.0),
        (0, 1.0, NAN, 1.0),
        (0, INF, s_w, 1.0),
        (0, INF, INF, 1.0),        # inf > inf is false
        (0, 0.0, 0.0, 1.0),        # 0 > 0 is false
        (0, 1e-300, 0.0, 1.0),     # a norm that may round to 0 in the type
        (0, 1e-12, s_w, 1.0),      # a clean record
    ]
    seen = []
    for epoch, (nans, s_g, s_w_, loss) in enumerate(cases, start=2):
        want = host_trip(key, nans, s_g, s_w_, loss, lr_ratio)
        gate, at = device_guard(dev, key, nans, s_g, s_w_, loss, lr_ratio, epoch)
        print(f"{key}: nans {nans} S_g {s_g!r} S_w {s_w_!r} loss {loss!r}: host {want} device gate {gate} epoch {at}")
        assert (gate, at) == ((1.0, float(epoch)) if want else (0.0, 0.0)), (nans, s_g, s_w_, loss)
        seen.append(want)
    assert seen[:7] == [False, False, True, True, True, False, False] and seen[8] and not seen[-1]


@pytest.mark.parametrize("key", KEYS)
def test_a_set_gate_stays_set_and_keeps_its_first_epoch(dev, key):
    s_w, lr_ratio = 4.0, 0.05
    tripping, clean = (1, 1e-12, s_w, 1.0), (0, 1e-12, s_w, 1.0)
    assert device_guard(dev, key, *tripping, lr_ratio, 5) == (1.0, 5.0)
    assert device_guard(dev, key, *clean, lr_ratio, 6, gate=(1.0, 5.0)) == (1.0, 5.0)     # not cleared
    assert device_guard(dev, key, *tripping, lr_ratio, 7, gate=(1.0, 5.0)) == (1.0, 5.0)  # the first epoch stays
    assert device_guard(dev, key, *clean, lr_ratio, 0) == (0.0, 0.0)
    assert device_guard(dev, key, *tripping, lr_ratio, 0) == (1.0, 0.0)                    # epoch 0 is an epoch


# ------------------------------------------------------------------ the gated steps
# name -> (key sizes in elements, offset of w and of g from a 16-B boundary in elements)
LISTS = {"one": ([1], 0, 0), "three": ([4097, 0, 63], 0, 0), "unaligned": ([37, 5, 4100], 1, 3)}
PAD = 16
LR = 0.03
ADAM = dict(lr=0.3, beta1=0.6, beta2=0.7, eps=1e-8, wd=0.3)
DIRTY = 7.25


class Side:
    """The keys of one side in one device buffer, sentinels between them."""

    def __init__(self, numel, off, values, dt, dev):
        per = 16 // torch.empty(0, dtype=dt).element_size()
        self.start, cursor = [], 0
        for n in numel:
            s = -(-(cursor + PAD) // per) * per + off
            self.start.append(s)
            cursor = s + n
        self.host = torch.full((cursor + PAD,), 123.0, dtype=dt)
        at = 0
        for s, n in zip(self.start, numel):
            self.host[s:s + n] = values[at:at + n]
            at += n
        self.numel = numel
        self.buf = self.host.to(dev)
        es = self.buf.element_size()
        self.ptrs = np.array([self.buf.data_ptr() + s * es for s in self.start], dtype=np.int64)

    def fresh(self):
        self.buf.copy_(self.host)


class Launch:
    """One key list with its buffers: the ungated entry and the gated one write into the same places in turn."""

    def __init__(self, name, key, dev, adam):
        numel, w_off, g_off = LISTS[name]
        self.key, self.dev, self.adam, self.dt = key, dev, adam, DTYPES[key]
        total = sum(numel)
        rng = np.random.default_rng(sum(map(ord, name + key)))
        self.w = Side(numel, w_off, torch.from_numpy(rng.normal(0.0, 0.05 if not adam else 1.0, total)).to(self.dt),
                      self.dt, dev)
        self.g = [Side(numel, g_off, torch.from_numpy(rng.normal(0.0, 1.0, total)).to(self.dt), self.dt, dev)
                  for _ in range(2)]
        self.numel = np.array(numel, dtype=np.int64)
        es = self.w.buf.element_size()
        per = 16 // es
        padded = (self.numel + per - 1) // per * per
        self.offset = (np.cumsum(padded) - padded).astype(np.int64)
        self.state_elems = int(max(padded.sum(), per))
        loop = _lib.load_clientloop()
        n = len(numel)
        ws = int(loop.fedavg_client_loop_workspace(n, 1 if adam else 0))
        nparts = int(loop.fedavg_client_loop_partials(self.numel.ctypes.data, n, es))
        self.partials = torch.full((max(nparts, 1),), DIRTY, dtype=torch.float64, device=dev)
        self.host_ws = torch.empty(max(ws, 16), dtype=torch.uint8, pin_memory=True)
        self.dev_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=dev)
        self.planes = torch.zeros(3 * self.state_elems, dtype=self.dt, device=dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def step(self, t, form, rec, gated):
        """Step t (0 or 1) of the chain; the record goes to rec[W:W + 4]."""
        base = rec.data_ptr()
        more = (base + 8 * G, base + 8 * GATE, base + 8 * STATE, base + 8 * LOSS) if gated else ()
        tail = (self.partials.data_ptr(), self.partials.numel(), base + 8 * W, self.host_ws.data_ptr(),
                self.dev_ws.data_ptr(), self.host_ws.numel(), self.stream)
        n = len(self.numel)
        if self.adam:
            coef = client_stats.adam_coef(ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], ADAM["wd"], t + 1)
            lib, check = (_lib.load_clientloop(), _lib.check_clientloop) if gated else \
                (_lib.load_clientadam(), _lib.check_clientadam)
            name = f"fedavg_client_adam_step_{'gated_' if gated else ''}{self.key}"
            rc = getattr(lib, name)(self.w.ptrs.ctypes.data, self.g[t].ptrs.ctypes.data, self.numel.ctypes.data,
                                    self.offset.ctypes.data, n, self.planes.data_ptr(), self.state_elems,
                                    coef.ctypes.data, int(t == 0), form, *tail, *more)
        else:
            lib, check = (_lib.load_clientloop(), _lib.check_clientloop) if gated else \
                (_lib.load_clientstep(), _lib.check_clientstep)
            name = f"fedavg_client_sgd_step_{'gated_' if gated else ''}{self.key}"
            rc = getattr(lib, name)(self.w.ptrs.ctypes.data, self.g[t].ptrs.ctypes.data, self.numel.ctypes.data, n,
                                    LR, form, *tail, *more)
        check(rc, name)
        torch.cuda.synchronize(self.dev)  # host_ws is rewritten by the next call

    def track(self, rec, abs_dloss):
        """fedavg_client_track* on rec's state from rec's two records."""
        base = rec.data_ptr()
        if self.key == "f32":
            lib, name, check = _lib.load(), "fedavg_client_track", lambda rc, what: _lib.check(rc, what, lib)
        else:
            lib, name, check = _lib.load_clientvec(), f"fedavg_client_track_{self.key}", _lib.check_clientvec
        check(getattr(lib, name)(base + 8 * STATE, base + 8 * W, base + 8 * G, abs_dloss, self.stream), name)
        torch.cuda.synchronize(self.dev)


def new_record(dev, gate):
    rec = torch.zeros(REC, dtype=torch.float64)
    rec[W:W + 4] = torch.tensor([DIRTY, DIRTY + 1, DIRTY + 2, DIRTY + 3])
    rec[G:G + 4] = torch.tensor([0.0, 3.5, 0.37, 0.0])  # the gradient record: sum d^2 = 0.37
    rec[LOSS], rec[LAST] = 0.6875, 1.3125
    rec[GATE], rec[EPOCH] = gate, (4.0 if gate else 0.0)
    return rec.to(dev)


@pytest.mark.parametrize("adam", (False, True), ids=("sgd", "adam"))
@pytest.mark.parametrize("name", tuple(LISTS))
@pytest.mark.parametrize("key", KEYS)
def test_open_gate_equals_the_ungated_entry_and_the_track_entry(dev, key, name, adam):
    run = Launch(name, key, dev, adam)
    for form in ((15, 5) if adam else (1, 0)):
        # the ungated entry, two chained steps, and fedavg_client_track* after each
        run.w.fresh()
        run.planes.zero_()
        plain = new_record(dev, 0.0)
        want = []
        losses = [(0.6875, 1.3125), (0.4375, 0.6875)]
        for t in range(2):
            run.step(t, form, plain, gated=False)
            run.track(plain, abs(losses[t][0] - losses[t][1]))
            want.append((run.w.buf.clone(), run.planes.clone(), plain.clone()))
        # the gated entry on the same inputs
        run.w.fresh()
        run.planes.zero_()
        rec = new_record(dev, 0.0)
        for t in range(2):
            rec[LOSS] = losses[t][0]
            run.step(t, form, rec, gated=True)
            w, planes, ref = want[t]
            assert same(run.w.buf, w), (form, t)            # the weights, sentinels included
            assert same(run.planes, planes), (form, t)      # m, v, vmax (zeros under SGD)
            assert same(rec[W:W + 4], ref[W:W + 4]), (form, t, rec[W:W + 4].tolist(), ref[W:W + 4].tolist())
            assert same(rec[STATE:STATE + 4], ref[STATE:STATE + 4]), (form, t, rec.tolist(), ref.tolist())
            assert float(rec[LOSS]) == float(rec[LAST]) == losses[t][0]  # loss moved to last_loss
            assert same(rec[G:G + 4], ref[G:G + 4]) and same(rec[GATE:], ref[GATE:])
        assert float(rec[STATE + 2]) == float(rec[STATE + 3]) == 1.0 and float(rec[W + 1]) > 0.0


@pytest.mark.parametrize("adam", (False, True), ids=("sgd", "adam"))
@pytest.mark.parametrize("name", tuple(LISTS))
@pytest.mark.parametrize("key", KEYS)
def test_set_gate_writes_nothing(dev, key, name, adam):
    run = Launch(name, key, dev, adam)
    run.planes.copy_(torch.from_numpy(np.random.default_rng(5).normal(0.0, 1.0, run.planes.numel())).to(run.dt))
    rec = new_record(dev, 1.0)
    rec[STATE:STATE + 4] = torch.tensor([DIRTY, DIRTY / 2, 1.0, 1.0], dtype=torch.float64)
    before = [t.clone() for t in (run.w.buf, run.planes, run.partials, rec)]
    for t, form in ((1, 15 if adam else 1), (0, 0)):  # a later step and a first one
        run.step(t, form, rec, gated=True)
        for was, now in zip(before, (run.w.buf, run.planes, run.partials, rec)):
            assert same(was, now), (t, form)


@pytest.mark.parametrize("key", KEYS)
def test_no_elements_zero_the_record_behind_the_gate(dev, key):
    """Keys without elements: no step launch; the finalize writes stats = 0 and tracks, or nothing under a set gate."""
    lib = _lib.load_clientloop()
    numel = np.zeros(2, dtype=np.int64)
    ptrs = np.array([4096, 8192], dtype=np.int64)
    host_ws = torch.empty(64, dtype=torch.uint8, pin_memory=True)
    dev_ws = torch.empty(64, dtype=torch.uint8, device=dev)
    partials = torch.full((4,), DIRTY, dtype=torch.float64, device=dev)
    name = f"fedavg_client_sgd_step_gated_{key}"
    for gate in (1.0, 0.0):
        rec = new_record(dev, gate)
        before = rec.clone()
        base = rec.data_ptr()
        rc = getattr(lib, name)(ptrs.ctypes.data, ptrs.ctypes.data, numel.ctypes.data, 2, LR, 1, partials.data_ptr(), 4,
                                base + 8 * W, host_ws.data_ptr(), dev_ws.data_ptr(), 64,
                                torch.cuda.current_stream(dev).cuda_stream, base + 8 * G, base + 8 * GATE,
                                base + 8 * STATE, base + 8 * LOSS)
        _lib.check_clientloop(rc, name)
        torch.cuda.synchronize(dev)
        if gate:
            assert same(rec, before)
        else:
            assert rec[W:W + 4].tolist() == [0.0] * 4 and float(rec[LAST]) == float(rec[LOSS])
            assert rec[STATE + 2:STATE + 4].tolist() == [1.0, 1.0]
