"""The promises the three product headers make for every entry that takes a
stream, checked through the C ABI on the case table of tests/abi_cases.py:

a. bounds and const inputs: every output and workspace sits inside a larger
   allocation with 4 KiB of 0xA5 in front and behind, workspaces exactly as
   large as the query answers; after the call the result is right, the guards
   are intact and every input holds the bytes that were uploaded;
b. dirty scratch: workspaces and outputs start as 0xFF bytes (NaN), and the
   call runs twice on the same scratch with other inputs the second time;
c. stream order: on a non-blocking side stream, behind a hold kernel, the real
   inputs are copied in, the call is made, the outputs are copied out and
   everything is poisoned -- the stream must still be busy when the call
   returns, and the copies must hold the right result; entries that stage
   tables also run as a pair that shares dev_ws behind one hold;
d. two streams at once, each with its own buffers.

Only value buffers are ever poisoned, never index, key or pointer tables: a
wrongly ordered launch reads wrong values, not a wrong address.  In the stream
tests a staged dev_ws is never filled with 0xFF either: it holds pointers.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import abi_cases as A

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = 0xA5
HOLD_FACTOR = 5  # margin for host jitter; the premise assertion is what guards the test
_holds = {}  # case name -> the hold its stream-order test used (cycles)


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L(dev):
    return A.libs()


def _hip_runtime():
    """The HIP runtime torch has loaded."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "torch has no HIP runtime loaded"
    return ctypes.CDLL(sorted(paths)[0])


def _is_non_blocking(hip, stream):
    flags = ctypes.c_uint(0)
    assert hip.hipStreamGetFlags(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags)) == 0
    return bool(flags.value & 1)  # hipStreamNonBlocking


@pytest.fixture(scope="module")
def sides(dev):
    """Two non-blocking side streams (the kind the product runs the entries on)."""
    torch.zeros(1, device=dev)
    hip = _hip_runtime()
    made, out = [], []
    for _ in range(2):
        s = torch.cuda.Stream(device=dev)
        if not _is_non_blocking(hip, s):
            h = ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(h), ctypes.c_uint(1)) == 0
            made.append(h)
            s = torch.cuda.ExternalStream(h.value, device=dev)
        assert s.cuda_stream != 0 and _is_non_blocking(hip, s)
        out.append(s)
    yield out
    torch.cuda.synchronize()
    for h in made:
        hip.hipStreamDestroy(h)


@pytest.fixture(scope="module")
def cycles_per_ms(dev):
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(1_000_000)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    print(f"_sleep(1_000_000) took {ms:.3f} ms")
    assert ms > 0
    return 1_000_000 / ms


class CaseData:
    """A case's two input draws and their expectations, computed once and shared by the four tests."""

    def __init__(self, case):
        self.case = case
        self.inp = [case.build(np.random.default_rng(seed)) for seed in (1, 2)]
        self.exp = [case.expected(i) for i in self.inp]


@pytest.fixture(scope="module", params=A.CASES, ids=lambda c: c.name)
def cd(request, L):
    return CaseData(request.param)


class Addr:
    """name -> address for Case.call; n[name]: the buffer's bytes."""

    def __init__(self, addr, n, events):
        self._addr, self.n, self._events = addr, n, events

    def __getattr__(self, name):
        try:
            return self._addr[name]
        except KeyError:
            raise AttributeError(name)

    def __getitem__(self, name):
        return self._addr[name]

    def events(self):
        return self._events


class Arena:
    """The buffers of one call.  Device and pinned buffers are views into
    larger allocations filled with PATTERN; `shared` hands in views of another
    arena (a dev_ws two calls share)."""

    def __init__(self, inp, L, dev, shared=None):
        self.dev, self.L = dev, L
        self.alloc, self.view, self.nbytes, self.hostmem = {}, {}, {}, {}
        for name, b in inp.bufs.items():
            n = b.data.nbytes if b.data is not None else int(b.size(L))
            assert n >= 0, (name, n)
            self.nbytes[name] = n
            if b.where == "host":
                continue
            if shared and name in shared:
                self.view[name] = shared[name]
                assert shared[name].numel() == n
                continue
            total = GUARD + 256 + b.off + n + GUARD
            t = (torch.empty(total, dtype=torch.uint8, pin_memory=True) if b.where == "pinned" else
                 torch.empty(total, dtype=torch.uint8, device=dev))
            t.fill_(PATTERN)
            start = (t.data_ptr() + GUARD + 255) // 256 * 256 + b.off - t.data_ptr()
            assert GUARD <= start and start + n + GUARD <= total
            self.alloc[name] = (t, start)
            self.view[name] = t[start:start + n]
            assert self.view[name].data_ptr() % 256 == b.off
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for ev in e:
            ev.record()
        self._ev = e
        self.ff = torch.full((max([16] + list(self.nbytes.values())),), 0xFF, dtype=torch.uint8, device=dev)
        self.inp = None

    # -- data ---------------------------------------------------------------
    def _resolve(self, inp):
        """Host arrays and the bytes of every data buffer, pointer tables filled in."""
        addr = {name: v.data_ptr() for name, v in self.view.items()}
        self.hostmem = {name: np.array(b.data, copy=True) for name, b in inp.bufs.items() if b.where == "host"}
        addr.update({name: a.ctypes.data for name, a in self.hostmem.items()})
        content = {}
        for name, b in inp.bufs.items():
            if b.data is None:
                continue
            arr = self.hostmem[name] if b.where == "host" else np.array(b.data, copy=True)
            if b.ptr_of is not None:
                flat = arr.reshape(-1)
                for i, target in enumerate(b.ptr_of):
                    if target is not None:
                        flat[i] += addr[target]
            content[name] = arr
        self.addr = Addr(addr, dict(self.nbytes), tuple(ev.cuda_event for ev in self._ev))
        return content

    def load(self, inp, only=None, skip=()):
        """Upload the data buffers of `inp` (all, or those `only(buf)` selects);
        returns device copies of the uploaded bytes by name."""
        self.inp = inp
        content = self._resolve(inp)
        staged = {}
        for name, arr in content.items():
            b = inp.bufs[name]
            if b.where == "host" or arr.nbytes == 0:
                continue
            staged[name] = torch.from_numpy(arr.reshape(-1).view(np.uint8)).to(self.dev)
            if name not in skip and (only is None or only(b)):
                self.view[name].copy_(staged[name])
        self.host_before = {name: a.copy() for name, a in self.hostmem.items()}
        return staged

    def fill(self, names, byte=0xFF):
        for name in names:
            if name in self.view and self.nbytes[name]:
                self.view[name].fill_(byte)

    def names(self, pred):
        return [name for name, b in self.inp.bufs.items() if b.where != "host" and pred(b)]

    def download(self, name, src=None):
        b = self.inp.bufs[name]
        raw = (self.view[name] if src is None else src).cpu().numpy()
        return raw.view(b.data.dtype).reshape(b.data.shape)

    def outputs(self, src=None):
        return {name: self.download(name, None if src is None else src[name]) for name in self.inp.cmp}

    # -- checks ---------------------------------------------------------------
    def guards_intact(self):
        bad = torch.zeros((), dtype=torch.int64, device=self.dev)
        for name, (t, start) in self.alloc.items():
            n = self.nbytes[name]
            for part in (t[:start], t[start + n:]):
                bad += torch.count_nonzero(part.to(self.dev, non_blocking=False) != PATTERN)
        if int(bad) == 0:
            return
        for name, (t, start) in self.alloc.items():  # name the buffer and the first stray byte
            n = self.nbytes[name]
            for where, part, base in (("front", t[:start], -start), ("behind", t[start + n:], n)):
                hit = torch.nonzero(part != PATTERN)
                assert hit.numel() == 0, f"{name}: guard {where} overwritten at byte {base + int(hit[0])} of the buffer"

    def inputs_untouched(self, staged):
        for name, b in self.inp.bufs.items():
            if b.role in ("value", "table"):
                if b.where == "host":
                    assert np.array_equal(self.hostmem[name].view(np.uint8), self.host_before[name].view(np.uint8)), name
                elif self.nbytes[name]:
                    assert torch.equal(self.view[name].to(self.dev), staged[name]), f"{name}: an input was written"


def _null():
    return torch.cuda.current_stream().cuda_stream


def _call(case, L, ar, stream):
    rc = case.call(L, ar.inp, ar.addr, stream)
    assert rc == ar.inp.rc, (case.name, rc, L.main.fedavg_last_error())


# ---------------------------------------------------------------------------
# a. bounds and const inputs
# ---------------------------------------------------------------------------
def test_bounds_and_const_inputs(cd, L, dev):
    """The probe entry of the window and hand-off cases has no workspace query:
    their workspace is the bound the window tests allocate, so the guard behind
    it does not stand at "exactly the queried size" there (an over-read of the
    partials shows in test b alone for those cases)."""
    case, inp = cd.case, cd.inp[0]
    ar = Arena(inp, L, dev)
    staged = ar.load(inp)
    torch.cuda.synchronize()
    _call(case, L, ar, _null())
    torch.cuda.synchronize()
    case.compare(inp, ar.outputs(), cd.exp[0])
    ar.guards_intact()
    ar.inputs_untouched(staged)


# ---------------------------------------------------------------------------
# b. dirty scratch, twice
# ---------------------------------------------------------------------------
def test_dirty_scratch_twice(cd, L, dev):
    case = cd.case
    ar = Arena(cd.inp[0], L, dev)
    dirty = lambda b: b.role == "ws" or (b.role == "out" and b.dirty)
    for i in (0, 1):
        inp = cd.inp[i]
        if i == 0:
            ar.load(inp)
            ar.fill(ar.names(dirty))  # 0xFF bytes: NaN in every float format
        else:
            ar.load(inp, only=lambda b: not dirty(b))  # scratch and outputs keep what the first call left
        torch.cuda.synchronize()
        _call(case, L, ar, _null())
        torch.cuda.synchronize()
        case.compare(inp, ar.outputs(), cd.exp[i])
    ar.guards_intact()


# ---------------------------------------------------------------------------
# c. stream order
# ---------------------------------------------------------------------------
def _is_value(b):
    return b.role == "value" or b.inout


def _prepare(ar, inp):
    """Tables in place, value buffers and outputs holding 0xFF; returns the real bytes on the device."""
    staged = ar.load(inp, only=lambda b: b.role == "table")
    ar.fill([n for n in ar.names(lambda b: b.role != "table") if n != "dev_ws"])
    res = {name: torch.zeros(ar.nbytes[name], dtype=torch.uint8, device=ar.dev) for name in inp.cmp}
    return staged, res


def _copy_in(ar, staged):
    for name in ar.names(_is_value):
        if ar.nbytes[name]:
            ar.view[name].copy_(staged[name], non_blocking=True)


def _copy_out_and_poison(ar, res):
    for name, r in res.items():
        if r.numel():
            r.copy_(ar.view[name], non_blocking=True)
    for name in ar.names(lambda b: _is_value(b) or b.role == "out"):
        n = ar.nbytes[name]
        if n:  # a stream-ordered copy: a pinned buffer must not be poisoned by the host ahead of the stream
            ar.view[name].copy_(ar.ff[:n], non_blocking=True)


def _sequence(case, L, ars, stageds, ress, stream, hold, premise):
    """Behind a hold on `stream`: inputs in, the call(s), outputs out, poison."""
    with torch.cuda.stream(stream):
        if hold:
            torch.cuda._sleep(hold)
        for ar, staged in zip(ars, stageds):
            _copy_in(ar, staged)
        for ar in ars:
            _call(case, L, ar, stream.cuda_stream)
        busy = not stream.query()
        for ar, res in zip(ars, ress):
            _copy_out_and_poison(ar, res)
    if premise:
        assert busy, "the stream was idle when the call returned: the hold was too short to prove anything"
    return busy


def _hold_for(name, cycles_per_ms, host_ms):
    """HOLD_FACTOR times the host time the same sequence just took on the
    null stream, 1 ms at least.  Per case, not per module: the first call
    after a code object is loaded would otherwise set every later hold."""
    hold = int(cycles_per_ms * max(HOLD_FACTOR * host_ms, 1.0))
    _holds[name] = max(hold, _holds.get(name, 0))
    print(f"{name}: the call sequence took {host_ms:.3f} ms of host time, hold {hold} cycles")
    return hold


def _run_ordered(case, L, dev, inps, exps, stream, cycles_per_ms, share_dev_ws=False):
    ars = [Arena(inps[0], L, dev)]
    for inp in inps[1:]:
        ars.append(Arena(inp, L, dev, shared={"dev_ws": ars[0].view["dev_ws"]} if share_dev_ws else None))
    # once on the null stream without a hold: the kernels are loaded and the host time of the sequence is known
    prep = [_prepare(ar, inp) for ar, inp in zip(ars, inps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _sequence(case, L, ars, [p[0] for p in prep], [p[1] for p in prep], torch.cuda.current_stream(), 0, False)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    hold = _hold_for(case.name, cycles_per_ms, host_ms)
    prep = [_prepare(ar, inp) for ar, inp in zip(ars, inps)]
    torch.cuda.synchronize()
    busy = _sequence(case, L, ars, [p[0] for p in prep], [p[1] for p in prep], stream, hold, not case.sync)
    if case.sync:
        assert not busy, "a synchronous entry left work on the stream"
    stream.synchronize()
    for ar, inp, exp, (_, res) in zip(ars, inps, exps, prep):
        case.compare(inp, ar.outputs(res), exp)
    torch.cuda.synchronize()


def test_stream_order(cd, L, dev, sides, cycles_per_ms):
    _run_ordered(cd.case, L, dev, cd.inp[:1], cd.exp[:1], sides[0], cycles_per_ms)
    if cd.case.staged:  # two calls back to back behind one hold: shared dev_ws, own host_ws, own clients and outputs
        _run_ordered(cd.case, L, dev, cd.inp, cd.exp, sides[0], cycles_per_ms, share_dev_ws=True)


# ---------------------------------------------------------------------------
# d. two streams at once
# ---------------------------------------------------------------------------
def test_two_streams_at_once(cd, L, dev, sides, cycles_per_ms):
    case = cd.case
    ars = [Arena(inp, L, dev) for inp in cd.inp]
    prep = [_prepare(ar, inp) for ar, inp in zip(ars, cd.inp)]
    torch.cuda.synchronize()
    hold = _holds.get(case.name) or int(cycles_per_ms)
    for ar, (staged, res), s in zip(ars, prep, sides):
        _sequence(case, L, [ar], [staged], [res], s, hold, False)
    for s in sides:
        s.synchronize()
    for ar, inp, exp, (_, res) in zip(ars, cd.inp, cd.exp, prep):
        case.compare(inp, ar.outputs(res), exp)
    torch.cuda.synchronize()
