"""fedavg_client_adam_step_{f32,bf16,f16,f64} on the MI355X against the exact
host reference of tests/client_adam_ref.py (itself checked against rational
arithmetic in tests/test_client_adam_ref_cpu.py), at masks 0, 15 and each
single bit: w, m, v and vmax bit for bit over three chained steps, the record
under test_gpu_client_step_ref.py's rule and bound, on the launches of
tests/client_adam_cases.py, then first=1 against first=0 on a zeroed state,
wd = 0, the special values and the contract of a stream entry (guards around
every output, exactly sized workspaces, dirty scratch, a call behind a hold on
a side stream).

The sums: the reference's are math.fsum, exact.  The kernel adds at most 32
squares per thread in order, then 6 DPP steps, 3 waves, and in the finalize
kernel at most ceil(units / 256) partials per thread and 8 tree steps: under
64 roundings on any path, inside SUM_RTOL = 1e-11 (test_gpu_client_step.py)."""
import math
import types

import numpy as np
import pytest
import torch

import client_adam_cases as C
import client_adam_ref as A
from mfl_amd import _lib
from test_gpu_client_step import SUM_RTOL

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes of guard around every output


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    return _lib.load_clientadam()


def _same_sum(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == want or abs(got - want) <= SUM_RTOL * abs(want)


def _assert_bits(got, want, what):
    """Equal bits; NaN where the reference has NaN (payloads are not compared)."""
    nan_got, nan_want = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_got, nan_want), what
    wrong = (A.bits(got) != A.bits(want)) & ~nan_want
    assert not bool(wrong.any()), (what, int(wrong.sum()), torch.nonzero(wrong).view(-1)[:8].tolist())


def _assert_record(stats, want, what):
    nans, s_w, s_d = want
    print(f"{what}: got {stats.tolist()} want {(nans, s_w, s_d, 0)}")
    assert stats[0] == float(nans) and stats[3] == 0.0, what
    assert _same_sum(float(stats[1]), s_w) and _same_sum(float(stats[2]), s_d), what


def _guarded(n_bytes, dev, fill=0xA5):
    """(whole buffer, the n_bytes in its middle) with GUARD bytes of `fill` on either side."""
    buf = torch.full((GUARD + n_bytes + GUARD,), fill, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n_bytes]


def _guards_intact(buf, n_bytes, fill=0xA5):
    host = buf.cpu()
    return bool((host[:GUARD] == fill).all()) and bool((host[GUARD + n_bytes:] == fill).all())


class Adam:
    """fedavg_client_adam_step_* calls over one case: exactly sized, guarded state, partials, stats and dev_ws."""

    def __init__(self, lib, dev, c):
        self.lib, self.c, self.dev = lib, c, dev
        self.name = f"fedavg_client_adam_step_{c.key}"
        self.fn = getattr(lib, self.name)
        self.es = es = torch.empty(0, dtype=c.dt).element_size()
        n = len(c.numel)
        self.nparts = int(lib.fedavg_client_adam_partials(c.numel.ctypes.data, n, es))
        self.ws = int(lib.fedavg_client_adam_workspace(n))
        assert self.ws == 40 * n and self.nparts == 3 * int(((c.numel + C.UNIT[c.key] - 1) // C.UNIT[c.key]).sum())
        self.host_ws = torch.empty(max(self.ws, 16), dtype=torch.uint8, pin_memory=True)
        self.bufs = {"state": _guarded(3 * c.state_elems * es, dev), "partials": _guarded(8 * self.nparts, dev),
                     "stats": _guarded(32, dev), "dev_ws": _guarded(self.ws, dev)}
        self.state = self.bufs["state"][1].view(c.dt)
        self.state.zero_()
        self.stats = self.bufs["stats"][1].view(torch.float64)

    def run(self, w, g, coef, first, form, stream=None):
        c = self.c
        w_ptrs = np.array([t.data_ptr() for t in w], dtype=np.int64)
        g_ptrs = np.array([t.data_ptr() for t in g], dtype=np.int64)
        cf = np.array(coef, dtype=np.float64)
        st = torch.cuda.current_stream() if stream is None else stream
        rc = self.fn(w_ptrs.ctypes.data, g_ptrs.ctypes.data, c.numel.ctypes.data, c.state_offset.ctypes.data,
                     len(c.numel), self.state.data_ptr(), c.state_elems, cf.ctypes.data, int(first), form,
                     self.bufs["partials"][1].data_ptr(), self.nparts, self.stats.data_ptr(), self.host_ws.data_ptr(),
                     self.bufs["dev_ws"][1].data_ptr(), self.ws, st.cuda_stream)
        _lib.check_clientadam(rc, self.name)
        if stream is None:
            torch.cuda.synchronize()
            return self.stats.cpu().numpy()

    def planes(self):
        """(m, v, vmax) on the host, the keys' elements only, end to end."""
        host = self.state.cpu().view(3, self.c.state_elems)
        return tuple(host[i][torch.from_numpy(self.c.pos["s"])] for i in range(3))

    def guards_intact(self):
        sizes = {"state": 3 * self.c.state_elems * self.es, "partials": 8 * self.nparts, "stats": 32, "dev_ws": self.ws}
        return all(_guards_intact(self.bufs[k][0], n) for k, n in sizes.items())


def _chain(lib, dev, c, form, what, first_flags=None, **change):
    """The case's chained steps under one mask against the reference; returns the Adam object."""
    ref = c.reference(form, **change)
    w_buf = c.host_buffer("w", c.w).to(dev)
    adam = Adam(lib, dev, c)
    pos_w = torch.from_numpy(c.pos["w"])
    gap = torch.ones(c.size["w"], dtype=torch.bool)
    gap[pos_w] = False
    for t, ((want, rec)) in enumerate(ref):
        host_g = c.host_buffer("g", c.g[t])
        g_buf = host_g.to(dev)
        assert w_buf.data_ptr() % 16 == 0 and g_buf.data_ptr() % 16 == 0
        first = t == 0 if first_flags is None else first_flags[t]
        stats = adam.run(c.views(w_buf, "w"), c.views(g_buf, "g"), C.coef(t + 1, **change), first, form)
        tag = f"{what} step {t + 1}"
        w_out = w_buf.cpu()
        for name, got, ref_t in zip(("w", "m", "v", "vmax"), (w_out[pos_w], *adam.planes()), want):
            _assert_bits(got, ref_t, f"{tag} {name}")
        assert bool((w_out[gap] == C.SENTINEL).all()), tag          # nothing stored outside a key
        assert torch.equal(A.bits(g_buf.cpu()), A.bits(host_g)), tag  # g and its sentinels unchanged
        _assert_record(stats, rec, tag)
        assert adam.guards_intact(), tag
    return adam


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("form", C.MASKS)
@pytest.mark.parametrize("key", C.KEYS)
def test_edge_sizes_over_three_steps_equal_the_reference(lib, dev, key, form):
    """Keys of 1, span - 1, span, span + 1 and 2 span + 3 elements, t = 1, 2, 3."""
    _chain(lib, dev, C.case("edges", key), form, f"edges {key} form {form}")


@pytest.mark.parametrize("form", (0, 15))
@pytest.mark.parametrize("key", C.KEYS)
def test_130_keys_at_every_offset_equal_the_reference(lib, dev, key, form):
    c = C.case("k130", key)
    live = c.numel > 0
    assert set(zip((c.off["w"][live] == 0).tolist(), (c.off["g"][live] == 0).tolist())) == \
        {(True, True), (True, False), (False, True), (False, False)}
    assert set(c.off["w"][live].tolist()) == set(range(C.KPER[key])) == set(c.off["g"][live].tolist())
    _chain(lib, dev, c, form, f"k130 {key} form {form}")


@pytest.mark.parametrize("key", C.KEYS)
def test_a_key_of_more_than_256_units_equals_the_reference(lib, dev, key):
    _chain(lib, dev, C.case("long", key), 15, f"long {key}")


@pytest.mark.parametrize("key", C.KEYS)
def test_first_equals_a_step_that_reads_a_zeroed_state(lib, dev, key):
    """first=0 at t = 1 on the zeroed state: the same reference, so the same bits as first=1."""
    _chain(lib, dev, C.case("edges", key), 15, f"first=0 {key}", first_flags=[False, False, False])


@pytest.mark.parametrize("form", (0, 15))
@pytest.mark.parametrize("key", C.KEYS)
def test_without_weight_decay_there_is_no_op_a(lib, dev, key, form):
    _chain(lib, dev, C.case("edges", key), form, f"wd=0 {key} form {form}", wd=0.0)


@pytest.mark.parametrize("form", (0, 4, 15))
@pytest.mark.parametrize("key", ("bf16", "f16"))
def test_site_c_on_mined_pairs_in_a_later_step(lib, dev, key, form):
    """One key of client_adam_cases.site_c()'s pairs, w = 0, m = 0, vmax = v, first=0: site C's two forms store
    different v' on every element (no chained case reaches that site in a 16-bit type)."""
    coef, w, g, m, v, x = C.site_c(key)
    n, P = len(v), C.KPER[key]
    c = types.SimpleNamespace(key=key, dt=C.DTYPES[key], numel=np.array([n], np.int64),
                              state_offset=np.zeros(1, np.int64), state_elems=-(-n // P) * P,
                              pos={"s": np.arange(n)})
    want, rec = A.reference(key, form, coef, False, w, g, m, v, x)
    other = A.reference(key, form ^ 4, coef, False, w, g, m, v, x)[0]
    assert bool((A.bits(want[2]) != A.bits(other[2])).all())
    adam = Adam(lib, dev, c)
    state = adam.state.view(3, c.state_elems)
    state[1, :n] = v.to(dev)
    state[2, :n] = x.to(dev)
    w_dev, g_dev = w.to(dev), g.to(dev)
    stats = adam.run([w_dev], [g_dev], coef, False, form)
    for name, got, ref_t in zip(("w", "m", "v", "vmax"), (w_dev.cpu(), *adam.planes()), want):
        _assert_bits(got, ref_t, f"site C {key} form {form} {name}")
    _assert_record(stats, rec, f"site C {key} form {form}")
    assert adam.guards_intact()


# ------------------------------------------------------------- special values
@pytest.mark.parametrize("form", (0, 15))
@pytest.mark.parametrize("key", C.KEYS)
def test_special_values_equal_the_reference(lib, dev, key, form):
    """NaN and +-inf in g, g = 0 so that v = 0 and s3 = eps, subnormal v (tiny g), -0.0, values that overflow fp16."""
    c = C.Case("edges", key, steps=2)
    dt = c.dt
    tiny = torch.finfo(dt).smallest_normal
    for t in range(2):
        g = c.g[t]
        g[0], g[1], g[2] = math.nan, math.inf, -math.inf
        g[3], c.w[3] = 0.0, 0.0                       # wd * w + g = 0: v' = 0, s3 = eps, 0 / eps
        g[4], c.w[4] = 0.0, -0.0
        g[5], c.w[5] = math.sqrt(tiny) / 4, 0.0       # g1^2 subnormal: subnormal v and vmax
        g[6], c.w[6] = tiny / 2, tiny / 4             # subnormal g and w
        g[7], c.w[7] = 6.0e4, 6.0e4                   # g1^2 overflows fp16
        g[len(g) - 1] = math.nan                      # in the ragged last slice of the last key
    ref = c.reference(form)
    assert ref[0][1][0] >= 3 and math.isnan(ref[0][1][1])          # NaN counted, sums NaN
    v1 = ref[0][0][2]
    assert float(v1[3]) == 0.0 and bool(((v1.abs() < tiny) & (v1 != 0)).any())  # v = 0 and a subnormal v
    _chain(lib, dev, c, form, f"specials {key} form {form}")


# ------------------------------------------------------------------- contract
@pytest.mark.parametrize("key", C.KEYS)
def test_dirty_scratch_and_a_second_call_change_nothing(lib, dev, key):
    """partials and dev_ws full of 0xFF before a call: the same bytes as from clean scratch."""
    c = C.case("edges", key)
    want, rec = c.reference(15)[0]
    outs = []
    for dirty in (False, True):
        adam = Adam(lib, dev, c)
        if dirty:
            adam.bufs["partials"][1].fill_(0xFF)
            adam.bufs["dev_ws"][1].fill_(0xFF)
        w_buf, g_buf = c.host_buffer("w", c.w).to(dev), c.host_buffer("g", c.g[0]).to(dev)
        stats = adam.run(c.views(w_buf, "w"), c.views(g_buf, "g"), C.coef(1), True, 15)
        outs.append((stats.tobytes(), A.bits(w_buf.cpu()), A.bits(adam.state.cpu())))
        _assert_record(stats, rec, f"dirty={dirty} {key}")
        assert adam.guards_intact()
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("key", C.KEYS)
def test_a_call_behind_a_hold_on_a_side_stream_is_ordered(lib, dev, key):
    """The weights are written on a side stream before the call on that stream and read after it, with no host
    synchronisation in between: the call sees the written weights and the reader sees the step."""
    c = C.case("edges", key)
    want, rec = c.reference(15)[0]
    side = torch.cuda.Stream(dev)
    adam = Adam(lib, dev, c)
    host_w = c.host_buffer("w", c.w).pin_memory()
    g_buf = c.host_buffer("g", c.g[0]).to(dev)
    w_buf = torch.zeros(c.size["w"], dtype=c.dt, device=dev)
    out = torch.empty(c.size["w"], dtype=c.dt).pin_memory()
    big = torch.empty(1 << 26, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big.normal_()                        # the hold: work queued in front of the copy
        w_buf.copy_(host_w, non_blocking=True)
        adam.run(c.views(w_buf, "w"), c.views(g_buf, "g"), C.coef(1), True, 15, stream=side)
        out.copy_(w_buf, non_blocking=True)
        stats = adam.stats.to("cpu", non_blocking=True)
    side.synchronize()
    _assert_bits(out[torch.from_numpy(c.pos["w"])], want[0], f"side stream {key}")
    _assert_record(stats.numpy(), rec, f"side stream {key}")
