"""Strided, offset and shared client tensors through every route, on the GPU.

The numeric suite checks what the kernels do once they hold the right
addresses; these tests check the step before: that every route hands its
kernels the right bytes when a client's tensor is not a plain, freshly
allocated, contiguous block (tests/layouts.py is the catalogue).  The
reference's loop (fedavg_trainer.py:450-457, ``local_model_params[k] * w`` and
``+=``; :291 subtracts key by key) takes every such layout without special
cases, so the oracle on a plain host copy of the round is the truth.

Every aggregate is compared bit for bit, its :291 distances with the bound
test_gpu_delta.py uses, FPF's ``local_w_diffs`` bit for bit; every case also
asserts, by the aggregator's counters and ``_last`` fields, that the route it
names is the one that ran.
"""
import contextlib
import weakref
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fedavg_oracle as O
import fpf_oracle as FO
import layouts as L
import mfl_amd
from mfl_amd.layout import KeyTable
from mfl_amd.layout import _collect_ext
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
LR = 0.03

# dtype group -> (dtype of the key that takes the layout, integer buffers in the model?)
GROUPS = {"f32": (F32, False), "f32_int": (F32, True), "f64": (F64, True), "f16": (F16, True), "bf16": (BF16, True)}
HOST_ROUTES = ("small", "native2", "pipelined", "session", "session_streamed")
DEVICE_ROUTES = ("zero_copy", "rows", "session_device")
# a model with an fp64 / fp16 / bf16 key has two dtype groups: its host rounds
# are pipelined ones whatever the threshold, so the small-round routes and the
# small session would repeat `pipelined` / `session_streamed`
VEC_ROUTES = ("pipelined", "session_streamed") + DEVICE_ROUTES


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_available):
    mfl_amd._lib.load()
    torch.cuda.set_device(DEV)
    yield


def _round(layout, group, K, seed, device=None, clients=(0, 2)):
    """The catalogue round of a case: ``layout`` on the group's key (and on the
    uint8 ``mask`` where its shape allows) of client 0 and one other client."""
    dt, ints = GROUPS[group]
    key = L.TARGET[layout]
    lay, dts = {key: layout}, {key: dt}
    if layout == "shared":
        dts[L.TWIN[key]] = dt
    if ints and layout in L.INT_TARGET:
        lay[L.INT_TARGET[layout]] = layout
    keys = list(L.KEY_SHAPES) if ints else L.FLOAT_KEYS
    return L.model(lay, dts, K, seed, clients=clients, keys=keys, device=device)


def _cases():
    out = []
    for layout in L.LAYOUTS:
        for group in GROUPS:
            routes = HOST_ROUTES + DEVICE_ROUTES if GROUPS[group][0] == F32 else VEC_ROUTES
            for route in routes:
                ks = (3, 5, 20) if (group in ("f16", "bf16") and route == "zero_copy" and layout == "plain") else (3, 5)
                for K in ks:
                    out.append(pytest.param(layout, group, route, K, id=f"{layout}-{group}-{route}-K{K}"))
    return out


def _run_session(agg, w_locals):
    sess = agg.begin_round(w_locals[0][1], len(w_locals) + 2)
    for n, sd in w_locals:
        sess.add(n, sd)
    return sess, sess.finish(w_locals)


def _check_average(out, w_locals, first, keys, ref_glob, snap, on_device, what):
    assert out is first and out is w_locals[0][1]
    assert list(out.keys()) == keys
    for k, exp in ref_glob.items():
        assert out[k].device == (DEV if on_device else torch.device("cpu")), k
        assert_bits(out[k], exp, f"{what}/{k}")
    L.assert_untouched(snap, w_locals)


def _check_distances(agg, w_locals, w_glob, ref_locals, ref_glob, delta=True):
    """:291 cached (the round ``agg`` just ran), uncached on a fresh
    aggregator, and :293 through the functional form."""
    exact = O.client_distances_exact(ref_locals, ref_glob)
    cat = L.cat_dtype(ref_locals)
    assert exact[0] == 0.0
    refs = agg._last.get("refs")
    assert refs is not None and agg._last["acc"]() is w_glob and all(r() is sd for r, (_, sd) in zip(refs, w_locals))
    cached = agg.client_distances(w_locals, w_glob)
    assert cached[0] == 0.0
    L.assert_norms(cached, exact, cat)
    fresh = mfl_amd.DeviceAggregator(DEV).client_distances(w_locals, w_glob)
    assert fresh[0] == 0.0
    L.assert_norms(fresh, exact, cat)
    if delta:
        sample_nums = [n for n, _ in w_locals]
        got = mfl_amd.estimate_delta(w_locals, w_glob, LR, device=DEV)
        assert got == O.delta_from_norms(sample_nums, fresh, LR)  # the same norms, the same host arithmetic


@pytest.mark.parametrize("layout,group,route,K", _cases())
def test_layout_through_route(layout, group, route, K, monkeypatch):
    dt, _ = GROUPS[group]
    on_device = route in DEVICE_ROUTES
    w_locals, ref_locals = _round(layout, group, K, seed=K, device=DEV if on_device else None)
    ref_glob = O.aggregate_torch(ref_locals)
    keys, first, snap = list(w_locals[0][1]), w_locals[0][1], L.snapshot(w_locals)
    contiguous = layout in L.CONTIGUOUS
    agg = mfl_amd.DeviceAggregator(DEV)
    ext = _collect_ext()
    native = ext is not None and hasattr(ext, "small_round")

    if route == "small":
        out = agg.aggregate(w_locals)
        assert "sumsq" not in agg._last and agg.fast_rounds == 0  # fedavg_round_f32, through the general walk
        assert (agg._fast_small is not None) == native
    elif route == "native2":
        if not native:
            pytest.skip("collect extension not built")
        plain_locals, _ = _round("plain", group, K, seed=100 + K)
        agg.aggregate(plain_locals)
        assert agg._fast_small is not None and agg.fast_rounds == 0
        out = agg.aggregate(w_locals)
        # the native walk reads contiguous tensors in place and declines any other
        assert agg.fast_rounds == (1 if contiguous else 0)
        assert "sumsq" not in agg._last and agg._fast_small is not None
    elif route == "pipelined":
        agg.SMALL_ROUND_BYTES = 0
        out = agg.aggregate(w_locals)
        assert "sumsq" in agg._last and agg._fast_small is None and agg.fast_rounds == 0
        assert agg.last_profile["pack_issue_ms"] > 0.0
    elif route in ("session", "session_streamed"):
        if route == "session_streamed":
            agg.SMALL_ROUND_BYTES = 0
        sess, out = _run_session(agg, w_locals)
        assert sess._small == (route == "session") and sess._client_dev.type == "cpu"
        assert agg._last["table"] is sess.table
    elif route == "zero_copy":
        monkeypatch.setattr(mfl_amd.DeviceAggregator, "DEVICE_SEGMENTS", True)
        out = agg.aggregate(w_locals)
        assert agg._last.get("segments") is True and agg._last["dev"][F32][0] is None
        sums = agg._last.get("sumsq", {})
        if dt == F32:
            # an fp32 source off 16-B alignment: the reduce alone (return code 1), no fused sums
            assert (F32 in sums) == (layout != "offset1")
            assert agg.vec_zero_copy_rounds == 0
        else:
            # a 16-bit / fp64 source off 16-B alignment: the library answers FEDAVG_EALIGN, rows are packed
            took = layout != "offset1"
            assert agg.vec_zero_copy_rounds == (1 if took else 0)
            assert (agg._last["dev"][dt][0] is None) == took
            assert F32 in sums and dt in sums
    elif route == "rows":
        monkeypatch.setattr(mfl_amd.DeviceAggregator, "DEVICE_SEGMENTS", False)
        out = agg.aggregate(w_locals)
        assert not agg._last.get("segments") and agg.vec_zero_copy_rounds == 0
        assert all(rows is not None for rows, _ in agg._last["dev"].values())
    else:
        sess, out = _run_session(agg, w_locals)
        assert not sess._small and sess._client_dev == DEV
        assert all(rows is not None for rows, _ in agg._last["dev"].values())
    assert agg.arena_rounds == 0
    assert set(agg._last["dev"]) == ({F32} if dt == F32 else {F32, dt})
    assert agg._last["K"] == K

    _check_average(out, w_locals, first, keys, ref_glob, snap, on_device, f"{layout}/{group}/{route}")
    _check_distances(agg, w_locals, out, ref_locals, ref_glob)
    L.assert_untouched(snap, w_locals)


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("layout", list(L.LAYOUTS))
def test_device_packer_matches_host_packer_in_every_layout(layout, group):
    """fedavg_pack_rows_device over the pointers ``collect`` gives for device
    clients == fedavg_pack_rows over those it gives for the same round on the
    host (which test_layouts_host.py pins to torch.cat), byte for byte,
    padding included.  A 16-bit / fp64 key at ``offset1`` takes the pack
    kernel's element-by-element path."""
    K = 3
    host_locals, _ = _round(layout, group, K, seed=31)
    dev_locals, _ = _round(layout, group, K, seed=31, device=DEV)
    lib = mfl_amd._lib.load()
    agg = mfl_amd.DeviceAggregator(DEV)
    table = KeyTable(host_locals[0][1])
    h_ptrs, h_keep = table.collect([sd for _, sd in host_locals])
    d_ptrs, d_keep = table.collect([sd for _, sd in dev_locals], DEV)
    assert len(h_keep) == len(d_keep) == (0 if layout in L.CONTIGUOUS else 2)
    for g in table.groups.values():
        host = torch.zeros((K, g.ld), dtype=g.dtype)
        items = table.pack_items(g, h_ptrs, 0, g.ld)
        mfl_amd._lib.check(lib.fedavg_pack_rows(items.ctypes.data, items.shape[0], host.data_ptr(),
                                                host.element_size(), 2), "fedavg_pack_rows")
        dev = torch.zeros((K, g.ld), dtype=g.dtype, device=DEV)
        agg._pack_on_device(table, g, d_ptrs, 0, dev, torch.cuda.current_stream(DEV))
        assert torch.equal(dev.cpu().view(torch.uint8), host.view(torch.uint8)), (layout, g.dtype)
    del h_keep, d_keep


# ---------------------------------------------------------------------------
# FPF bookkeeping (fedavg_trainer.py:209-210) from clients in every layout
# ---------------------------------------------------------------------------
_FPF_LAYOUTS = [k for k in L.LAYOUTS if k != "plain"]
# the uint8 mask stays out: the reference's `w - last_w` wraps in uint8 before
# torch.cat promotes it, which is a question of dtypes, not of layouts
_FPF_KEYS = [k for k in L.KEY_SHAPES if k != "mask"]


@pytest.mark.parametrize("mode", ["record_client", "record_round"])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("group", ["f32_int", "f16"])
@pytest.mark.parametrize("layout", _FPF_LAYOUTS)
def test_fpf_rows_from_clients_in_every_layout(layout, group, where, mode):
    dt, _ = GROUPS[group]
    key = L.TARGET[layout]
    dts = {key: dt}
    if layout == "shared":
        dts[L.TWIN[key]] = dt
    K, n_total, idx = 3, 8, [5, 1, 7]
    device = DEV if where == "device" else None
    w_locals, ref_locals = L.model({key: layout}, dts, K, seed=11, keys=_FPF_KEYS, device=device)
    (_, last_w), (_, last_ref) = (x[0] for x in L.model({}, dts, 1, seed=12, keys=_FPF_KEYS, device=device))
    agg = mfl_amd.DeviceAggregator(DEV)
    t = mfl_amd.FPFTracker(n_total, last_ref, 2, device=DEV, aggregator=agg)
    assert t.full and t._mixed == (group == "f16")  # the f16 model runs fedavg_fpf_cat_diff
    o = FO.FPFOracle(n_total, sum(v.numel() for v in last_ref.values()), 2)
    for c, (_, sd) in zip(idx, ref_locals):
        o.record_client(c, sd, last_ref)
    t.begin_round(last_w)
    if mode == "record_client":
        for c, (_, sd) in zip(idx, w_locals):
            t.record_client(c, sd)
    w_glob = agg.aggregate(w_locals)
    if mode == "record_round":
        t.record_round(idx, w_locals, w_glob)
    assert torch.equal(t.local_w_diffs.cpu(), o.local_w_diffs)  # bit-identical, as test_gpu_fpf.py requires
    ref_glob = O.aggregate_torch(ref_locals)
    for k, exp in ref_glob.items():
        assert_bits(w_glob[k], exp, f"{layout}/{group}/{where}/{k}")


# ---------------------------------------------------------------------------
# round-to-round changes on one aggregator
# ---------------------------------------------------------------------------
def _allocation_heavy_step(agg):
    """Device tensors of the sizes the last round used, filled with NaN: a
    copy or a cached buffer freed too early is handed out again here."""
    sizes = set()
    for dt, (rows, out_dev) in agg._last["dev"].items():
        g = agg._last["table"].groups[dt]
        sizes.update((g.P * out_dev.element_size(), agg._last["K"] * g.ld * out_dev.element_size()))
        sizes.update(e.numel * out_dev.element_size() for e in g.keys)
    return [torch.full((max(1, (n + 3) // 4),), float("nan"), dtype=F32, device=DEV)
            for n in sorted(sizes) for _ in range(3)]


@pytest.mark.parametrize("where", ["host", "device"])
def test_round_to_round_changes_on_one_aggregator(where, monkeypatch):
    on_device = where == "device"
    device = DEV if on_device else None
    monkeypatch.setattr(mfl_amd.DeviceAggregator, "DEVICE_SEGMENTS", True)
    agg = mfl_amd.DeviceAggregator(DEV)
    ext = _collect_ext()
    native = ext is not None and hasattr(ext, "small_round")
    state = {"r": 0, "glob": None}

    def run(w_locals, ref_locals, delay=False):
        state["r"] += 1
        ref_glob = O.aggregate_torch(ref_locals)
        keys, first, snap = list(w_locals[0][1]), w_locals[0][1], L.snapshot(w_locals)
        out = agg.aggregate(w_locals)
        junk = _allocation_heavy_step(agg) if delay else None
        _check_average(out, w_locals, first, keys, ref_glob, snap, on_device, f"{where} round {state['r']}")
        _check_distances(agg, w_locals, out, ref_locals, ref_glob, delta=False)
        del junk
        state["glob"] = out
        return out

    def from_last_glob(w_locals, ref_locals):
        """Client 0's dict IS last round's w_glob (views of its output buffer),
        as the reference's clients start from the model :219 loaded."""
        glob = state["glob"]
        n0 = w_locals[0][0]
        ref0 = OrderedDict((k, v.detach().cpu().clone()) for k, v in glob.items())
        return [(n0, glob)] + w_locals[1:], [(n0, ref0)] + ref_locals[1:]

    fp16_w = {"fc.weight": F16}
    # 1. plain, K = 5
    run(*L.model({}, None, 5, 1, device=device))
    assert agg.fast_rounds == 0 and (on_device or (agg._fast_small is not None) == native)
    # 2. same keys, client 2's fc.weight transposed; its distances only after an allocation-heavy step
    run(*L.model({"fc.weight": "transposed"}, None, 5, 2, clients=(2,), device=device), delay=True)
    assert agg.fast_rounds == 0  # the native walk declined the transposed tensor
    # 3. plain again: the fast path resumes
    run(*L.model({}, None, 5, 3, device=device))
    if on_device:
        assert agg._last.get("segments") is True and F32 in agg._last["sumsq"]
    else:
        assert agg.fast_rounds == (1 if native else 0)
    hint3 = agg._table_hint
    assert hint3 is not None and set(hint3.groups) == {F32}
    # 4. fc.weight becomes fp16 in every client: the table hint is dropped
    vec0 = agg.vec_zero_copy_rounds
    run(*L.model({}, fp16_w, 5, 4, device=device))
    hint4 = agg._table_hint
    assert hint4 is not hint3 and set(hint4.groups) == {F32, F16} and agg._fast_small is None
    assert agg.vec_zero_copy_rounds == vec0 + (1 if on_device else 0)
    # 5. K = 3 with `big` at offset1 (fp32, 4-byte aligned): the same table serves
    run(*L.model({"big": "offset1"}, fp16_w, 3, 5, device=device))
    if ext is not None:
        assert agg._table_hint is hint4
    if on_device:
        assert F32 not in agg._last.get("sumsq", {}) and agg.vec_zero_copy_rounds == vec0 + 2
    #    ... and a round whose client 0 is that round's w_glob (its integer keys came back fp32, :455)
    loaded = dict(fp16_w, **{k: F32 for k in L.INT_KEYS})
    run(*from_last_glob(*L.model({}, loaded, 3, 6, device=device)))
    # 6. K = 20 bf16-only, then K = 5 bf16-only: the per-K answer of the 16-bit library is remembered per table
    bf = {k: BF16 for k in L.FLOAT_KEYS}
    vec0 = agg.vec_zero_copy_rounds
    run(*L.model({}, bf, 20, 7, keys=L.FLOAT_KEYS, device=device))
    assert agg.vec_zero_copy_rounds == vec0 + (1 if on_device else 0)
    run(*L.model({}, bf, 5, 8, keys=L.FLOAT_KEYS, device=device))
    assert agg.vec_zero_copy_rounds == vec0 + (2 if on_device else 0)
    assert set(agg._table_hint.groups) == {BF16}
    # 7. client 0's dict is last round's w_glob
    run(*from_last_glob(*L.model({}, bf, 3, 9, keys=L.FLOAT_KEYS, device=device)))
    assert agg.fast_rounds == (1 if native and not on_device else 0)


# ---------------------------------------------------------------------------
# lifetime of the contiguous copies
# ---------------------------------------------------------------------------
def _on(stream):
    return contextlib.nullcontext() if stream is None else torch.cuda.stream(stream)


@pytest.mark.parametrize("side", [False, True], ids=["default_stream", "side_stream"])
@pytest.mark.parametrize("group", ["f32_int", "f16"])
@pytest.mark.parametrize("route", ["zero_copy", "rows", "session_device", "session_streamed"])
def test_contiguous_copies_outlive_the_kernels_that_read_them(route, group, side, monkeypatch):
    """Right after the round returns -- no synchronization -- tensors of the
    non-contiguous key's byte size are allocated on the current stream and
    filled with NaN.  The caching allocator hands freed blocks back per
    stream: a copy freed before its reader was issued, or made on one stream
    and read on another, puts the NaNs into the average."""
    K = 5
    on_device = route != "session_streamed"
    dt, _ = GROUPS[group]
    monkeypatch.setattr(mfl_amd.DeviceAggregator, "DEVICE_SEGMENTS", route == "zero_copy")
    w_locals, ref_locals = _round("step2", group, K, seed=21, device=DEV if on_device else None,
                                  clients=tuple(range(K)))  # `big` strided in every client
    ref_glob = O.aggregate_torch(ref_locals)
    n = L.KEY_SHAPES["big"][0]
    agg = mfl_amd.DeviceAggregator(DEV)
    if route == "session_streamed":
        agg.SMALL_ROUND_BYTES = 0
    torch.cuda.synchronize()  # the clients' tensors were made on the default stream
    s = torch.cuda.Stream(DEV) if side else None
    with _on(s):
        if route.startswith("session"):
            _, out = _run_session(agg, w_locals)
        else:
            out = agg.aggregate(w_locals)
        junk = [torch.full((n,), float("nan"), dtype=dt, device=DEV) for _ in range(2 * K)]
        torch.cuda.current_stream(DEV).synchronize()
    if s is not None:
        torch.cuda.current_stream(DEV).wait_stream(s)
    for k, exp in ref_glob.items():
        assert_bits(out[k], exp, f"{route}/{group}/{k}")
    assert all(bool(torch.isnan(j).all()) for j in junk)
    with _on(s):
        _check_distances(agg, w_locals, out, ref_locals, ref_glob, delta=False)


@pytest.mark.parametrize("route", ["zero_copy", "rows"])
def test_copies_are_held_until_the_launches_are_issued(route, monkeypatch):
    """``aggregate`` may drop the contiguous copies only once the kernels that
    read them are in the stream: every copy ``collect`` made is still alive
    when ``_reduce_groups_device`` is entered and when it returns."""
    monkeypatch.setattr(mfl_amd.DeviceAggregator, "DEVICE_SEGMENTS", route == "zero_copy")
    w_locals, ref_locals = _round("step2", "f16", 5, seed=23, device=DEV, clients=(0, 1, 2, 3, 4))
    ref_glob = O.aggregate_torch(ref_locals)
    made, seen = [], []
    collect = KeyTable.collect

    def recording_collect(self, *a, **kw):
        ptrs, keep = collect(self, *a, **kw)
        made.extend(weakref.ref(t) for ts in keep for t in ts)
        return ptrs, keep

    reduce_device = mfl_amd.DeviceAggregator._reduce_groups_device

    def watched_reduce(self, *a, **kw):
        seen.append(sum(r() is not None for r in made))
        try:
            return reduce_device(self, *a, **kw)
        finally:
            seen.append(sum(r() is not None for r in made))

    monkeypatch.setattr(KeyTable, "collect", recording_collect)
    monkeypatch.setattr(mfl_amd.DeviceAggregator, "_reduce_groups_device", watched_reduce)
    out = mfl_amd.DeviceAggregator(DEV).aggregate(w_locals)
    n_keys = len(w_locals[0][1])
    assert len(made) == 5 * n_keys  # every client had a strided key: one kept list of its tensors each
    assert seen == [len(made), len(made)]
    for k, exp in ref_glob.items():
        assert_bits(out[k], exp, f"{route}/{k}")


def test_session_holds_device_copies_until_finish():
    """A streamed round packs a device client on the copy stream: the copies
    ``add`` made stay in the session until ``finish`` has ordered the current
    stream after that stream."""
    w_locals, ref_locals = _round("transposed", "f32_int", 3, seed=25, device=DEV)
    ref_glob = O.aggregate_torch(ref_locals)
    agg = mfl_amd.DeviceAggregator(DEV)
    sess = agg.begin_round(w_locals[0][1], 3)
    for n, sd in w_locals:
        sess.add(n, sd)
    assert len(sess._keepalive) == 2  # clients 0 and 2
    held = [weakref.ref(t) for keep in sess._keepalive for ts in keep for t in ts if not any(
        t is v for _, sd in w_locals for v in sd.values())]
    assert len(held) == 4  # fc.weight and mask of both clients
    out = sess.finish(w_locals)
    assert sess._keepalive == []
    for k, exp in ref_glob.items():
        assert_bits(out[k], exp, k)


@pytest.mark.parametrize("layout", ["transposed", "channels_last"])
def test_client_stats_still_rejects_non_contiguous_parameters(layout):
    """ClientStepStats takes the parameters' raw addresses and makes no copies:
    its fused mode is for contiguous fp32 parameters, and asking for it with
    any other layout is a TypeError, not a read of the wrong bytes."""
    from mfl_amd.client_stats import ClientStepStats, _fused_ok

    values = torch.randn(L.KEY_SHAPES[L.TARGET[layout]], device=DEV)
    p = L.LAYOUTS[layout](values)
    assert not p.is_contiguous() and torch.equal(p, values)
    assert _fused_ok([values]) and not _fused_ok([values, p])
    with pytest.raises(TypeError):
        ClientStepStats([values, p], stats="hip")
