"""The case table of the C-ABI contract tests (tests/test_gpu_abi_contract.py)
-- TEST INFRASTRUCTURE ONLY, importable without a GPU.

One ``Case`` per entry point of include/fedavg_amd.h, fedavg_amd_fusedvec.h
and fedavg_amd_segvec.h that takes a ``void* stream``, at the smallest shapes
that reach each code path.  A case's ``build(rng)`` draws host-side numpy
inputs and names every buffer of the call with its role:

  value  float / 16-bit / integer-key data the kernels read as numbers;
  table  index, key, flag or pointer arrays (device or host): what a kernel
         turns into an address -- never poisoned by the stream tests;
  out    what the call writes (``inout``: state it reads and rewrites);
  ws     scratch, sized to exactly what the entry's query answers.

``expected`` comes from the CPU references only (oracle/fedavg_oracle.py,
tests/fpf_kernel_ref.py, tests/client_stats_oracle.py, numpy fp64 sums of the
rounded differences, plain copies for the packers and transfers), ``call``
makes the ctypes call on addresses the GPU tests hand in, ``compare`` holds
each output to the bar its own module's tests hold it to.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

import client_stats_oracle as CS
import fedavg_oracle as O
import fpf_kernel_ref as R
from mfl_amd import _lib
from test_gpu_device_round import _SPECS
from test_gpu_launch_geometry import VEC_K
from test_gpu_window import INSTANCES

F32, F64, U16 = np.float32, np.float64, np.uint16
SENTINEL = 7.0


# ---------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------
@dataclass
class Buf:
    """One buffer of a call.  ``data``: the bytes uploaded before the call (an
    output's initial content; None for a workspace, whose byte size
    ``size(libs)`` asks the library for).  ``where``: "dev", "pinned" or
    "host" (pageable numpy memory the call reads synchronously).  ``off``:
    bytes past a 256-B boundary the buffer starts at (deliberate
    misalignment).  ``ptr_of``: per element of ``data`` the name of the buffer
    whose address is added to it (None: a plain number) -- how pointer tables
    are written before any address exists.  ``dirty``: the dirty-scratch test
    may pre-fill it with 0xFF (every element is written by the call)."""
    role: str
    data: Optional[np.ndarray] = None
    where: str = "dev"
    off: int = 0
    ptr_of: Optional[List[Optional[str]]] = None
    size: Optional[Callable] = None
    inout: bool = False
    dirty: bool = True

    def __post_init__(self):
        assert self.role in ("value", "table", "out", "ws") and self.where in ("dev", "pinned", "host")
        if self.data is not None:
            self.data = np.ascontiguousarray(self.data)
        if self.ptr_of is not None:
            assert self.data.dtype == np.int64 and len(self.ptr_of) == self.data.size


def value(a, **kw): return Buf("value", a, **kw)
def table(a, **kw): return Buf("table", a, **kw)
def out(a, **kw): return Buf("out", a, **kw)
def inout(a, **kw): return Buf("out", a, inout=True, dirty=False, **kw)
def ws(size, **kw): return Buf("ws", None, size=size, **kw)
def host(a, role="table", **kw): return Buf(role, a, where="host", **kw)


@dataclass
class Inputs:
    bufs: Dict[str, Buf]
    call: Callable  # (L, a, stream) -> rc; L: the libraries, a: name -> address (a.n[name]: a workspace's bytes)
    expected: Callable  # () -> {output name: array}
    cmp: Dict[str, str]  # output name -> "bits" | "sums" | "pair32" | "between64" | "splitk" | "rel12"
    rc: int = 0
    aux: dict = field(default_factory=dict)


@dataclass
class Case:
    name: str
    entry: str  # the header's function this case stands for
    make: Callable  # rng -> Inputs
    lib: str = "main"  # "main" | "probe" | "fusedvec" | "segvec"
    sync: bool = False  # the entry waits for the stream itself
    staged: bool = False  # stages tables through host_ws / dev_ws

    def build(self, rng) -> Inputs:
        return self.make(rng)

    def expected(self, inputs: Inputs):
        return inputs.expected()

    def call(self, L, inputs: Inputs, a, stream) -> int:
        return inputs.call(L, a, stream)

    def compare(self, inputs: Inputs, got, expected):
        for name, kind in inputs.cmp.items():
            compare(kind, got[name], expected[name], f"{self.name}: {name}", inputs.aux)


def libs():
    """The four libraries, each loaded on first use."""
    return SimpleNamespace(main=_lib.load(), probe=_LazyLib(_lib.load_probe), fusedvec=_LazyLib(_lib.load_fusedvec),
                           segvec=_LazyLib(_lib.load_segvec))


class _LazyLib:
    def __init__(self, loader):
        self._loader = loader

    def __getattr__(self, name):
        return getattr(self._loader(), name)


# ---------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------
def sums_close(got, ref, what, rtol=1e-12):
    """Relative 1e-12 against the fp64 sums of the same rounded differences."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got[fin] - ref[fin])
    bad = err > rtol * np.abs(ref[fin])
    assert not bad.any(), (what, got[fin][bad][:4], ref[fin][bad][:4])


def splitk_close(got, ref, what):
    """The header's bound for fedavg_reduce_splitk_f32: norm-wise relative 1e-6."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert np.isfinite(got).all(), what
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert rel <= 1e-6, (what, rel)


def bits(x):
    """fpf_kernel_ref.bits, and plain bytes as they are."""
    x = np.asarray(x)
    return x.view(np.uint8) if x.dtype.itemsize == 1 else R.bits(x)


def compare(kind, got, want, what, aux=None):
    if kind == "bits":
        g, w = bits(got), bits(want)
        assert g.shape == w.shape, (what, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} of {g.size} differ, first at {bad[0].tolist()}"
    elif kind == "sums":
        sums_close(got, want, what)
    elif kind == "rel12":  # an fp64 A_mat (tests/test_gpu_fpf_kernels.py holds it to this)
        P = aux["P"]
        np.testing.assert_allclose(got[:P], want[:P], rtol=1e-12, atol=0.0, err_msg=what)
        assert (R.bits(got[P:]) == R.bits(want[P:])).all(), what
    elif kind == "pair32":
        ok = R.in_pair(got, want)
        assert ok.all(), (what, np.argwhere(~ok).ravel())
    elif kind == "between64":
        ok = R.between_pair(got, want)
        assert ok.all(), (what, np.argwhere(~ok).ravel())
    elif kind == "splitk":
        splitk_close(got, want, what)
    else:
        raise ValueError(kind)


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
KINDS = {"f32": (F32, 4), "f64": (F64, 8), "f16": (np.float16, 2), "bf16": (U16, 2)}


def _to_kind(vals64, kind):
    if kind == "bf16":
        return O.f32_to_bf16_bits(vals64.astype(F32))
    return vals64.astype(KINDS[kind][0])


def _as_f64(a, kind):
    return O.bf16_bits_to_f32(a).astype(F64) if kind == "bf16" else np.asarray(a).astype(F64)


def _nan_of(kind):
    return U16(0x7FC1) if kind == "bf16" else np.nan


def _rows(rng, K, P, ld, kind="f32"):
    """[K, ld] model-like rows, NaN in the padding columns."""
    x = np.full((K, ld), _nan_of(kind), dtype=KINDS[kind][0])
    x[:, :P] = _to_kind(rng.normal(0.0, 0.05, (K, P)) + rng.normal(0.0, 1e-2, (K, 1)), kind)
    return x


def _weights(rng, K):
    return O.sample_weights([int(c) for c in rng.integers(1, 1000, K)])


def _reduce(x, w, kind):
    if kind == "f32":
        return O.reduce_f32(x, w)
    if kind == "f64":
        return O.reduce_f64(x, w)
    return O.reduce_half(x, w, "float16" if kind == "f16" else "bfloat16")


def _sumsq(x, g, kind):
    """fp64 sums of the squares of the differences as the reference rounds them."""
    if kind == "f64":
        d = x - g[None, :]
    elif kind == "f32":
        d = (x - g[None, :]).astype(F32).astype(F64)
    else:
        d32 = (_as_f64(x, kind).astype(F32) - _as_f64(g, kind).astype(F32)[None, :]).astype(F32)
        d = _as_f64(_to_kind(d32.astype(F64), kind), kind)
    return (d * d).sum(axis=1)


def _w_dev(w, kind):
    return np.asarray(w, F64) if kind == "f64" else np.asarray(w, F64).astype(F32)


def _ld64(P):
    return (P + 63) // 64 * 64


# ---------------------------------------------------------------------------
# packed rows: reduce, client_sqdist, reduce_sqdist
# ---------------------------------------------------------------------------
def _reduce_rows(entry, kind, K, P, ld, *, row_off=0, out_off=0, splits=0, timed=False):
    def make(rng):
        x, w = _rows(rng, K, P, ld, kind), _weights(rng, K)
        bufs = {"clients": value(x, off=row_off), "weights": value(_w_dev(w, kind)),
                "out": out(np.full(P, SENTINEL, KINDS[kind][0]) if kind != "bf16" else np.full(P, 0x40E0, U16),
                           off=out_off)}

        def call(L, a, s):
            fn = getattr(L.main, entry)
            if splits:
                return fn(a.clients, K, P, ld, a.weights, a.out, splits, s)
            if timed:
                e0, e1 = a.events()
                return fn(a.clients, K, P, ld, a.weights, a.out, s, e0, e1)
            return fn(a.clients, K, P, ld, a.weights, a.out, s)

        return Inputs(bufs, call, lambda: {"out": _reduce(x[:, :P], w, kind)},
                      {"out": "splitk" if splits else "bits"})
    return make


def _sqdist_rows(entry, kind, K, P):
    es = KINDS[kind][1]
    ld = _ld64(P)

    def make(rng):
        x = _rows(rng, K, P, ld, kind)
        g = np.full(ld, _nan_of(kind), dtype=KINDS[kind][0])
        g[:P] = _to_kind(rng.normal(0.0, 0.05, P), kind)
        n = lambda L: (L.main.fedavg_client_sqdist_workspace(K, P) if kind == "f32" else
                       L.main.fedavg_client_sqdist_workspace_elems(K, P, es))
        bufs = {"clients": value(x), "glob": value(g), "workspace": ws(lambda L: 8 * n(L)),
                "sumsq": out(np.full(K, -1.0, F64))}
        call = lambda L, a, s: getattr(L.main, entry)(a.clients, K, P, ld, a.glob, a.workspace, a.n["workspace"] // 8,
                                                      a.sumsq, s)
        return Inputs(bufs, call, lambda: {"sumsq": _sumsq(x[:, :P], g[:P], kind)}, {"sumsq": "sums"})
    return make


def _fused_rows(entry, lib, kind, K, P, *, code=None):
    es = KINDS[kind][1]
    ld = _ld64(P)

    def make(rng):
        x, w = _rows(rng, K, P, ld, kind), _weights(rng, K)
        if code is not None:  # the probe entry has no query: the bound its own tests allocate (K x 4 x 2048 workgroups)
            n = lambda L: K * 4 * 2048
        elif kind == "f32":
            n = lambda L: L.main.fedavg_reduce_sqdist_workspace(K, P)
        else:
            n = lambda L: L.fusedvec.fedavg_reduce_sqdist_vec_workspace(K, P, es)
        bufs = {"clients": value(x), "weights": value(_w_dev(w, kind)),
                "out": out(np.zeros(P, KINDS[kind][0])), "workspace": ws(lambda L: 8 * n(L)),
                "sumsq": out(np.full(K, -1.0, F64))}

        def call(L, a, s):
            args = (a.clients, K, P, ld, a.weights, a.out, a.workspace, a.n["workspace"] // 8, a.sumsq)
            if code is not None:
                return L.probe.fedavg_reduce_sqdist_f32_variant(*args, code, 0, s)
            return getattr(getattr(L, lib), entry)(*args, s)

        def expected():
            g = _reduce(x[:, :P], w, kind)
            return {"out": g, "sumsq": _sumsq(x[:, :P], g, kind)}

        return Inputs(bufs, call, expected, {"out": "bits", "sumsq": "sums"})
    return make


# ---------------------------------------------------------------------------
# zero-copy entries: clients as separate tensors, key / pointer tables
# ---------------------------------------------------------------------------
_NP_OF = {torch.float32: F32, torch.int64: np.int64, torch.int32: np.int32, torch.bool: np.bool_}
_KIND_OF = {torch.float32: 0, torch.int64: 1, torch.int32: 2, torch.bool: 6}  # fedavg_pack_item kinds


def _spec_numels(specs):
    return [int(np.prod(shape, dtype=np.int64)) for shape, _ in specs]


def _client_blobs(rng, K, specs):
    """Per client one byte blob holding every key 16-B aligned (an empty key
    shares its neighbour's address) and the keys' byte offsets in it."""
    numels = _spec_numels(specs)
    offs, pos = [], 0
    for n, (_, dt) in zip(numels, specs):
        offs.append(pos)
        pos += (n * np.dtype(_NP_OF[dt]).itemsize + 15) // 16 * 16
    blobs, keys = [], []
    for _ in range(K):
        blob = np.zeros(max(pos, 16), np.uint8)
        vals = []
        for n, off, (_, dt) in zip(numels, offs, specs):
            if dt == torch.float32:
                v = (rng.normal(0.0, 0.05, n)).astype(F32)
            elif dt == torch.bool:
                v = rng.random(n) > 0.5
            else:
                v = rng.integers(-3000, 3000, n).astype(_NP_OF[dt])
            blob[off:off + v.nbytes] = v.view(np.uint8)
            vals.append(v)
        blobs.append(blob)
        keys.append(vals)
    return blobs, offs, keys


def _packed(keys, numels):
    """[K, P] fp32 rows: the keys cast to fp32 (ATen's static_cast) and concatenated."""
    return np.stack([np.concatenate([v.astype(F32) for v in vals]) if sum(numels) else np.zeros(0, F32)
                     for vals in keys])


def _seg_f32(entry, K, *, sums=True, round_=False):
    """The fp32 zero-copy entries on the key list of tests/test_gpu_device_round.py."""
    specs = _SPECS
    numels = _spec_numels(specs)
    n_keys, P = len(specs), sum(numels)
    numel = np.array(numels, np.int64)
    offset = np.concatenate([[0], np.cumsum(numel)[:-1]]).astype(np.int64)
    kind = np.array([_KIND_OF[dt] for _, dt in specs], np.int64)
    extra = 2 if round_ else 0  # the round's address table is wider than the group: unnamed columns hold 0

    def make(rng):
        blobs, offs, keys = _client_blobs(rng, K, specs)
        w = _weights(rng, K)
        x = _packed(keys, numels)
        bufs = {f"client{k}": value(blobs[k]) for k in range(K)}
        ptr = np.zeros((K, n_keys + extra), np.int64)
        ptr[:, :n_keys] = offs
        ptr_of = [f"client{k}" if j < n_keys else None for k in range(K) for j in range(n_keys + extra)]
        bufs["client_ptrs"] = host(ptr, ptr_of=ptr_of)
        bufs["key_numel"], bufs["key_offset"], bufs["key_kind"] = host(numel), host(offset), host(kind)
        wsq = (lambda L: L.main.fedavg_device_round_workspace(K, n_keys)) if round_ else (
            lambda L: L.main.fedavg_segments_workspace(K, n_keys))
        bufs["host_ws"], bufs["dev_ws"] = ws(wsq, where="pinned"), ws(wsq)
        glob = rng.normal(0.0, 0.05, P).astype(F32)
        cmp = {}
        if entry != "fedavg_client_sqdist_segments_f32":
            bufs["out"] = out(np.zeros(P, F32))
            cmp["out"] = "bits"
            bufs["weights"] = host(np.asarray(w, F64), role="value") if round_ else value(_w_dev(w, "f32"))
        else:
            bufs["glob"] = value(glob)
        if sums:
            bufs["sumsq"] = out(np.full(K, -1.0, F64))
            cmp["sumsq"] = "sums"
            if entry == "fedavg_client_sqdist_segments_f32":
                bufs["partials"] = ws(lambda L: 8 * L.main.fedavg_segments_partials(numel.ctypes.data, n_keys, K))
            else:
                bufs["partials"] = ws(lambda L: 8 * L.main.fedavg_reduce_sqdist_segments_partials(K))
        if round_:
            bufs["key_index"] = host(np.arange(n_keys, dtype=np.int64))
            if sums:
                bufs["int_scratch"] = ws(lambda L: 4 * L.main.fedavg_device_round_scratch(
                    numel.ctypes.data, kind.ctypes.data, n_keys, K))

        def call(L, a, s):
            tabs = (a.key_numel, a.key_offset, a.key_kind, n_keys, K)
            tail = (a.host_ws, a.dev_ws, a.n["dev_ws"], s)
            if entry == "fedavg_reduce_segments_f32":
                return L.main.fedavg_reduce_segments_f32(a.client_ptrs, *tabs, a.weights, a.out, *tail)
            if entry == "fedavg_client_sqdist_segments_f32":
                return L.main.fedavg_client_sqdist_segments_f32(a.client_ptrs, *tabs, a.glob, a.partials,
                                                                a.n["partials"] // 8, a.sumsq, *tail)
            if entry == "fedavg_reduce_sqdist_segments_f32":
                return L.main.fedavg_reduce_sqdist_segments_f32(a.client_ptrs, *tabs, a.weights, a.out, a.partials,
                                                                a.n["partials"] // 8, a.sumsq, *tail)
            if sums:
                return L.main.fedavg_device_round_f32(a.client_ptrs, n_keys + extra, a.key_index, *tabs, a.weights,
                                                      a.out, a.partials, a.n["partials"] // 8, a.sumsq,
                                                      a.int_scratch if a.n["int_scratch"] else None,
                                                      a.n["int_scratch"] // 4, *tail)
            return L.main.fedavg_device_round_f32(a.client_ptrs, n_keys + extra, a.key_index, *tabs, a.weights, a.out,
                                                  None, 0, None, None, 0, *tail)

        def expected():
            if entry == "fedavg_client_sqdist_segments_f32":
                return {"sumsq": _sumsq(x, glob, "f32")}
            g = O.reduce_f32(x, w)
            return {"out": g, "sumsq": _sumsq(x, g, "f32")} if sums else {"out": g}

        # a round without sums answers 1: only `out` was written
        return Inputs(bufs, call, expected, cmp, rc=1 if (round_ and not sums) else 0)
    return make


def _seg_vec(entry, kind, K):
    """fedavg_device_round_{f64,f16,bf16}: the fp32 keys of _SPECS as raw keys of the group's dtype."""
    es = KINDS[kind][1]
    numels = [n for n, (_, dt) in zip(_spec_numels(_SPECS), _SPECS) if dt == torch.float32]
    n_keys, P = len(numels), sum(numels)
    numel = np.array(numels, np.int64)
    offset = np.concatenate([[0], np.cumsum(numel)[:-1]]).astype(np.int64)

    def make(rng):
        offs, pos = [], 0
        for n in numels:
            offs.append(pos)
            pos += (n * es + 15) // 16 * 16
        w = _weights(rng, K)
        x = _rows(rng, K, P, P, kind)
        bufs = {}
        for k in range(K):
            blob = np.zeros(pos, np.uint8)
            for n, o, off in zip(numels, offset, offs):
                blob[off:off + n * es] = x[k, o:o + n].view(np.uint8)
            bufs[f"client{k}"] = value(blob)
        ptr = np.tile(np.array(offs, np.int64), (K, 1))
        bufs["client_ptrs"] = host(ptr, ptr_of=[f"client{k}" for k in range(K) for _ in range(n_keys)])
        bufs["key_numel"], bufs["key_offset"] = host(numel), host(offset)
        bufs["weights"] = host(np.asarray(w, F64), role="value")
        bufs["out"] = out(np.zeros(P, KINDS[kind][0]))
        bufs["partials"] = ws(lambda L: 8 * L.segvec.fedavg_device_round_vec_partials(K, es))
        bufs["sumsq"] = out(np.full(K, -1.0, F64))
        wsq = lambda L: L.segvec.fedavg_device_round_vec_workspace(K, n_keys)
        bufs["host_ws"], bufs["dev_ws"] = ws(wsq, where="pinned"), ws(wsq)
        call = lambda L, a, s: getattr(L.segvec, entry)(
            a.client_ptrs, n_keys, None, a.key_numel, a.key_offset, n_keys, K, a.weights, a.out, a.partials,
            a.n["partials"] // 8, a.sumsq, a.host_ws, a.dev_ws, a.n["dev_ws"], s)

        def expected():
            g = _reduce(x, w, kind)
            return {"out": g, "sumsq": _sumsq(x, g, kind)}

        return Inputs(bufs, call, expected, {"out": "bits", "sumsq": "sums"})
    return make


def _reduce_ptrs(K, P, offs):
    """fedavg_reduce_ptrs_f32: a DEVICE pointer table; client k starts offs[k % len] bytes into its buffer."""
    def make(rng):
        x, w = _rows(rng, K, P, P), _weights(rng, K)
        bufs = {f"client{k}": value(x[k], off=offs[k % len(offs)]) for k in range(K)}
        bufs["client_ptrs"] = table(np.zeros(K, np.int64), ptr_of=[f"client{k}" for k in range(K)])
        bufs["weights"], bufs["out"] = value(_w_dev(w, "f32")), out(np.zeros(P, F32))
        call = lambda L, a, s: L.main.fedavg_reduce_ptrs_f32(a.client_ptrs, K, P, a.weights, a.out, s)
        return Inputs(bufs, call, lambda: {"out": O.reduce_f32(x, w)}, {"out": "bits"})
    return make


def _pack_device(es):
    """fedavg_pack_rows_device: 3 clients x 4 keys into [3, ld] rows; element
    size 4 carries the integer kinds."""
    np_t = {4: F32, 2: np.float16, 8: F64}[es]
    if es == 4:
        keys = [(37, F32, 0), (1, np.int64, 1), (5, np.int32, 2), (3, np.int16, 3), (6, np.int8, 4), (9, np.uint8, 5),
                (10, np.bool_, 6), (1030, F32, 0)]
    else:
        keys = [(37, np_t, 0), (1, np_t, 0), (1030, np_t, 0)]
    K = 3
    P = sum(n for n, _, _ in keys)
    ld = P + 3

    def make(rng):
        bufs, items, ptr_of, want = {}, [], [], np.full((K, ld), SENTINEL, np_t)
        for k in range(K):
            col = 0
            for j, (n, t, kind) in enumerate(keys):
                if t in (F32, F64, np.float16):
                    v = rng.normal(0.0, 0.05, n).astype(t)
                elif t == np.bool_:
                    v = rng.random(n) > 0.5
                else:
                    v = rng.integers(0 if t == np.uint8 else -100, 100, n).astype(t)
                bufs[f"src{k}_{j}"] = value(v)
                items.append([0, n, k * ld + col, kind])
                ptr_of += [f"src{k}_{j}", None, None, None]
                want[k, col:col + n] = v.astype(np_t)
                col += n
        bufs["items"] = host(np.array(items, np.int64), ptr_of=ptr_of)
        bufs["dst"] = inout(np.full((K, ld), SENTINEL, np_t))
        wsq = lambda L: L.main.fedavg_pack_rows_device_workspace(len(items))
        bufs["host_ws"], bufs["dev_ws"] = ws(wsq, where="pinned"), ws(wsq)
        call = lambda L, a, s: L.main.fedavg_pack_rows_device(a.items, len(items), a.dst, es, a.host_ws, a.dev_ws,
                                                              a.n["dev_ws"], s)
        return Inputs(bufs, call, lambda: {"dst": want}, {"dst": "bits"})
    return make


def _round_f32():
    """fedavg_round_f32 (synchronous): host items -> pinned rows -> one kernel."""
    K = 5
    numels = [2000, 1, 51]
    P = ld = sum(numels)  # no padding columns: the call writes every element of host_rows (on the host) and dev_rows

    def make(rng):
        w = _weights(rng, K)
        bufs, items, ptr_of, x = {}, [], [], np.zeros((K, P), F32)
        for k in range(K):
            col = 0
            for j, n in enumerate(numels):
                v = rng.integers(-3000, 3000, n) if n == 1 else rng.normal(0.0, 0.05, n).astype(F32)
                bufs[f"src{k}_{j}"] = host(v, role="value")
                items.append([0, n, k * ld + col, 1 if n == 1 else 0])
                ptr_of += [f"src{k}_{j}", None, None, None]
                x[k, col:col + n] = v.astype(F32)
                col += n
        rows = np.zeros((K, ld), F32)
        rows[:, :P] = x
        bufs["items"] = host(np.array(items, np.int64), ptr_of=ptr_of)
        bufs["weights"] = host(np.asarray(w, F64), role="value")
        bufs["host_rows"] = out(np.zeros((K, ld), F32), where="pinned")
        bufs["dev_rows"] = out(np.zeros((K, ld), F32))
        bufs["host_w"], bufs["dev_w"] = out(np.zeros(K, F32), where="pinned"), out(np.zeros(K, F32))
        bufs["dev_out"], bufs["host_out"] = out(np.zeros(P, F32)), out(np.zeros(P, F32), where="pinned")
        call = lambda L, a, s: L.main.fedavg_round_f32(a.items, len(items), a.host_rows, a.dev_rows, K, P, ld,
                                                       a.weights, a.host_w, a.dev_w, a.dev_out, a.host_out, 2, s)

        def expected():
            g, w32 = O.reduce_f32(x, w), _w_dev(w, "f32")
            return {"host_rows": rows, "dev_rows": rows, "host_w": w32, "dev_w": w32, "dev_out": g, "host_out": g}

        return Inputs(bufs, call, expected, {n: "bits" for n in ("host_rows", "dev_rows", "host_w", "dev_w", "dev_out",
                                                                 "host_out")})
    return make


# ---------------------------------------------------------------------------
# FPF2
# ---------------------------------------------------------------------------
def _n_rows(P):
    """fpf_kernel_ref.n_rows_for at its edge shapes, its largest row count at any other P."""
    return R.n_rows_for(P) if P in R.P_EDGE else R.N_ROWS[-1]


def _a_padded(a, ld):
    o = np.zeros(ld, F32)
    o.view(np.uint32)[:] = R.PAD_A
    o[:a.size] = a
    return o


def _fpf_set_rows(P):
    n, ld = _n_rows(P), R.round4(P) + 8

    def make(rng):
        diffs, _, last_w, _ = R.state_f32(P, n, int(rng.integers(1 << 20)))
        K = min(n, 3)
        idx = [-1] + rng.permutation(n)[:K].tolist() + [n]  # out-of-range entries are skipped
        rows = R.padded((last_w + rng.normal(0.0, 1e-2, (len(idx), P))).astype(F32), ld + 4, np.nan)
        lw, d0 = R.padded(last_w, ld, np.nan), R.padded(diffs, ld, R.PAD_D)
        bufs = {"diffs": inout(d0), "row_idx": table(np.array(idx, np.int64)), "rows": value(rows), "last_w": value(lw)}
        call = lambda L, a, s: L.main.fedavg_fpf_set_rows_f32(a.diffs, n, ld, a.row_idx, len(idx), a.rows, ld + 4,
                                                              a.last_w, P, s)
        return Inputs(bufs, call, lambda: {"diffs": R.set_rows(d0, idx, rows, lw, P)}, {"diffs": "bits"})
    return make


def _draw_state(rng, P, n, T=torch.float32):
    """state_f32 on a seed whose mean is decided in T (fpf_kernel_ref.mean_is_unambiguous)."""
    for _ in range(50):
        st = R.state_f32(P, n, int(rng.integers(1 << 20)))
        if R.mean_is_unambiguous(T, R.gdiff_f32(st[3], st[2])):
            return st
    raise AssertionError("no unambiguous mean in 50 draws")


def _fpf_end_round(P):
    n, ld = _n_rows(P), R.round4(P) + 8

    def make(rng):
        diffs, a, last_w, w_glob = _draw_state(rng, P, n)
        mean = R.mean_as(torch.float32, R.gdiff_f32(w_glob, last_w))
        keep = R.keep_form("alt", n)
        d0, a0 = R.padded(diffs, ld, R.PAD_D), _a_padded(a, ld)
        bufs = {"diffs": inout(d0), "keep_rows": table(keep), "a_mat": inout(a0),
                "w_glob": value(R.padded(w_glob, ld, np.nan)), "last_w": value(R.padded(last_w, ld, np.nan)),
                "workspace": ws(lambda L: 8 * L.main.fedavg_fpf_workspace(P))}
        call = lambda L, a_, s: L.main.fedavg_fpf_end_round_f32(a_.diffs, n, ld, a_.keep_rows, a_.a_mat, a_.w_glob,
                                                                a_.last_w, P, 2.0, a_.workspace,
                                                                a_.n["workspace"] // 8, s)

        def expected():
            d, am = R.end_round_f32(d0, keep, a0, w_glob, last_w, P, 2.0, mean)
            return {"diffs": d, "a_mat": am}

        return Inputs(bufs, call, expected, {"diffs": "bits", "a_mat": "bits"})
    return make


def _fpf_update_g(n):
    def make(rng):
        G0 = rng.uniform(0.0, 5.0, n).astype(F32)
        itr0, lru0 = rng.integers(0, 9, n).astype(F32), rng.integers(0, 40, n).astype(F32)
        sel = (rng.random(n) > 0.5).astype(np.uint8)
        bufs = {"g_mat": inout(G0), "itr_row": inout(itr0), "lru_itr": inout(lru0), "selected": table(sel)}
        call = lambda L, a, s: L.main.fedavg_fpf_update_g(a.g_mat, a.itr_row, a.lru_itr, a.selected, n, 3.0, 1, 2.0, s)

        def expected():
            G, it, lru = R.update_g(G0, itr0, lru0, sel, 3.0, 1, 2.0)
            return {"g_mat": G, "itr_row": it, "lru_itr": lru}

        return Inputs(bufs, call, expected, {"g_mat": "bits", "itr_row": "bits", "lru_itr": "bits"})
    return make


def _fpf_index(P, f64):
    n, ld = _n_rows(P), R.round4(P) + 8

    def make(rng):
        diffs, a, G = R.index_state(P, n, int(rng.integers(1 << 20)))
        m = len(G)
        if f64:
            a = a.astype(F64) * (1.0 + 2.0 ** -30)
        bufs = {"diffs": value(R.padded(diffs, ld, np.nan)),
                "a_mat": value(R.padded(a, ld, np.nan) if f64 else _a_padded(a, ld)), "g_mat": value(G),
                "fpf": out(np.full(m, -7.0, F64 if f64 else F32))}
        fn = "fedavg_fpf_index_f64" if f64 else "fedavg_fpf_index_f32"
        call = lambda L, a_, s: getattr(L.main, fn)(a_.diffs, m, ld, P, a_.a_mat, a_.g_mat, a_.fpf, s)
        exp = lambda: {"fpf": (R.index_f64 if f64 else R.index_f32)(diffs, a, G, P)}
        return Inputs(bufs, call, exp, {"fpf": "between64" if f64 else "pair32"})
    return make


def _fpf_index_lru(n):
    def make(rng):
        lru, G = rng.integers(0, 40, n).astype(F32), rng.uniform(0.1, 5.0, n).astype(F32)
        G[0], lru[n - 1] = 0.0, np.nan
        bufs = {"lru_itr": value(lru), "g_mat": value(G), "fpf": out(np.full(n, -7.0, F32))}
        call = lambda L, a, s: L.main.fedavg_fpf_index_lru(a.lru_itr, a.g_mat, n, a.fpf, s)
        return Inputs(bufs, call, lambda: {"fpf": R.index_lru(lru, G)}, {"fpf": "bits"})
    return make


def _fpf_cat_diff(P, out_f64):
    """Three keys in two dtype groups (fp32, fp16) of P columns in all."""
    n, K = _n_rows(P), min(_n_rows(P), 3)
    numels = [1, P - 2, 1] if P >= 4 else [P]
    kinds = [0, 2, 0] if P >= 4 else [0]
    ld_out = P + 3

    def make(rng):
        keys, goff, cat = [], {0: 0, 2: 0}, 0
        order = sorted(set(kinds))
        for numel, kind in zip(numels, kinds):
            keys.append((numel, cat, order.index(kind), goff[kind], 0))
            cat += numel
            goff[kind] += numel
        cur, last, bufs = {}, {}, {}
        for g, kind in enumerate(order):
            T, ldg = R.KIND_DTYPE[kind], goff[kind] + 5
            last[g] = torch.from_numpy(rng.normal(0.0, 1.0, ldg)).to(T)
            cur[g] = (last[g].to(torch.float64) + torch.from_numpy(rng.normal(0.0, 0.1, (K, ldg)))).to(T)
            view = (lambda t: t.view(torch.int16).numpy().view(U16) if t.element_size() == 2 else t.numpy())
            bufs[f"cur{g}"], bufs[f"last{g}"] = value(view(cur[g])), value(view(last[g]))
        idx = [n - 1, -1, 0][:K]
        init = np.full((n, ld_out), 123.0, F64 if out_f64 else F32)
        bufs["keys"], bufs["row_idx"] = table(np.array(keys, np.int64)), table(np.array(idx, np.int64))
        bufs["out"] = inout(init)

        def call(L, a, s):
            cg, lg = _lib.FpfGroups(), _lib.FpfGroups()
            for g, kind in enumerate(order):
                cg.base[g], cg.ld[g], cg.kind[g] = a[f"cur{g}"], cur[g].shape[1], kind
                lg.base[g], lg.ld[g], lg.kind[g] = a[f"last{g}"], last[g].shape[0], kind
            return L.main.fedavg_fpf_cat_diff(a.keys, len(keys), P, ctypes.addressof(cg), K, ctypes.addressof(lg),
                                              a.row_idx, n, a.out, ld_out, int(out_f64), s)

        def expected():
            ref, want = R.cat_diff(keys, cur, last, K, out_f64), init.copy()
            for k, r in enumerate(idx):
                if 0 <= r < n:
                    want[r, :P] = ref[k]
            return {"out": want}

        return Inputs(bufs, call, expected, {"out": "bits"})
    return make


def _fpf_end_round_promoted(P, t_kind):
    n, ld = _n_rows(P), R.round4(P) + 8
    f64 = t_kind in (1, 4)
    T = torch.float64 if f64 else R.KIND_DTYPE[t_kind]

    def make(rng):
        for _ in range(50):
            gd = R.gdiff_T(P, t_kind, int(rng.integers(1 << 20)))
            if f64 or R.mean_is_unambiguous(T, gd):
                break
        else:
            raise AssertionError("no unambiguous mean in 50 draws")
        mean = R.mean_as(T, gd)
        diffs = rng.normal(0.0, 1e-3, (n, P)).astype(F32)
        a = rng.uniform(0.5, 1.5, P).astype(F32)
        keep = R.keep_form("alt", n)
        d0 = R.padded(diffs, ld, R.PAD_D)
        a0 = R.padded(a.astype(F64) * ((1.0 + 2.0 ** -30) if t_kind == 1 else 1.0), ld, np.nan) if f64 else \
            _a_padded(a, ld)
        bufs = {"diffs": inout(d0), "keep_rows": table(keep), "a_mat": inout(a0),
                "gdiff": value(R.padded(gd, ld, np.nan)), "workspace": ws(lambda L: 8 * L.main.fedavg_fpf_workspace(P))}
        call = lambda L, a_, s: L.main.fedavg_fpf_end_round_promoted(a_.diffs, n, ld, a_.keep_rows, a_.a_mat, a_.gdiff,
                                                                     P, t_kind, 2.0, a_.workspace,
                                                                     a_.n["workspace"] // 8, s)

        def expected():
            d, am = R.end_round_promoted(d0, keep, a0, gd, P, t_kind, 2.0, mean)
            return {"diffs": d, "a_mat": am}

        return Inputs(bufs, call, expected, {"diffs": "bits", "a_mat": "rel12" if f64 else "bits"}, aux={"P": P})
    return make


# ---------------------------------------------------------------------------
# client statistics, transfers
# ---------------------------------------------------------------------------
def _client_stats(has_snap, misaligned):
    numels = [37, 4, 1030, 1]
    numel = np.array(numels, np.int64)
    padded = (numel + 3) // 4 * 4
    offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    P, n = int(padded.sum()), len(numels)

    def make(rng):
        prev = [rng.normal(0.0, 0.05, m).astype(F32) for m in numels]
        cur = [(p + 1e-3 * rng.normal(0.0, 1.0, p.size)).astype(F32) for p in prev]
        snap0 = np.full(P, 123.0, F32)
        want = snap0.copy()
        for p, c, o in zip(prev, cur, offset):
            if has_snap:
                snap0[o:o + p.size] = p
            want[o:o + c.size] = c
        bufs = {f"cur{j}": value(c, off=4 if (misaligned and j == 2) else 0) for j, c in enumerate(cur)}
        bufs["cur_ptrs"] = host(np.zeros(n, np.int64), ptr_of=[f"cur{j}" for j in range(n)])
        bufs["key_numel"], bufs["key_offset"] = host(numel), host(offset)
        bufs["snap"] = inout(snap0)
        bufs["partials"] = ws(lambda L: 8 * L.main.fedavg_client_stats_partials(numel.ctypes.data, n))
        bufs["stats"] = out(np.full(4, -7.0, F64))
        wsq = lambda L: L.main.fedavg_client_stats_workspace(n)
        bufs["host_ws"], bufs["dev_ws"] = ws(wsq, where="pinned"), ws(wsq)
        call = lambda L, a, s: L.main.fedavg_client_stats_f32(a.cur_ptrs, a.key_numel, a.key_offset, n, a.snap, P,
                                                              has_snap, a.partials, a.n["partials"] // 8, a.stats,
                                                              a.host_ws, a.dev_ws, a.n["dev_ws"], s)

        def expected():
            nan_count, s_cur, s_d = CS.record(np.concatenate(cur), np.concatenate(prev) if has_snap else None)
            return {"snap": want, "stats": np.array([nan_count, s_cur, s_d, 0.0])}

        return Inputs(bufs, call, expected, {"snap": "bits", "stats": "sums"})
    return make


def _client_track():
    def make(rng):
        sw, sg, dl = float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.1, 1.0))
        bufs = {"state": inout(np.zeros(4, F64)), "w_stats": value(np.array([0.0, 1.0, sw, 0.0])),
                "g_stats": value(np.array([0.0, 1.0, sg, 0.0]))}
        call = lambda L, a, s: L.main.fedavg_client_track(a.state, a.w_stats, a.g_stats, dl, s)

        def expected():
            t = CS.Track()
            t.step(sw, sg, dl)
            return {"state": np.array([float(t.rho), float(t.beta), 1.0, 1.0])}

        return Inputs(bufs, call, expected, {"state": "bits"})
    return make


def _copy_to_host(blocks, nbytes=4112):
    def make(rng):
        src = rng.integers(0, 256, nbytes).astype(np.uint8)
        bufs = {"src": value(src), "host_dst": out(np.zeros(nbytes, np.uint8), where="pinned")}
        call = lambda L, a, s: L.main.fedavg_copy_to_host(a.src, a.host_dst, nbytes, blocks, s)
        return Inputs(bufs, call, lambda: {"host_dst": src}, {"host_dst": "bits"})
    return make


def _upload_shard():
    rows, width, spitch, dpitch = 7, 400, 1000, 528  # floats: the shard is 400 of the buffer's 1000 columns

    def make(rng):
        src = rng.normal(0.0, 0.05, (rows, spitch)).astype(F32)
        want = np.full((rows, dpitch), SENTINEL, F32)
        want[:, :width] = src[:, 200:200 + width]
        bufs = {"host_src": value(src, where="pinned"), "dst": inout(np.full((rows, dpitch), SENTINEL, F32))}
        call = lambda L, a, s: L.main.fedavg_upload_shard(a.dst, dpitch * 4, a.host_src + 800, spitch * 4, width * 4,
                                                          rows, s)
        return Inputs(bufs, call, lambda: {"dst": want}, {"dst": "bits"})
    return make


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def multi_launch_P(K=2):
    """The smallest P = 2^n + 3 <= 64M at K clients for which
    fedavg_f32_schedule reports launches >= 2 (None: no such P).  At K = 2
    there is none: up to 4 clients always take one launch."""
    for e in range(2, 27):
        P = (1 << e) + 3
        if P <= 64 * (1 << 20) and _lib.f32_schedule(K, P)["launches"] >= 2:
            return P
    return None


# a round-split shape of fedavg_reduce_f32: 5 clients on rows just past 768 workgroups of 256 float4 columns, where
# the global-pointer kernel runs in launches of 3 workgroups per CU (tests/test_abi_cases.py holds the schedule to it)
MULTI_LAUNCH = (5, 768 * 256 * 4 + 1024 + 7)


FUSED_K = (1, 5, 16, 17, 64, 65, 128, 129, 320, 369, 513, 1024, 1025)
FUSED_P = (3, 12_345)
VEC_MAX_K = {"f64": 64, "f16": 128, "bf16": 128}  # the largest fused K of each dtype


def _cases():
    c = []
    add = lambda name, entry, make, **kw: c.append(Case(name, entry, make, **kw))
    r = "fedavg_reduce_f32"
    add("reduce_f32-aligned-3x4097", r, _reduce_rows(r, "f32", 3, 4097, _ld64(4097)))
    add("reduce_f32-17x65", r, _reduce_rows(r, "f32", 17, 65, 68))
    add("reduce_f32-scalar-5x4099", r, _reduce_rows(r, "f32", 5, 4099, 4101, row_off=4, out_off=4))
    mk, mp = MULTI_LAUNCH
    add(f"reduce_f32-multilaunch-{mk}x{mp}", r, _reduce_rows(r, "f32", mk, mp, _ld64(mp)))
    add("reduce_f32_timed-17x4097", "fedavg_reduce_f32_timed",
        _reduce_rows("fedavg_reduce_f32_timed", "f32", 17, 4097, _ld64(4097), timed=True))
    add("reduce_ptrs-2x4096", "fedavg_reduce_ptrs_f32", _reduce_ptrs(2, 4096, [0]))
    add("reduce_ptrs-4x4097-mixed", "fedavg_reduce_ptrs_f32", _reduce_ptrs(4, 4097, [0, 4, 8, 12]))
    for kind in ("f64", "f16", "bf16"):
        e = f"fedavg_reduce_{kind}"
        ldq = 16 // KINDS[kind][1]
        for K, P in ((3, 70), (10, 4099)):
            add(f"reduce_{kind}-{K}x{P}", e, _reduce_rows(e, kind, K, P, (P + ldq - 1) // ldq * ldq + ldq))
    for splits in (2, 4, 8):
        add(f"splitk-{splits}", "fedavg_reduce_splitk_f32",
            _reduce_rows("fedavg_reduce_splitk_f32", "f32", 10, 7850, 7852, splits=splits))
    for kind in ("f32", "f64", "f16", "bf16"):
        e = f"fedavg_client_sqdist_{kind}"
        add(f"client_sqdist_{kind}-7x4099", e, _sqdist_rows(e, kind, 7, 4099))
    e = "fedavg_reduce_sqdist_f32"
    for K in FUSED_K:
        for P in FUSED_P:
            add(f"reduce_sqdist_f32-{K}x{P}", e, _fused_rows(e, "main", "f32", K, P))
    for kmax, vec in INSTANCES:
        add(f"reduce_sqdist_f32-window-{kmax}x{vec}", e,
            _fused_rows(e, "probe", "f32", kmax - 1, 64 * vec + 5, code=70000000 + kmax * 100 + 40 + vec), lib="probe")
    for K, code in ((65, 91000808), (513, 91001616)):
        add(f"reduce_sqdist_f32-handoff-{code}", e, _fused_rows(e, "probe", "f32", K, 67, code=code), lib="probe")
    for kind in ("f64", "f16", "bf16"):
        e = f"fedavg_reduce_sqdist_{kind}"
        for K in VEC_K:
            add(f"reduce_sqdist_{kind}-{K}x4099", e, _fused_rows(e, "fusedvec", kind, K, 4099), lib="fusedvec")
    for K in (5, 100, 300):
        for e in ("fedavg_reduce_segments_f32", "fedavg_client_sqdist_segments_f32"):
            add(f"{e[7:]}-K{K}", e, _seg_f32(e, K, sums=e != "fedavg_reduce_segments_f32"), staged=True)
        if K <= 256:  # the fused segments entry takes 1..256 clients
            e = "fedavg_reduce_sqdist_segments_f32"
            add(f"{e[7:]}-K{K}", e, _seg_f32(e, K), staged=True)
        e = "fedavg_device_round_f32"
        add(f"device_round_f32-sums-K{K}", e, _seg_f32(e, K, round_=True), staged=True)
        add(f"device_round_f32-reduce-K{K}", e, _seg_f32(e, K, sums=False, round_=True), staged=True)
    for kind in ("f64", "f16", "bf16"):
        e = f"fedavg_device_round_{kind}"
        for K in (5, VEC_MAX_K[kind]):
            add(f"device_round_{kind}-K{K}", e, _seg_vec(e, kind, K), lib="segvec", staged=True)
    for es in (4, 2, 8):
        add(f"pack_rows_device-es{es}", "fedavg_pack_rows_device", _pack_device(es), staged=True)
    add("round_f32", "fedavg_round_f32", _round_f32(), sync=True)
    for P in (5, 4099):
        add(f"fpf_set_rows-{P}", "fedavg_fpf_set_rows_f32", _fpf_set_rows(P))
        add(f"fpf_end_round-{P}", "fedavg_fpf_end_round_f32", _fpf_end_round(P))
        add(f"fpf_index_f32-{P}", "fedavg_fpf_index_f32", _fpf_index(P, False))
        add(f"fpf_index_f64-{P}", "fedavg_fpf_index_f64", _fpf_index(P, True))
        for f64 in (0, 1):
            add(f"fpf_cat_diff-{P}-f64_{f64}", "fedavg_fpf_cat_diff", _fpf_cat_diff(P, bool(f64)))
        for t_kind in range(5):
            add(f"fpf_end_round_promoted-{P}-t{t_kind}", "fedavg_fpf_end_round_promoted",
                _fpf_end_round_promoted(P, t_kind))
        n = _n_rows(P)
        add(f"fpf_update_g-{n}", "fedavg_fpf_update_g", _fpf_update_g(n))
        add(f"fpf_index_lru-{n}", "fedavg_fpf_index_lru", _fpf_index_lru(n))
    add("client_stats-first", "fedavg_client_stats_f32", _client_stats(0, False), staged=True)
    add("client_stats-snap", "fedavg_client_stats_f32", _client_stats(1, False), staged=True)
    add("client_stats-snap-misaligned", "fedavg_client_stats_f32", _client_stats(1, True), staged=True)
    add("client_track", "fedavg_client_track", _client_track())
    for blocks in (0, 8):
        add(f"copy_to_host-blocks{blocks}", "fedavg_copy_to_host", _copy_to_host(blocks))
    add("upload_shard-7rows", "fedavg_upload_shard", _upload_shard())
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
