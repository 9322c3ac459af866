"""GPU parity of the zero-copy device round for fp64 / fp16 / bf16 groups
(fedavg_device_round_{f64,f16,bf16}, libfedavg_amd_segvec.so) and of the
drop-in route that uses it.

Expected values come from code the library does not share: ``out`` must carry
the bits of ``mfl_amd.reduce_packed`` on rows packed from the same tensors and
of the CPU oracle's chain (NaN positions compared, payloads not); ``sumsq``
is held to the bound tests/test_gpu_fused_vec.py derives -- the 16-bit
squares are exact in fp64 and the fp64 ones carry one fma rounding each, and
two fixed summation orders of P non-negative terms each sit within
(P - 1) * 2^-53 of the exact sum, so any two of {this pass, client_sqdist,
math.fsum of the oracle's rounded differences squared} differ by at most
2 (P + 1) 2^-53 relative.
"""
import copy
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fedavg_oracle as O
import mfl_amd
from mfl_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [torch.float64, torch.float16, torch.bfloat16]
IDS = lambda d: str(d).split(".")[-1]  # noqa: E731
ENTRY = {torch.float64: "fedavg_device_round_f64", torch.float16: "fedavg_device_round_f16",
         torch.bfloat16: "fedavg_device_round_bf16"}
MAX_K = {torch.float64: 64, torch.float16: 128, torch.bfloat16: 128}
SENTINEL = 7.0


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_available):
    _lib.load_segvec()
    torch.cuda.set_device(DEV)
    yield


def _es(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _bound(P):
    return 2 * (P + 1) * 2.0 ** -53


def _plan(dtype, K):
    """(KMAX, slice bytes, window columns) of K clients, from the library."""
    code = _lib.load_segvec().fedavg_device_round_vec_plan_of(K, _es(dtype), int(dtype == torch.bfloat16))
    assert code // 1_000_000 == 3, (dtype, K, code)
    kmax, sb = code // 100 % 10_000, code % 100
    return kmax, sb, 64 * sb // _es(dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()]).numpy()


def _oracle_out(h, weights):
    """The oracle's chain on packed CPU rows [K, P] (its own representation)."""
    if h.dtype == torch.float64:
        return O.reduce_f64(h.numpy(), weights)
    if h.dtype == torch.float16:
        return O.reduce_half(h.numpy(), weights, "float16")
    return O.reduce_half(h.contiguous().view(torch.int16).numpy().view(np.uint16), weights, "bfloat16")


def _same_bits_or_nan(got, exp_arr):
    """Bit equality; NaN payloads are not compared, NaN positions are."""
    if got.dtype == torch.bfloat16:
        g = O.bf16_bits_to_f32(got.cpu().contiguous().view(torch.int16).numpy().view(np.uint16))
        e = O.bf16_bits_to_f32(exp_arr)
    else:
        g, e = got.cpu().numpy(), exp_arr
    gn, en = np.isnan(g), np.isnan(e)
    assert np.array_equal(gn, en)
    assert g[~gn].tobytes() == e[~en].tobytes()


def _oracle_sumsq(h, g):
    """math.fsum of the oracle's rounded differences squared, per client (CPU tensors)."""
    if h.dtype == torch.float64:
        with np.errstate(invalid="ignore"):  # inf - inf where a test plants them: NaN, as on the device
            d = h.numpy() - g.numpy()[None, :]
    else:
        d = (h.float() - g.float()[None, :]).to(h.dtype).double().numpy()  # rh(f32(x) - f32(g)), widened exactly
    return [math.fsum((row * row).tolist()) for row in d]


def _check_sums(got, ref, P, what):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what
    fin = ~(nan | inf)
    err = np.abs(got[fin] - ref[fin])
    rel = err / np.maximum(np.abs(ref[fin]), 1e-300)
    rel[err == 0] = 0.0
    print(f"{what}: max relative distance {rel.max() if rel.size else 0.0:.3e} (bound {_bound(P):.3e})")
    assert (rel <= _bound(P)).all(), (what, float(rel.max()), _bound(P))


class _Round:
    """K clients' keys as 16-B aligned views into ONE NaN-filled device arena,
    at least 16 B of NaN between any two keys (an over-read or a padding leak
    shows as NaN), keys back to back in the output as layout.KeyTable lays
    them; the same values packed into [K, ld] rows with NaN padding."""

    def __init__(self, dtype, K, numels, seed, packed=None):
        self.dtype, self.K, self.numels = dtype, K, [int(n) for n in numels]
        es = self.es = _es(dtype)
        self.P = P = sum(self.numels)
        g = torch.Generator().manual_seed(seed)
        if packed is None:
            packed = (torch.randn((K, P), generator=g, dtype=torch.float64) * 0.05
                      + torch.randn((K, 1), generator=g, dtype=torch.float64) * 1e-2).to(dtype)
        self.packed = packed  # CPU [K, P]
        counts = torch.randint(1, 1000, (K,), generator=g).tolist()
        self.weights = mfl_amd.sample_weights(counts)
        per16 = 16 // es
        starts, pos = [], per16  # a key starts on a 16-B multiple, 16..31 B of NaN after the previous key's end
        for n in self.numels:
            starts.append(pos)
            pos = (pos + n + per16 - 1) // per16 * per16 + per16
        self.A = A = pos + per16
        self.starts = np.array(starts, dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.numels)[:-1]]).astype(np.int64)
        cols = (np.concatenate([s + np.arange(n) for s, n in zip(starts, self.numels)]).astype(np.int64)
                if P else np.zeros(0, np.int64))
        arena = torch.full((K, A), float("nan"), dtype=dtype)
        arena[:, torch.from_numpy(cols)] = packed
        self.arena = arena.to(DEV)
        assert self.arena.data_ptr() % 16 == 0 and (A * es) % 16 == 0
        base = self.arena.data_ptr()
        self.ptrs = (base + (np.arange(K, dtype=np.int64)[:, None] * A + self.starts[None, :]) * es).astype(np.int64)
        self.ld = ld = (P + 63) // 64 * 64 + 64
        rows = torch.full((K, ld), float("nan"), dtype=dtype)
        rows[:, :P] = packed
        self.rows = rows.to(DEV)

    def call(self, out=None, ptrs=None, expect=0):
        """The C ABI call; returns (out, sumsq) with out sized past P and pre-filled with a sentinel."""
        lib = _lib.load_segvec()
        K, n = self.K, len(self.numels)
        if out is None:
            out = torch.full((self.P + 67,), SENTINEL, dtype=self.dtype, device=DEV)
        ptrs = np.ascontiguousarray(self.ptrs if ptrs is None else ptrs, dtype=np.int64)
        numel = np.array(self.numels, dtype=np.int64)
        w64 = np.array(self.weights, dtype=np.float64)
        n_part = lib.fedavg_device_round_vec_partials(K, self.es)
        partials = torch.empty(max(n_part, 1), dtype=torch.float64, device=DEV)
        sumsq = torch.full((K,), -1.0, dtype=torch.float64, device=DEV)
        need = lib.fedavg_device_round_vec_workspace(K, n)
        host_ws = torch.empty(need, dtype=torch.uint8, pin_memory=True)
        dev_ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        rc = getattr(lib, ENTRY[self.dtype])(ptrs.ctypes.data, n, None, numel.ctypes.data, self.offsets.ctypes.data, n,
                                             K, w64.ctypes.data, out.data_ptr(), partials.data_ptr(), n_part,
                                             sumsq.data_ptr(), host_ws.data_ptr(), dev_ws.data_ptr(), need,
                                             torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        assert rc == expect, (rc, lib.fedavg_segvec_last_error())
        return out, sumsq

    def check(self, what, oracle=True):
        """out against reduce_packed (and the oracle), the sentinel outside the
        keys, sumsq against client_sqdist and fsum, and a second call's bits."""
        P = self.P
        out, sumsq = self.call()
        w = mfl_amd.weights_tensor(self.weights, self.dtype, DEV)
        two = mfl_amd.reduce_packed(self.rows, w, P)
        on, tn = torch.isnan(out[:P]), torch.isnan(two[:P])
        assert torch.equal(on, tn), what
        assert np.array_equal(_bits(out[:P][~on]), _bits(two[:P][~tn])), what
        assert bool((out[P:] == SENTINEL).all()), what  # nothing written outside the keys
        if oracle:
            _same_bits_or_nan(out[:P], _oracle_out(self.packed, self.weights))
        alone = mfl_amd.client_sqdist(self.rows, two, P)
        _check_sums(sumsq.cpu().numpy(), alone.cpu().numpy(), P, f"{what} vs client_sqdist")
        if oracle:
            _check_sums(sumsq.cpu().numpy(), _oracle_sumsq(self.packed, out[:P].cpu()), P, f"{what} vs fsum")
        again = self.call()[1]
        assert np.array_equal(_bits(sumsq), _bits(again)), what  # deterministic, NaN sums included
        return out, sumsq


def _edge_ks(dtype):
    return [1, 2, 16, 17, 32, 33, 64] + ([] if dtype == torch.float64 else [65, 100, 101, 128])


@pytest.mark.parametrize("dtype,K", [(d, K) for d in DTYPES for K in _edge_ks(d)],
                         ids=lambda v: IDS(v) if isinstance(v, torch.dtype) else str(v))
def test_band_edges_and_window_tails(dtype, K):
    """Every band edge; keys of 0, 1, 7, WC-1, WC, WC+1, 2 WC+3 and 3 elements
    in that order: ragged and full windows, and later keys at output offsets
    that are no multiple of 4 B or 16 B (the guarded element stores)."""
    _, _, WC = _plan(dtype, K)
    numels = [0, 1, 7, WC - 1, WC, WC + 1, 2 * WC + 3, 3]
    r = _Round(dtype, K, numels, K * 1009 + _es(dtype))
    assert any((o * r.es) % 4 for o in r.offsets) or r.es == 8
    assert any((o * r.es) % 16 for o in r.offsets)
    out, sumsq = r.check(f"{dtype} K={K}")
    assert bool(torch.isfinite(sumsq).all()) and bool(torch.isfinite(out[:r.P].double()).all())  # no NaN leaked in


@pytest.mark.parametrize("K", [5, 40])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nonfinite_and_subnormal_columns(dtype, K):
    """NaN / +-inf / subnormals in single clients' keys, at a key's first and
    last element: the NaN (and inf) positions of out and sumsq equal the packed
    route's and the CPU oracle's, finite sums stay within the bound."""
    tiny = {torch.float64: 5e-324, torch.float16: 6e-8, torch.bfloat16: 9.2e-41}[dtype]
    specials = [float("nan"), float("inf"), float("-inf"), tiny, -tiny]
    numels = [300, 1, 77, 0, 515]
    P = sum(numels)
    first = np.concatenate([[0], np.cumsum(numels)[:-1]])
    for n_special in (1, 3, 5):
        g = torch.Generator().manual_seed(K * 31 + n_special)
        packed = (torch.randn((K, P), generator=g, dtype=torch.float64) * 0.05).to(dtype)
        live = [j for j, n in enumerate(numels) if n]
        for s in range(n_special):
            j = live[s % len(live)]
            col = int(first[j]) if s % 2 == 0 else int(first[j]) + numels[j] - 1  # the key's first / last element
            packed[(s * 7 + 1) % K, col] = specials[s]
        packed[K - 1, P - 1] = tiny  # the last key's last element, next to the NaN gap
        _Round(dtype, K, numels, 5, packed=packed).check(f"{dtype} K={K} specials={n_special}")
    g = torch.Generator().manual_seed(K)
    packed = (torch.randn((K, P), generator=g, dtype=torch.float64) * 0.05).to(dtype)
    packed[0, 0] = tiny
    packed[K - 1, 300] = -tiny
    out, sumsq = _Round(dtype, K, numels, 6, packed=packed).check(f"{dtype} K={K} subnormals")
    assert bool(torch.isfinite(sumsq).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_steady_state_across_keys(dtype):
    """~9,000 keys of 1..300 elements at K = 3: more windows than the grid's
    4,096 waves, so waves take a second and third window in ANOTHER key -- the
    forward key scan, reloads across key boundaries, accumulators carried."""
    rng = np.random.default_rng(20240 + _es(dtype))
    numels = rng.integers(1, 301, size=9000)
    numels[rng.integers(0, 9000, size=200)] = 0  # empty keys among them
    r = _Round(dtype, 3, numels.tolist(), 99)
    _, _, WC = _plan(dtype, 3)
    assert sum(-(-n // WC) for n in r.numels) > 2 * 4096
    r.check(f"{dtype} 9000 keys")


# (K: the band's smallest, KMAX, slice bytes, workgroups per CU) per band of
# kVecBands16 / kVecBands64, and the tail: tests/test_gpu_fused_vec.py's STEADY
BANDS16 = [(1, 16, 16, 4), (17, 32, 8, 4), (33, 64, 8, 3), (65, 100, 4, 3), (101, 128, 4, 3)]
BANDS64 = [(1, 16, 16, 4), (17, 32, 16, 3), (33, 64, 8, 3)]
STEADY = ([(torch.float64, *b, 3) for b in BANDS64] + [(torch.float16, *b, 77) for b in BANDS16]
          + [(torch.bfloat16, *b, 77) for b in BANDS16])


@pytest.mark.parametrize("dtype,K,kmax,slice_bytes,per_cu,tail", STEADY,
                         ids=[f"{IDS(c[0])}-{c[2]}x{c[3]}" for c in STEADY])
def test_steady_state_in_one_key(dtype, K, kmax, slice_bytes, per_cu, tail):
    """One key long enough that every wave takes a second window and the
    first a third, ragged one: the reload of row i after its square, the next
    window's base and byte count, a ragged window reached through a prefetched
    register image."""
    lib = _lib.load_segvec()
    es = _es(dtype)
    assert _plan(dtype, K) == (kmax, slice_bytes, 64 * slice_bytes // es)
    waves, WC = 256 * per_cu * 4, 64 * slice_bytes // es
    P = 2 * waves * WC + tail
    ld = (P + 63) // 64 * 64 + 64
    g = torch.Generator(device=DEV).manual_seed(kmax * 1000 + es)
    x = torch.full((K, ld), float("nan"), dtype=dtype, device=DEV)
    for k in range(K):
        x[k, :P] = (torch.randn(P, generator=g, device=DEV) * 0.05 + 1e-2 * (k % 7 - 3)).to(dtype)
    weights = mfl_amd.sample_weights(torch.randint(1, 1000, (K,), generator=torch.Generator().manual_seed(kmax)).tolist())
    ptrs = np.array([[x[k].data_ptr()] for k in range(K)], dtype=np.int64)
    assert not (ptrs % 16).any()
    numel, offset, w64 = np.array([P], np.int64), np.array([0], np.int64), np.array(weights, np.float64)
    n_part = lib.fedavg_device_round_vec_partials(K, es)
    need = lib.fedavg_device_round_vec_workspace(K, 1)
    host_ws = torch.empty(need, dtype=torch.uint8, pin_memory=True)
    dev_ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    partials = torch.empty(n_part, dtype=torch.float64, device=DEV)

    def run():
        out = torch.full((P + 64,), SENTINEL, dtype=dtype, device=DEV)
        sumsq = torch.empty(K, dtype=torch.float64, device=DEV)
        rc = getattr(lib, ENTRY[dtype])(ptrs.ctypes.data, 1, None, numel.ctypes.data, offset.ctypes.data, 1, K,
                                        w64.ctypes.data, out.data_ptr(), partials.data_ptr(), n_part, sumsq.data_ptr(),
                                        host_ws.data_ptr(), dev_ws.data_ptr(), need,
                                        torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.fedavg_segvec_last_error()
        return out, sumsq

    out, sumsq = run()
    w = mfl_amd.weights_tensor(weights, dtype, DEV)
    two = mfl_amd.reduce_packed(x, w, P)
    assert np.array_equal(_bits(out[:P]), _bits(two[:P]))
    assert bool((out[P:] == SENTINEL).all())
    edges = [0, waves * WC, 2 * waves * WC]
    idx = torch.cat([torch.arange(max(0, e - 2 * WC), min(P, e + 2 * WC)) for e in edges]
                    + [torch.arange(P - tail - WC, P)]).unique().to(DEV)
    _same_bits_or_nan(out[idx], _oracle_out(x[:, idx].cpu(), weights))
    alone = mfl_amd.client_sqdist(x, two, P)
    _check_sums(sumsq.cpu().numpy(), alone.cpu().numpy(), P, f"{dtype} K={K} P={P} ({kmax} x {slice_bytes} B)")
    if K > 1:
        assert bool((sumsq[1:] > 0).all())
    assert np.array_equal(_bits(sumsq), _bits(run()[1]))
    del x, out, two, alone, partials
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refusals_launch_nothing(dtype):
    """A source 2 B (8 B for fp64) off 16-B alignment: FEDAVG_EALIGN; one
    client more than the bands hold: FEDAVG_EMODE; a host pointer in the
    table: FEDAVG_EINVAL.  All before any launch: out and sumsq untouched."""
    lib = _lib.load_segvec()
    es = _es(dtype)
    r = _Round(dtype, 4, [40, 0, 129], 3)
    out = torch.full((r.P + 67,), SENTINEL, dtype=dtype, device=DEV)
    for k, j in ((0, 0), (3, 2)):
        bad = r.ptrs.copy()
        bad[k, j] += es
        o, sumsq = r.call(out=out, ptrs=bad, expect=_lib.FEDAVG_EALIGN)
        assert bool((o == SENTINEL).all()) and bool((sumsq == -1.0).all())
    assert lib.fedavg_segvec_last_error().startswith(ENTRY[dtype].encode())
    off = r.ptrs.copy()
    off[:, 1] += es  # the EMPTY key's sources are never read: any address passes
    r.call(ptrs=off)
    host = torch.zeros(64, dtype=dtype).pin_memory()
    for k, j in ((0, 0), (3, 2)):  # the spot-checked sources: the first and the last
        bad = r.ptrs.copy()
        bad[k, j] = (host.data_ptr() + 15) // 16 * 16
        o, sumsq = r.call(out=out, ptrs=bad, expect=_lib.FEDAVG_EINVAL)
        assert bool((o == SENTINEL).all()) and bool((sumsq == -1.0).all())
    big = _Round(dtype, MAX_K[dtype] + 1, [40, 129], 4)
    o, sumsq = big.call(expect=_lib.FEDAVG_EMODE)
    assert bool((o == SENTINEL).all()) and bool((sumsq == -1.0).all())
    # every key empty: nothing to read, the sums are zero
    o, sumsq = _Round(dtype, 4, [0, 0], 5).call()
    assert bool((o == SENTINEL).all()) and bool((sumsq == 0.0).all())


# ---------------------------------------------------------------------------
# Drop-in (the SHAPES / MODELS of tests/test_gpu_fused_vec.py)
# ---------------------------------------------------------------------------
SHAPES = {"conv.weight": (16, 3, 3, 3), "conv.bias": (16,), "fc.weight": (10, 301), "fc.bias": (10,)}
MODELS = {
    "bf16": {k: torch.bfloat16 for k in SHAPES},
    "fp16": {k: torch.float16 for k in SHAPES},
    "fp64": {k: torch.float64 for k in SHAPES},
    "mixed": {"conv.weight": torch.float32, "conv.bias": torch.float32, "fc.weight": torch.bfloat16,
              "fc.bias": torch.bfloat16},
}
ROUNDS = [(m, K) for m in MODELS for K in (12, 64 if m == "fp64" else 100)]


def _model_round(model, K, seed):
    """CPU state_dicts (the reference's input); _to_dev puts them in HBM."""
    g = torch.Generator().manual_seed(seed)
    base = {k: torch.randn(s, generator=g) * 0.05 for k, s in SHAPES.items()}
    w_locals = []
    for i in range(K):
        sd = OrderedDict()
        for k, s in SHAPES.items():
            sd[k] = (base[k] + torch.randn(s, generator=g) * 5e-3).to(MODELS[model][k])
        if model == "mixed":
            sd["bn.num_batches_tracked"] = torch.tensor(100 + 3 * i, dtype=torch.int64)
        w_locals.append((int(torch.randint(1, 1000, (1,), generator=g)), sd))
    return w_locals


def _to_dev(w_locals):
    return [(n, OrderedDict((k, v.to(DEV)) for k, v in sd.items())) for n, sd in w_locals]


def _vec_groups(w_locals):
    return {t.dtype for t in w_locals[0][1].values() if t.dtype in ENTRY}


def _check_average(w_glob, ref):
    for k, e in ref.items():
        got = w_glob[k].cpu()
        assert got.dtype == e.dtype and got.shape == e.shape, k
        gn, en = torch.isnan(got.double()), torch.isnan(e.double())
        assert torch.equal(gn, en), k
        assert np.array_equal(_bits(got.reshape(-1)[~gn.reshape(-1)]), _bits(e.reshape(-1)[~en.reshape(-1)])), k


def _one_unit(w_locals):
    cat = None
    for t in w_locals[0][1].values():
        cat = t.dtype if cat is None else torch.promote_types(cat, t.dtype)
    return {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -10,
            torch.bfloat16: 2.0 ** -7}[cat]


def _two_pass_norms(ref_locals):
    """The same round through a second aggregator that packs every group into
    rows (the route before the zero-copy one) and whose fused sums are dropped:
    client_sqdist on packed rows."""
    agg2 = mfl_amd.DeviceAggregator(DEV)
    agg2.DEVICE_SEGMENTS = False
    locals2 = _to_dev(copy.deepcopy(ref_locals))
    w_glob2 = agg2.aggregate(locals2)
    assert agg2.vec_zero_copy_rounds == 0 and all(rows is not None for rows, _ in agg2._last["dev"].values())
    assert agg2._last.pop("sumsq", None)
    return np.asarray(agg2.client_distances(locals2, w_glob2), dtype=np.float64)


@pytest.mark.parametrize("model,K", ROUNDS, ids=[f"{m}-{K}" for m, K in ROUNDS])
def test_dropin_device_resident_rounds_take_the_zero_copy_route(model, K):
    ref_locals = _model_round(model, K, K + len(model))
    ref = O.aggregate_torch(copy.deepcopy(ref_locals))
    w_locals = _to_dev(ref_locals)
    groups = _vec_groups(ref_locals)
    agg = mfl_amd.DeviceAggregator(DEV)
    w_glob = agg.aggregate(w_locals)
    assert agg.vec_zero_copy_rounds == len(groups) >= 1
    for dt in groups:
        assert agg._last["dev"][dt][0] is None  # no rows were packed
        assert dt not in agg._staging  # and no [K, ld] staging buffer exists
        assert dt in agg._last["sumsq"]
    assert agg._last["segments"] is True
    assert w_glob is w_locals[0][1]
    _check_average(w_glob, ref)
    norms = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
    assert norms[0] == 0.0
    np.testing.assert_allclose(norms, _two_pass_norms(ref_locals), rtol=_one_unit(ref_locals), atol=0)


@pytest.mark.parametrize("model", ["bf16", "fp16", "fp64", "mixed"])
def test_fall_through_to_the_pack_route(model):
    """One client's key a misaligned view, and one client more than the bands
    hold: today's pack route, the same results, the counter unchanged."""
    dt = {"fp64": torch.float64, "fp16": torch.float16}.get(model, torch.bfloat16)
    for K, misalign in ((12, True), (MAX_K[dt] + 1, False)):
        ref_locals = _model_round(model, K, 7 * K + len(model))
        ref = O.aggregate_torch(copy.deepcopy(ref_locals))
        w_locals = _to_dev(ref_locals)
        if misalign:  # the same values, one element (2 B / 8 B) off the allocation's alignment
            sd = w_locals[5][1]
            t = sd["fc.weight"]
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
            buf[1:] = t.reshape(-1)
            sd["fc.weight"] = buf[1:].view(t.shape)
            assert sd["fc.weight"].data_ptr() % 16 != 0
        agg = mfl_amd.DeviceAggregator(DEV)
        w_glob = agg.aggregate(w_locals)
        assert agg.vec_zero_copy_rounds == 0
        assert agg._last["dev"][dt][0] is not None and dt in agg._staging  # packed rows
        assert w_glob is w_locals[0][1]
        _check_average(w_glob, ref)
        norms = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
        assert norms[0] == 0.0
        agg2 = mfl_amd.DeviceAggregator(DEV)
        agg2.DEVICE_SEGMENTS = False  # every group packed
        locals2 = _to_dev(copy.deepcopy(ref_locals))
        norms2 = np.asarray(agg2.client_distances(locals2, agg2.aggregate(locals2)), dtype=np.float64)
        np.testing.assert_allclose(norms, norms2, rtol=_one_unit(ref_locals), atol=0)


def test_fpf_record_round_after_a_zero_copy_round():
    """A mixed fp32 + bf16 model: record_round after the aggregate (rows packed
    on demand, client 0 from its own tensors) equals record_client before it."""
    K, n_total = 6, 9
    ref_locals = _model_round("mixed", K, 41)
    init = OrderedDict((k, torch.zeros_like(v)) for k, v in ref_locals[0][1].items())
    idx = [7, 2, 5, 0, 8, 3]
    agg = mfl_amd.DeviceAggregator(DEV)
    before = mfl_amd.FPFTracker(n_total, init, 3, device=DEV, aggregator=agg)
    after = mfl_amd.FPFTracker(n_total, init, 3, device=DEV, aggregator=agg)
    last_w = OrderedDict((k, v.to(DEV)) for k, v in init.items())
    w_locals = _to_dev(ref_locals)
    before.begin_round(last_w)
    after.begin_round(last_w)
    for c, (_, sd) in zip(idx, w_locals):
        before.record_client(c, sd)
    n0 = agg.vec_zero_copy_rounds
    w_glob = agg.aggregate(w_locals)
    assert agg.vec_zero_copy_rounds == n0 + 1 and agg._last["dev"][torch.bfloat16][0] is None
    after.record_round(idx, w_locals, w_glob)
    assert torch.equal(after.local_w_diffs.cpu(), before.local_w_diffs.cpu())
    assert bool((before.local_w_diffs[7] != 0).any())


@pytest.mark.parametrize("model", ["bf16", "fp64", "mixed"])
def test_client_distances_after_dropping_the_fused_sums(model):
    """Without the round's fused sums the rows are packed on demand and
    squared by client_sqdist: each group's fp64 sums against the fused pass's,
    and the norms against the fused norms, within 2 (P + 1) 2^-53 relative."""
    K = 12
    ref_locals = _model_round(model, K, 5 + len(model))
    w_locals = _to_dev(ref_locals)
    agg = mfl_amd.DeviceAggregator(DEV)
    w_glob = agg.aggregate(w_locals)
    fused = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
    fused_sums = agg._last.pop("sumsq")
    assert set(_vec_groups(ref_locals)) <= set(fused_sums)
    assert all(agg._last["dev"][dt][0] is None for dt in _vec_groups(ref_locals))
    two = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
    assert all(agg._last["dev"][dt][0] is not None for dt in _vec_groups(ref_locals))  # materialized
    # what the path computes before the root and its rounding: client_sqdist on the materialized rows
    for dt in _vec_groups(ref_locals):
        rows, out_dev = agg._last["dev"][dt]
        Pg = agg._last["table"].groups[dt].P
        alone = mfl_amd.client_sqdist(rows, out_dev, Pg)
        _check_sums(alone.cpu().numpy(), fused_sums[dt].cpu().numpy(), Pg, f"{model} {dt} materialized rows vs fused sums")
    P = sum(v.numel() for v in ref_locals[0][1].values())
    np.testing.assert_allclose(two, fused, rtol=_bound(P), atol=0)
    assert two[0] == 0.0 and bool((two[1:] > 0).all())
