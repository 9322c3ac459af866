"""GPU parity of the one-read aggregate + :291 pass for fp64 / fp16 / bf16
rows (fedavg_reduce_sqdist_{f64,f16,bf16}, libfedavg_amd_fusedvec.so).

``out`` carries the bits of ``reduce_packed`` and of the oracle's chain.
``sumsq`` is held to a bound, not a measurement: the 16-bit squares are exact
in fp64 and the fp64 ones carry one fma rounding each, and two fixed
summation orders of P non-negative terms each sit within (P - 1) * 2^-53 of
the exact sum -- so any two of {fused pass, standalone pass, math.fsum of the
oracle's rounded differences squared} differ by at most 2 (P + 1) 2^-53
relative.
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
KS = [1, 2, 16, 17, 32, 33, 64, 65, 100, 128, 129]  # every band edge and the first K of the two-pass route
PS = [1, 7, 8, 9, 63, 64, 65, 127, 129, 511, 513, 4097]  # slice, lane and window tails
ENTRY = {torch.float64: "fedavg_reduce_sqdist_f64", torch.float16: "fedavg_reduce_sqdist_f16",
         torch.bfloat16: "fedavg_reduce_sqdist_bf16"}


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_available):
    _lib.load_fusedvec()
    torch.cuda.set_device(DEV)
    yield


def _bound(P):
    return 2 * (P + 1) * 2.0 ** -53


def _rows(dtype, K, P, seed):
    """[K, ld] rows, ld padded past P with NaN in the padding; weights from
    random sample counts through the project's helpers."""
    ld = (P + 63) // 64 * 64 + 64
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn((K, P), generator=g, dtype=torch.float64) * 0.05 + torch.randn((K, 1), generator=g,
                                                                                   dtype=torch.float64) * 1e-2
    x = torch.full((K, ld), float("nan"), dtype=dtype)
    x[:, :P] = vals.to(dtype)
    counts = torch.randint(1, 1000, (K,), generator=g).tolist()
    weights = mfl_amd.sample_weights(counts)
    return x.to(DEV), ld, weights


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()]).numpy()


def _oracle_out(x, P, weights):
    """The oracle's chain on the rows' valid columns (its own representation)."""
    h = x[:, :P].cpu()
    if h.dtype == torch.float64:
        return O.reduce_f64(h.numpy(), weights)
    if h.dtype == torch.float16:
        return O.reduce_half(h.numpy(), weights, "float16")
    return O.reduce_half(h.contiguous().view(torch.int16).numpy().view(np.uint16), weights, "bfloat16")


def _same_bits_or_nan(got, exp_arr):
    """Bit equality; NaN payloads are not compared, NaN positions are."""
    if got.dtype == torch.float64:
        g, e = got.cpu().numpy(), exp_arr
    elif got.dtype == torch.float16:
        g, e = got.cpu().numpy(), exp_arr
    else:
        g = O.bf16_bits_to_f32(got.cpu().contiguous().view(torch.int16).numpy().view(np.uint16))
        e = O.bf16_bits_to_f32(exp_arr)
    gn, en = np.isnan(g), np.isnan(e)
    assert np.array_equal(gn, en)
    assert g[~gn].tobytes() == e[~en].tobytes()


def _oracle_sumsq(x, out, P):
    """math.fsum of the oracle's rounded differences squared, per client."""
    h, g = x[:, :P].cpu(), out[:P].cpu()
    if h.dtype == torch.float64:
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


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_fused_vec_vs_two_passes_and_oracle(dtype, K):
    fv = _lib.load_fusedvec()
    es = torch.empty((), dtype=dtype).element_size()
    for P in PS:
        x, ld, weights = _rows(dtype, K, P, K * 100_003 + P)
        w = mfl_amd.weights_tensor(weights, dtype, DEV)
        assert (fv.fedavg_fused_vec_plan_of(K, P, es, int(dtype == torch.bfloat16)) != 0) == (
            K <= (64 if dtype == torch.float64 else 128))
        out, sumsq = mfl_amd.reduce_with_sqdist(x, w, P)
        two = mfl_amd.reduce_packed(x, w, P)
        assert np.array_equal(_bits(out), _bits(two)), (K, P)
        _same_bits_or_nan(out, _oracle_out(x, P, weights))
        alone = mfl_amd.client_sqdist(x, out, P)
        _check_sums(sumsq.cpu().numpy(), alone.cpu().numpy(), P, f"{dtype} K={K} P={P} vs client_sqdist")
        _check_sums(sumsq.cpu().numpy(), _oracle_sumsq(x, out, P), P, f"{dtype} K={K} P={P} vs fsum")
        again = mfl_amd.reduce_with_sqdist(x, w, P)[1]
        assert torch.equal(sumsq, again), (K, P)  # deterministic


@pytest.mark.parametrize("K", [5, 40, 100])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_fused_vec_nonfinite_and_subnormal_columns(dtype, K):
    """NaN / +-inf / subnormal entries in single columns: sumsq's NaN (and
    inf) positions equal the standalone pass's, finite sums stay within the
    bound -- another client's NaN reaches a client only through the average.
    (fp64 at K = 100 is the two-pass route inside the same call.)"""
    P = 777
    tiny = {torch.float64: 5e-324, torch.float16: 6e-8, torch.bfloat16: 9.2e-41}[dtype]
    specials = [float("nan"), float("inf"), float("-inf"), tiny, -tiny]
    for n_special in (1, 3, 5):
        x, ld, weights = _rows(dtype, K, P, K * 31 + n_special)
        for j in range(n_special):
            x[(j * 7 + 1) % K, (j * 131 + 5) % P] = specials[j]
        x[K - 1, P - 1] = tiny  # the last valid column, next to the NaN padding
        w = mfl_amd.weights_tensor(weights, dtype, DEV)
        out, sumsq = mfl_amd.reduce_with_sqdist(x, w, P)
        two = mfl_amd.reduce_packed(x, w, P)
        on, tn = torch.isnan(out), torch.isnan(two)
        assert torch.equal(on, tn)
        assert np.array_equal(_bits(out[~on]), _bits(two[~tn]))
        alone = mfl_amd.client_sqdist(x, out, P)
        _check_sums(sumsq.cpu().numpy(), alone.cpu().numpy(), P, f"{dtype} K={K} specials={n_special}")
    # only subnormals: every sum finite and positive
    x, ld, weights = _rows(dtype, K, P, K)
    x[0, 3] = tiny
    x[K - 1, 4] = -tiny
    w = mfl_amd.weights_tensor(weights, dtype, DEV)
    out, sumsq = mfl_amd.reduce_with_sqdist(x, w, P)
    assert bool(torch.isfinite(sumsq).all())
    _check_sums(sumsq.cpu().numpy(), _oracle_sumsq(x, out, P), P, f"{dtype} K={K} subnormals")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_fused_vec_unaligned_rows_are_refused(dtype):
    """A row base 2 B / 8 B off 16, or ld * elem_size % 16 != 0: FEDAVG_EALIGN, out untouched."""
    fv = _lib.load_fusedvec()
    es = torch.empty((), dtype=dtype).element_size()
    K, P = 3, 100
    buf = torch.zeros(K * 256 + 64, dtype=dtype, device=DEV)
    w = mfl_amd.weights_tensor([0.25, 0.25, 0.5], dtype, DEV)
    out = torch.full((128,), 7.0, dtype=dtype, device=DEV)
    ws = torch.empty(max(fv.fedavg_reduce_sqdist_vec_workspace(K, P, es), 1), dtype=torch.float64, device=DEV)
    sumsq = torch.full((K,), -1.0, dtype=torch.float64, device=DEV)
    fn = getattr(fv, ENTRY[dtype])
    s = torch.cuda.current_stream(DEV).cuda_stream
    off_elems = [1] if es == 8 else [1, 4]  # 8 B; 2 B and 8 B
    for off in off_elems:
        rc = fn(buf.data_ptr() + off * es, K, P, 256, w.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                sumsq.data_ptr(), s)
        assert rc == _lib.FEDAVG_EALIGN, off
    bad_ld = 256 + (1 if es == 8 else 4)
    rc = fn(buf.data_ptr(), K, P, bad_ld, w.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), sumsq.data_ptr(), s)
    assert rc == _lib.FEDAVG_EALIGN
    assert fv.fedavg_fusedvec_last_error().startswith(ENTRY[dtype].encode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((sumsq == -1.0).all())
    with pytest.raises(_lib.FedAvgLibraryError):
        mfl_amd.reduce_with_sqdist(buf[1:1 + K * 256].view(K, 256), w, P)
    # P == 0 zeroes sumsq
    assert fn(buf.data_ptr(), K, 0, 256, w.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), sumsq.data_ptr(),
              s) == 0
    torch.cuda.synchronize()
    assert bool((sumsq == 0.0).all())


# ---------------------------------------------------------------------------
# Steady state: rows long enough that every wave takes a second window and
# the first wave a third, ragged one.  The launch is persistent -- 256 CUs x
# 3 or 4 workgroups x 4 waves, a window of 64 lanes x `slice` bytes per wave --
# so below 2 x waves x window columns (0.2M to 2M columns by band) a wave
# runs its loop once and every reload reads the empty descriptor.  Here the
# reload of row i after its square, the next window's address and byte count,
# the LDS accumulators carried across windows and a ragged last window
# reached through a prefetched register image all decide the result.
# (K, KMAX, slice bytes, workgroups per CU) per band of kVecBands16 / 64.
# ---------------------------------------------------------------------------
BANDS16 = [(10, 16, 16, 4), (20, 32, 8, 4), (50, 64, 8, 3), (100, 100, 4, 3), (128, 128, 4, 3)]
BANDS64 = [(10, 16, 16, 4), (20, 32, 16, 3), (64, 64, 8, 3)]
STEADY = ([(torch.float64, *b, 3) for b in BANDS64] + [(torch.float16, *b, 77) for b in BANDS16]
          + [(torch.bfloat16, *b, 77) for b in BANDS16])


def _long_rows(dtype, K, P, seed):
    """_rows on the device (up to 100M elements): NaN padding past P."""
    ld = (P + 63) // 64 * 64 + 64
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.full((K, ld), float("nan"), dtype=dtype, device=DEV)
    for k in range(K):
        x[k, :P] = (torch.randn(P, generator=g, device=DEV) * 0.05 + 1e-2 * (k % 7 - 3)).to(dtype)
    counts = torch.randint(1, 1000, (K,), generator=torch.Generator().manual_seed(seed)).tolist()
    return x, mfl_amd.sample_weights(counts)


@pytest.mark.parametrize("dtype,K,kmax,slice_bytes,per_cu,tail", STEADY,
                         ids=[f"{str(c[0]).split('.')[-1]}-{c[2]}x{c[3]}" for c in STEADY])
def test_fused_vec_steady_state_windows(dtype, K, kmax, slice_bytes, per_cu, tail):
    fv = _lib.load_fusedvec()
    es = torch.empty((), dtype=dtype).element_size()
    waves = 256 * per_cu * 4
    win_cols = 64 * slice_bytes // es
    P = 2 * waves * win_cols + tail
    assert fv.fedavg_fused_vec_plan_of(K, P, es, int(dtype == torch.bfloat16)) == 3_000_000 + kmax * 100 + slice_bytes
    x, weights = _long_rows(dtype, K, P, kmax * 1000 + es)
    w = mfl_amd.weights_tensor(weights, dtype, DEV)
    out, sumsq = mfl_amd.reduce_with_sqdist(x, w, P)
    two = mfl_amd.reduce_packed(x, w, P)
    assert np.array_equal(_bits(out), _bits(two))
    # the oracle on the columns around every window a wave changes at: the first windows,
    # the end of the first pass / start of the second, of the second / the third, and the tail
    edges = [0, waves * win_cols, 2 * waves * win_cols]
    idx = torch.cat([torch.arange(max(0, e - 2 * win_cols), min(P, e + 2 * win_cols)) for e in edges]
                    + [torch.arange(P - tail - win_cols, P)]).unique().to(DEV)
    _same_bits_or_nan(out[idx], _oracle_out(x[:, idx], idx.numel(), weights))
    alone = mfl_amd.client_sqdist(x, out, P)
    _check_sums(sumsq.cpu().numpy(), alone.cpu().numpy(), P, f"{dtype} K={K} P={P} ({kmax} x {slice_bytes} B)")
    assert bool((sumsq[1:] > 0).all())
    again = mfl_amd.reduce_with_sqdist(x, w, P)[1]
    assert torch.equal(sumsq, again)
    del x, out, two
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# Drop-in
# ---------------------------------------------------------------------------
SHAPES = {"conv.weight": (16, 3, 3, 3), "conv.bias": (16,), "fc.weight": (10, 301), "fc.bias": (10,)}
MODELS = {
    "bf16": {k: torch.bfloat16 for k in SHAPES},
    "fp16": {k: torch.float16 for k in SHAPES},
    "fp64": {k: torch.float64 for k in SHAPES},
    "mixed": {"conv.weight": torch.float32, "conv.bias": torch.float32, "fc.weight": torch.bfloat16,
              "fc.bias": torch.bfloat16},
}


def _model_round(model, K, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    base = {k: torch.randn(s, generator=g) * 0.05 for k, s in SHAPES.items()}
    w_locals = []
    for i in range(K):
        sd = OrderedDict()
        for k, s in SHAPES.items():
            sd[k] = (base[k] + torch.randn(s, generator=g) * 5e-3).to(MODELS[model][k]).to(device)
        if model == "mixed":
            sd["bn.num_batches_tracked"] = torch.tensor(100 + 3 * i, dtype=torch.int64, device=device)
        w_locals.append((int(torch.randint(1, 1000, (1,), generator=g)), sd))
    return w_locals


def _float_groups(w_locals):
    """The dtype groups of the packed round: integer keys ride in the fp32 group."""
    return {torch.float32 if not t.dtype.is_floating_point else t.dtype for t in w_locals[0][1].values()}


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


def _two_pass_norms(ref_locals, device="cpu"):
    """The same round through a second aggregator whose fused sums are dropped."""
    agg2 = mfl_amd.DeviceAggregator(DEV)
    agg2.SMALL_ROUND_BYTES = 0
    locals2 = [(n, OrderedDict((k, v.to(device)) for k, v in sd.items())) for n, sd in copy.deepcopy(ref_locals)]
    w_glob2 = agg2.aggregate(locals2)
    assert agg2._last.pop("sumsq", None)
    return np.asarray(agg2.client_distances(locals2, w_glob2), dtype=np.float64)


@pytest.mark.parametrize("K", [3, 100])
@pytest.mark.parametrize("model", list(MODELS))
def test_dropin_host_state_dicts(model, K):
    w_locals = _model_round(model, K, K + len(model))
    ref_locals = copy.deepcopy(w_locals)
    ref = O.aggregate_torch(copy.deepcopy(ref_locals))
    agg = mfl_amd.DeviceAggregator(DEV)
    agg.SMALL_ROUND_BYTES = 0
    w_glob = agg.aggregate(w_locals)
    assert set(agg._last["sumsq"]) == _float_groups(ref_locals)
    norms = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
    assert norms[0] == 0.0
    _check_average(w_glob, ref)
    np.testing.assert_allclose(norms, _two_pass_norms(ref_locals), rtol=_one_unit(ref_locals), atol=0)


def test_dropin_device_resident_bf16_clients():
    K = 12
    w_locals = _model_round("bf16", K, 77, device=DEV)
    ref_locals = [(n, OrderedDict((k, v.cpu()) for k, v in sd.items())) for n, sd in w_locals]
    ref = O.aggregate_torch(copy.deepcopy(ref_locals))
    agg = mfl_amd.DeviceAggregator(DEV)
    w_glob = agg.aggregate(w_locals)
    assert set(agg._last["sumsq"]) == {torch.bfloat16}
    norms = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
    assert norms[0] == 0.0
    _check_average(w_glob, ref)
    np.testing.assert_allclose(norms, _two_pass_norms(ref_locals, device=DEV), rtol=_one_unit(ref_locals), atol=0)


def test_dropin_streamed_fp16_round():
    K = 9
    w_locals = _model_round("fp16", K, 99)
    ref_locals = copy.deepcopy(w_locals)
    ref = O.aggregate_torch(copy.deepcopy(ref_locals))
    agg = mfl_amd.DeviceAggregator(DEV)
    agg.SMALL_ROUND_BYTES = 0
    sess = agg.begin_round(w_locals[0][1], K)
    for n, sd in w_locals:
        sess.add(n, sd)
    w_glob = sess.finish(w_locals)
    assert set(agg._last["sumsq"]) == {torch.float16}
    norms = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
    assert norms[0] == 0.0
    _check_average(w_glob, ref)
    np.testing.assert_allclose(norms, _two_pass_norms(ref_locals), rtol=_one_unit(ref_locals), atol=0)


@pytest.mark.parametrize("model", ["bf16", "mixed"])
def test_dropin_sharded_round(model):
    """multi.ShardedAggregator's round reduces each device's column shard
    through the same ``reduce_rows``: its 16-bit shards take the one-read pass
    too (two shards rehearsed on one device)."""
    K = 12
    w_locals = _model_round(model, K, 55 + len(model))
    ref_locals = copy.deepcopy(w_locals)
    ref = O.aggregate_torch(copy.deepcopy(ref_locals))
    agg = mfl_amd.ShardedAggregator([DEV.index or 0] * 2)
    agg.SMALL_ROUND_BYTES = 0
    w_glob = agg.aggregate(w_locals)
    assert agg.rounds_sharded == 1
    parts = [p for dev in agg._last["per_dev"] for p in dev.items()]
    assert torch.bfloat16 in {dt for dt, _ in parts} and all(p[2] is not None for _, p in parts)
    norms = np.asarray(agg.client_distances(w_locals, w_glob), dtype=np.float64)
    assert norms[0] == 0.0
    _check_average(w_glob, ref)
    np.testing.assert_allclose(norms, _two_pass_norms(ref_locals), rtol=_one_unit(ref_locals), atol=0)
