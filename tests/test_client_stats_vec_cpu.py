"""The bf16 / fp16 / fp64 client statistics on the CPU.

(a) The dtype oracle (tests/client_stats_vec_oracle.py) is pinned to the
    reference's own expressions: ClientStepStats(stats="torch") on CPU
    parameters of each dtype, fed the recorded (w_t, g_t, loss_t) sequences of
    tests/golden/client cast to the dtype, takes the oracle's guard decisions
    and ends within 4 units in the last place of T of its rho / beta (one ulp
    of a norm, ATen's opmath accumulation against the exact sum, passes
    through at most three roundings).  A fixture whose norm(g) lies within
    2 ulp of its bound has no well-defined decision and is dropped; the two
    tripping and at least two non-tripping fixtures must remain.
(b) Mode selection on CPU tensors, the refusal text of stats="hip", and the
    host-side rounding helpers against torch's CPU casts.
"""
import math

import numpy as np
import pytest
import torch

import client_stats_oracle as O
import client_stats_vec_oracle as V
import mfl_amd
from mfl_amd import client_stats

CASES = O.client_case_names()
TRIPPING = ("nan_input_trips", "tiny_weights_trip")
_replays = {}


def _replay(name, key):
    """(case, w, g, trip, beta, rho, margins) of the oracle, once per (fixture, dtype)."""
    if (name, key) not in _replays:
        dt = V.DTYPES[key]
        case = O.load_client_case(name)
        w, g = V.cast_sequence(case, dt)
        margins = []
        trip, beta, rho = V.replay(w, g, case["loss"], case["meta"]["lr"], case["meta"]["ratio"], dt, margins)
        _replays[(name, key)] = (case, w, g, trip, beta, rho, margins)
    return _replays[(name, key)]


def _well_defined(name, key):
    return all(m >= 2.0 for m in _replay(name, key)[6])


@pytest.mark.parametrize("key", sorted(V.DTYPES))
def test_enough_fixtures_have_a_well_defined_guard(key):
    kept = [n for n in CASES if _well_defined(n, key)]
    print(f"{key}: kept {kept}; margins {[(n, [round(m, 1) for m in _replay(n, key)[6]]) for n in CASES]}")
    tripping = [n for n in kept if _replay(n, key)[3] is not None]
    assert set(TRIPPING) <= set(tripping)
    assert len(kept) - len(tripping) >= 2


def _set(params, flat, grads):
    off = 0
    with torch.no_grad():
        for p in params:
            n = p.numel()
            t = flat[off:off + n].view_as(p)
            if grads:
                p.grad = t.clone()
            else:
                p.copy_(t)
            off += n


@pytest.mark.parametrize("key", sorted(V.DTYPES))
@pytest.mark.parametrize("name", CASES)
def test_torch_mode_on_cpu_agrees_with_the_oracle(name, key):
    dt = V.DTYPES[key]
    case, w, g, o_trip, o_beta, o_rho, margins = _replay(name, key)
    if not _well_defined(name, key):
        # no skip: the fixture is simply not among those this dtype relies on (see the test above)
        assert min(margins) < 2.0
        return
    meta, loss = case["meta"], case["loss"]
    net = O.build_model(meta["model"]).to(dt)
    params = list(net.parameters())
    _set(params, w[0], False)
    _set(params, g[0], True)
    stats = mfl_amd.ClientStepStats(params, stats="torch")
    assert stats.mode == "torch"
    stats.begin(float(loss[0]))
    tripped_at = None
    for t in range(1, len(g)):
        _set(params, g[t], True)
        if stats.after_backward(torch.tensor(float(loss[t])), meta["lr"], meta["ratio"]):
            tripped_at = t - 1
            break
        _set(params, w[t], False)
        stats.after_step(float(loss[t]), float(loss[t - 1]))
    beta, rho = stats.result()
    print(f"{name} {key}: trip {tripped_at} oracle {o_trip}; beta {beta!r} oracle {o_beta!r}; rho {rho!r} "
          f"oracle {o_rho!r}")
    assert tripped_at == o_trip
    assert (tripped_at is not None) == meta["tripped"]
    if tripped_at is not None:
        return
    assert V.within_ulps(beta, o_beta, 4, dt), (beta, o_beta)
    assert V.within_ulps(rho, o_rho, 4, dt), (rho, o_rho)


def test_mode_selection_on_cpu_and_the_refusal_text():
    net = O.build_model({"sizes": [4, 3]})
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        params = list(net.to(dt).parameters())
        assert mfl_amd.ClientStepStats(params).mode == "torch"  # CPU parameters stay on torch
        assert not client_stats._fused_ok(params)
        with pytest.raises(TypeError, match="one dtype among fp32, bf16, fp16 and fp64"):
            mfl_amd.ClientStepStats(params, stats="hip")
    mixed = [torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(3))]
    assert mfl_amd.ClientStepStats(mixed).mode == "torch"
    with pytest.raises(TypeError, match="all of one dtype"):
        mfl_amd.ClientStepStats(mixed, stats="hip")
    assert not client_stats._fused_ok([])
    assert set(client_stats.FUSED_DTYPES) == {torch.float32, torch.bfloat16, torch.float16, torch.float64}


class _Fake:
    """Stands in for a CUDA parameter: _fused_ok reads attributes only."""

    def __init__(self, dtype, device="cuda:0", contiguous=True):
        self.dtype, self.device, self.is_cuda, self._c = dtype, device, True, contiguous

    def is_contiguous(self):
        return self._c


def test_the_dtype_rule():
    ok = client_stats._fused_ok
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        assert ok([_Fake(dt), _Fake(dt)])
        assert not ok([_Fake(dt), _Fake(dt, contiguous=False)])
        assert not ok([_Fake(dt), _Fake(dt, device="cuda:1")])
    assert not ok([_Fake(torch.bfloat16), _Fake(torch.float16)])
    assert not ok([_Fake(torch.float32), _Fake(torch.float64)])
    for dt in (torch.int64, torch.float8_e4m3fn, torch.complex64):
        assert not ok([_Fake(dt)])


@pytest.mark.parametrize("key", ["bf16", "f16"])
def test_host_rounding_equals_torch_cpu_casts(key):
    """client_stats._round_to / _norm_of / _guard_bound (the host side of the
    :71 guard) against torch's CPU casts and the oracle's guard terms."""
    dt = V.DTYPES[key]
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.normal(0, 1, 500) * 10.0 ** rng.integers(-12, 6, 500),
                         [0.0, -0.0, math.inf, -math.inf, 65504.0, 65520.0, 65519.99, 3.3895e38, 3.4e38, 1e-45, 6e-8,
                          2.98e-8, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -9]])
    for x in xs:
        assert V.same(client_stats._round_to(float(x), dt), V.rT(float(x), dt)), x
    assert math.isnan(client_stats._round_to(math.nan, dt)) and math.isnan(client_stats._norm_of(math.nan, dt))
    for s_g, s_w, lr_ratio in zip(rng.uniform(0, 50, 300) ** 2, rng.uniform(0, 50, 300) ** 2,
                                  rng.uniform(1e-3, 30.0, 300)):
        n_g, bound = V.guard_terms(s_g, s_w, lr_ratio, 1.0, dt)
        assert client_stats._norm_of(s_g, dt) == n_g
        assert client_stats._guard_bound(client_stats._norm_of(s_w, dt), lr_ratio, dt) == bound
    assert client_stats._norm_of(math.inf, dt) == math.inf


_TIES = 600


def _fp32_guard_sums():
    """Sums of squares whose roots sit at the edges of fp32: zero, the
    subnormal ends, the overflow end, inf and nan, then for _TIES seeded fp32
    rounding midpoints m the sums (m (1 - 2^-40))^2 and (m (1 + 2^-40))^2,
    whose roots lie either side of the tie, and m^2 with its two fp64
    neighbours, whose fp64 roots may land on the tie itself."""
    rng = np.random.default_rng(71)
    f = (rng.uniform(1.0, 2.0, _TIES) * 2.0 ** rng.integers(-140, 127, _TIES)).astype(np.float32)
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2  # exact in fp64
    sq = mid * mid
    return [0.0, 5e-324, 2.0 ** -149, 2.0 ** -126, 2.0 ** 127, 2.0 ** 128, 2.0 ** 256, 1e300, math.inf, math.nan,
            *((mid * (1 - 2.0 ** -40)) ** 2).tolist(), *((mid * (1 + 2.0 ** -40)) ** 2).tolist(),
            *np.nextafter(sq, 0.0).tolist(), *sq.tolist(), *np.nextafter(sq, np.inf).tolist()]


def test_fp32_guard_terms_equal_the_inline_fp32_expressions_bit_for_bit():
    """_norm_of / _guard_bound at fp32 against the expressions the fp32 guard
    was written with (``np.float32(math.sqrt(s))``, NaN kept apart, and
    ``np.float32(lr * ratio) * n_w``): equal bits, NaN matched as NaN, and the
    same ``n_g > bound`` on the whole cross product.  No case is left out."""
    dt = torch.float32
    bits = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)  # noqa: E731
    sums = _fp32_guard_sums()
    lr_ratios = [0.0, 1e-30, 0.1, 1e10, 1e12 * 0.01, 1e39, math.inf]
    with np.errstate(all="ignore"):
        inline = np.array([np.float32(math.sqrt(s)) if not math.isnan(s) else np.float32("nan") for s in sums])
        norms = np.array([client_stats._norm_of(s, dt) for s in sums])  # Python floats
        assert np.array_equal(norms.astype(np.float32).astype(np.float64), norms, equal_nan=True)  # fp32 values
        nan = np.isnan(inline)
        assert np.array_equal(nan, np.isnan(norms)) and nan.sum() == 1
        assert np.array_equal(bits(inline)[~nan], bits(norms)[~nan])
        assert {0.0, math.inf} <= set(norms[~nan].tolist())
        assert (norms[10:10 + _TIES] < norms[10 + _TIES:10 + 2 * _TIES]).all()  # the two sides of every tie part
        inline_b = np.array([[np.float32(r) * n_w for n_w in inline] for r in lr_ratios])
        bounds = np.array([[client_stats._guard_bound(float(n_w), r, dt) for n_w in norms] for r in lr_ratios])
    nan_b = np.isnan(inline_b)
    assert np.array_equal(nan_b, np.isnan(bounds)) and nan_b.any() and not nan_b.all()  # inf * 0, NaN norms
    assert np.array_equal(bits(inline_b)[~nan_b], bits(bounds)[~nan_b])
    assert np.isinf(bounds[~nan_b]).any() and (bounds[~nan_b] == 0.0).any()
    flat_inline, flat = inline_b.reshape(-1), bounds.reshape(-1)
    trips = 0
    for n_inline, n in zip(inline, norms):  # n_g over every (lr * ratio, n_w)
        want = n_inline > flat_inline
        assert np.array_equal(want, n > flat)
        trips += int(want.sum())
    assert 0 < trips < len(sums) * flat.size


def test_host_rounding_fp64_is_plain_fp64():
    dt = torch.float64
    assert client_stats._round_to(0.1, dt) == 0.1
    assert client_stats._norm_of(2.0, dt) == math.sqrt(2.0)
    assert client_stats._guard_bound(3.0, 0.1, dt) == 3.0 * 0.1 == V.guard_terms(1.0, 9.0, 0.1, 1.0, dt)[1]
