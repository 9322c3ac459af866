"""The numpy oracle of the client statistics against the reference's own
``Client.train`` (fixtures: scripts/gen_golden_client.py), and the update rule
of client.py:79 / :83 pinned on synthetic sequences.  CPU only."""
import math

import numpy as np
import pytest

import client_stats_oracle as O

CASES = O.client_case_names()


def test_fixtures_present():
    assert set(CASES) >= {"linear_20x5_it3", "linear_20x5_it1", "mlp_16x24x4_it4", "mnist_lr_it2", "nan_input_trips",
                          "tiny_weights_trip"}


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference(name):
    case = O.load_client_case(name)
    meta = case["meta"]
    tripped_at, beta, rho = O.replay(case["w"], case["g"], case["loss"], meta["lr"], meta["ratio"])
    if meta["tripped"]:
        # the reference returned the all-None tuple (client.py:73)
        assert tripped_at == meta["steps"] and beta is None and rho is None
        assert all(math.isnan(v) for v in case["ret"])
        return
    assert tripped_at is None
    ref_beta, ref_rho = float(case["ret"][1]), float(case["ret"][2])
    bound = O.ref_bound(meta)
    print(f"{name}: beta {beta!r} vs {ref_beta!r}, rho {rho!r} vs {ref_rho!r}, bound {bound:.3e}")
    assert O.rel(beta, ref_beta) <= bound
    assert O.rel(rho, ref_rho) <= bound


def test_guard_scenarios_trip_for_their_own_reason():
    nan_case = O.load_client_case("nan_input_trips")
    assert O.record(nan_case["g"][1])[0] > 0 and math.isnan(float(nan_case["loss"][1]))
    tiny = O.load_client_case("tiny_weights_trip")
    nan_g, sum_g, _ = O.record(tiny["g"][1])
    assert nan_g == 0 and not math.isnan(float(tiny["loss"][1]))
    assert O.guard(0, sum_g, O.record(tiny["w"][0])[1], float(tiny["loss"][1]), tiny["meta"]["lr"],
                   tiny["meta"]["ratio"])


def test_record_sums_are_exact():
    cur = np.array([3.0, 4.0, np.nan, 1e-30], dtype=np.float32)
    assert O.record(cur[:2]) == (0, 25.0, 0.0)
    assert O.record(cur[:2], np.array([0.0, 1.0], np.float32)) == (0, 25.0, 18.0)
    n, s, _ = O.record(cur)
    assert n == 1 and math.isnan(s)
    assert O.record(np.array([np.inf, -np.inf, 1.0], np.float32))[:2] == (0, math.inf)


def test_rtruediv_formula_matches_installed_torch():
    """python_float / fp32 0-dim tensor: the formula written into include/fedavg_amd.h."""
    import torch

    rng = np.random.default_rng(5)
    for _ in range(200):
        n_w = np.float32(rng.uniform(1e-4, 10.0))
        a = float(rng.uniform(0.0, 3.0))
        got = (a / torch.tensor(n_w)).item()
        want = float(np.float32(np.float32(1.0) / n_w) * np.float32(a))
        assert got == want
        n_g = np.float32(rng.uniform(1e-4, 10.0))
        assert (torch.tensor(n_g) / torch.tensor(n_w)).item() == float(np.float32(n_g / n_w))


def _run(seq):
    t = O.Track()
    for n_w, n_g, dl in seq:
        t.step(float(n_w) ** 2, float(n_g) ** 2, dl)
    return t


def test_first_zero_is_replaced_by_a_smaller_later_value():
    # iteration 1 of every run: loss == last_loss and grads == last_grads -> rho = beta = 0
    t = _run([(1.0, 0.0, 0.0), (1.0, 0.5, 0.25)])
    assert float(t.rho) == 0.25 and float(t.beta) == 0.5
    t = _run([(1.0, 2.0, 2.0), (1.0, 0.5, 0.25)])  # a set non-zero maximum stays
    assert float(t.rho) == 2.0 and float(t.beta) == 2.0


def test_nan_after_a_set_value_is_ignored():
    t = _run([(1.0, 2.0, 3.0), (1.0, float("nan"), float("nan")), (1.0, 1.0, 1.0)])
    assert float(t.rho) == 3.0 and float(t.beta) == 2.0


def test_nan_first_is_sticky():
    t = _run([(1.0, float("nan"), float("nan")), (1.0, 5.0, 5.0)])
    assert math.isnan(t.rho) and math.isnan(t.beta)
    t = _run([(1.0, 0.0, 0.0), (1.0, float("nan"), float("nan")), (1.0, 5.0, 5.0)])  # NaN replaces a zero
    assert math.isnan(t.rho) and math.isnan(t.beta)


def test_update_rule_is_the_reference_statement():
    """``if not x or tmp > x: x = tmp`` on torch tensors, for every pairing."""
    import torch

    vals = [None, 0.0, 1.0, 2.0, float("nan")]
    for x in vals:
        for tmp in vals[1:]:
            xt = None if x is None else torch.tensor(x)
            tt = torch.tensor(tmp)
            ref = xt
            if not ref or tt > ref:
                ref = tt
            got = O.update(None if x is None else np.float32(x), np.float32(tmp))
            assert (math.isnan(got) and math.isnan(ref.item())) or float(got) == ref.item(), (x, tmp)
