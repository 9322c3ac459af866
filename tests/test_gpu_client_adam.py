"""The fused client Adam step on the MI355X through the Python layer:
client_stats.adam_form's answer, and client_train on the small MLP case with
client_optimizer="adam", step="fused" against step="torch" (the traced weights
after every iteration bit for bit, the same guard decisions, rho / beta under
test_gpu_client_step.py's rule), one host sync per iteration, and the refusal
for a dtype without a form.

If adam_form finds no mask for any dtype this file fails: the feature would be
unusable, and the per-op probe (scripts/probe_adam_ops.py) has to be taken
further."""
import types

import numpy as np
import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import client_stats

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
KEYS = [k for k, dt in DTYPES.items() if dt in client_stats.ADAM_DTYPES]
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def test_some_dtype_has_a_form():
    assert KEYS, "adam_form found a mask for no dtype: the fused Adam step cannot be offered"
    assert "f32" in KEYS


@pytest.mark.parametrize("key", KEYS)
def test_adam_form_is_one_mask_stable_and_cached(dev, key):
    found = client_stats.adam_form_probe(dev, DTYPES[key])
    print(f"adam_form {key}: form {found['form']} off {found['off']}")
    assert found["form"] is not None and 0 <= found["form"] < 16
    assert sum(found["match"]) == 1 and found["match"][found["form"]] and found["off"][found["form"]] == 0
    assert all(o > 0 for f, o in enumerate(found["off"]) if f != found["form"])  # every other mask differs from torch
    assert client_stats.adam_form(dev, DTYPES[key]) == found["form"] == mfl_amd.adam_form(dev, DTYPES[key])
    assert client_stats.adam_form_probe(dev, DTYPES[key]) is found  # cached: one probe per (device, dtype)
    again = client_stats._probe_adam_form(dev, DTYPES[key])          # and a second probe finds the same
    assert again["form"] == found["form"] and again["off"] == found["off"]


def test_a_dtype_without_a_form_is_refused_under_fused_and_torch_under_auto(dev, monkeypatch):
    """ADAM_DTYPES is what adam_form answers for: with bf16 taken out of it, a bf16 model has no form."""
    monkeypatch.setattr(client_stats, "ADAM_DTYPES", (torch.float32,))
    dt = torch.bfloat16
    assert client_stats.adam_form(dev, dt) is None
    p = torch.nn.Parameter(torch.full((16,), 0.5, device=dev, dtype=dt))
    with pytest.raises(TypeError, match="step='fused' needs .*adam_form"):
        mfl_amd.ClientStepStats([p], step="fused", optimizer="adam", adam=dict(lr=0.001))
    assert mfl_amd.ClientStepStats([p], step="auto", optimizer="adam", adam=dict(lr=0.001)).step_mode == "torch"


def test_sgd_step_and_adam_step_are_kept_apart(dev):
    p = torch.nn.Parameter(torch.full((16,), 0.5, device=dev))
    p.grad = torch.ones(16, device=dev)
    adam = mfl_amd.ClientStepStats([p], step="fused", optimizer="adam", adam=dict(lr=0.25, weight_decay=0.0))
    sgd = mfl_amd.ClientStepStats([p], step="fused")
    assert adam.step_mode == sgd.step_mode == "fused"
    adam.begin(1.0)
    sgd.begin(1.0)
    with pytest.raises(RuntimeError, match="sgd_step.*optimizer='adam'"):
        adam.sgd_step(0.25, 0.5, 1.0)
    with pytest.raises(RuntimeError, match="adam_step.*optimizer='sgd'"):
        sgd.adam_step(0.5, 1.0)
    with pytest.raises(RuntimeError, match="after_step.*fused stepping"):
        adam.after_step(0.5, 1.0)
    version = p._version
    assert not adam.after_backward(torch.tensor(0.5, device=dev), 0.25, 1e9)
    adam.adam_step(0.5, 1.0)
    want = torch.nn.Parameter(torch.full((16,), 0.5, device=dev))
    want.grad = torch.ones(16, device=dev)
    torch.optim.Adam([want], lr=0.25, amsgrad=True).step()
    assert p._version > version and torch.equal(_bits(p.detach()), _bits(want.detach()))
    for fallback in (dict(lr=0.1, amsgrad=False), dict(lr=0.1, betas=(0.5, 0.999))):
        with pytest.raises(TypeError, match="step='fused' needs"):
            mfl_amd.ClientStepStats([p], step="fused", optimizer="adam", adam=fallback)
        assert mfl_amd.ClientStepStats([p], step="auto", optimizer="adam", adam=fallback).step_mode == "torch"
    frozen = torch.nn.Parameter(torch.zeros(4, device=dev), requires_grad=False)
    with pytest.raises(TypeError, match="step='fused' needs"):
        mfl_amd.ClientStepStats([p, frozen], step="fused", optimizer="adam", adam=dict(lr=0.1))


def _train(case, dev, dt, step):
    client, net = O.case_client(case, dev)
    client.args = types.SimpleNamespace(**{**vars(client.args), "client_optimizer": "adam", "wd": 0.001})
    if dt != torch.float32:
        x, labels = client.local_training_data[0]
        client.local_training_data = [(x.to(dt), labels)]
        net = net.to(dt)
    seen, syncs = [], []
    real = client_stats.ClientStepStats.result

    def counting(self):
        syncs.append(self.host_syncs)
        return real(self)

    client_stats.ClientStepStats.result = counting
    try:
        out = client_stats.client_train(client, net, case["meta"]["local_iteration"], stats="hip", step=step,
                                        trace=lambda stage, w, g, loss: seen.append((stage, w, g, loss)))
    finally:
        client_stats.ClientStepStats.result = real
    return out, seen, syncs


@pytest.mark.parametrize("key", KEYS)
def test_client_train_fused_equals_torch(dev, key, monkeypatch):
    """mlp_16x24x4_it4 with Adam: the traced weights after every iteration are bit-equal between step="fused" and
    step="torch", the stages (so the guard's decisions) are the same, rho and beta agree to 1e-6 relative (the rule
    test_gpu_client_step.py applies: the fused record's norms are exactly rounded, torch.norm's are not), one host
    sync per iteration, and under fused stepping no torch optimizer is built."""
    dt = DTYPES[key]
    case = O.load_client_case("mlp_16x24x4_it4")
    iters = case["meta"]["local_iteration"]
    (sd_t, loss_t, beta_t, rho_t, acc_t, _), seen_t, _ = _train(case, dev, dt, "torch")
    built = []
    real_adam = torch.optim.Adam
    monkeypatch.setattr(torch.optim, "Adam", lambda *a, **k: built.append(1) or real_adam(*a, **k))
    (sd_f, loss_f, beta_f, rho_f, acc_f, _), seen_f, syncs = _train(case, dev, dt, "fused")
    # fp16 rounds eps = 1e-8 to 0, so s3 = 0 where v is 0 and the weights turn NaN: the guard then trips in the
    # next iteration, under both kinds of stepping alike (result() and its sync are never reached)
    tripped = loss_t is None
    assert not tripped or key == "f16"
    assert built == [] and syncs == ([] if tripped else [iters])
    assert [s[0] for s in seen_f] == [s[0] for s in seen_t]
    assert tripped or len(seen_f) == 1 + 2 * iters
    assert sum(s[0] == "after_step" for s in seen_f) >= 1  # a fused step was taken and compared
    for i, (a, b) in enumerate(zip(seen_f, seen_t)):
        for j in (1, 2):  # the weights and the gradients at every stage, NaN where torch has NaN
            if a[j] is not None:
                nan = torch.isnan(b[j])
                assert torch.equal(torch.isnan(a[j]), nan) and torch.equal(_bits(a[j])[~nan], _bits(b[j])[~nan]), \
                    (i, a[0], j)
        assert a[3] == b[3] or (a[3] != a[3] and b[3] != b[3]), (i, a[0])  # and the loss
    print(f"{key}: beta {beta_f!r} torch {beta_t!r}; rho {rho_f!r} torch {rho_t!r}")
    assert loss_f == loss_t and acc_f == acc_t
    if not tripped:
        assert O.rel(beta_f, beta_t) <= 1e-6 and O.rel(rho_f, rho_t) <= 1e-6
        for k in sd_t:
            assert torch.equal(sd_f[k], sd_t[k]), k
    # the guard: the tripping cases trip under both, before any step
    for name in ("nan_input_trips", "tiny_weights_trip"):
        trips = O.load_client_case(name)
        for step in ("fused", "torch"):
            out, seen, _ = _train(trips, dev, dt, step)
            assert out[1:] == (None,) * 5 and [s[0] for s in seen] == ["begin", "after_backward"], (name, step)


def test_patch_passes_adam_through(dev):
    case = O.load_client_case("mlp_16x24x4_it4")
    client, net = O.case_client(case, dev)
    client.args = types.SimpleNamespace(**{**vars(client.args), "client_optimizer": "adam", "wd": 0.001})
    with client_stats.patch(type(client), step="fused", stats="hip"):
        out = client.train(net, 2)
    assert out[1] is not None and np.isfinite(out[1])
