"""ClientStepStats(guard="device") on the MI355X against guard="host".

The whole loop driven by hand with seeded gradients, on one nn.Linear(7, 3)
and on a model of three odd-sized tensors, SGD and Adam, fp32 / bf16 / fp64:
parameters and Adam state after every iteration, (beta, rho) and the final
loss bit for bit, one host sync against seven; then iteration 3 poisoned three
ways (a NaN gradient, a gradient past the bound, a NaN loss): finish() and
poll() report epoch 3 and the parameters are those of the host-guard run that
stopped there, with a ring of 1 and of 4.

client_train end to end on a stub Client: all six return values equal under
both guards, and the tripping fixtures return five None and the host guard's
parameters."""
import itertools
import math
import sys
import types

import numpy as np
import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import client_stats

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
MODELS = {"linear": [(3, 7), (3,)], "odd": [(4099,), (9, 7), (1,)]}
ITERS, LR, RATIO = 6, 0.05, 1000.0
ADAM = dict(lr=0.01, weight_decay=0.001, amsgrad=True)
LOSSES = [2.5, 2.25, 1.75, 1.5, 1.375, 1.25, 1.1875]  # the prologue's and six iterations': exact in bf16


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def seeded(model, key, dev):
    """(initial parameters, gradients of the prologue and of every iteration), seeded."""
    rng = np.random.default_rng(sum(map(ord, model + key)))
    dt = DTYPES[key]
    make = lambda scale: [torch.from_numpy(rng.normal(0.0, scale, s)).to(dt).to(dev) for s in MODELS[model]]  # noqa: E731
    return make(0.3), [make(1.0) for _ in range(ITERS + 1)]


def poisoned(grads, losses, how, dt):
    grads = [[g.clone() for g in gs] for gs in grads]
    losses = list(losses)
    if how == "nan_grad":
        grads[4][0].view(-1)[2] = math.nan  # grads[0] is the prologue's: iteration 3 is grads[4]
    elif how == "large_grad":
        grads[4] = [g * 4096.0 for g in grads[4]]
    elif how == "nan_loss":
        losses[4] = math.nan
    return grads, losses


def run(dev, key, model, optimizer, guard, grads, losses, w0, ahead=None, poll_after_sync=False):
    """Drive one ClientStepStats by hand; returns what the run left behind."""
    dt = DTYPES[key]
    params = [torch.nn.Parameter(w.clone()) for w in w0]
    kwargs = dict(optimizer="adam", adam=ADAM) if optimizer == "adam" else {}
    t = mfl_amd.ClientStepStats(params, stats="hip", step="fused", guard=guard, ahead=ahead, **kwargs)
    assert t.step_mode == "fused" and t.guard_mode == guard

    def give(gs):
        for p, g in zip(params, gs):
            p.grad = g.clone()

    def snapshot():
        state = t._step.state.clone() if optimizer == "adam" else None
        return [p.detach().clone() for p in params], state

    loss_of = lambda i: torch.tensor(losses[i], dtype=dt, device=dev)  # noqa: E731
    give(grads[0])
    out = types.SimpleNamespace(snaps=[], trip=None, polled=None)
    if guard == "device":
        t.begin(loss_of(0))
        for i in range(ITERS):
            give(grads[i + 1])
            t.guarded_step(loss_of(i + 1), LR, RATIO)
            out.snaps.append(snapshot())
        if poll_after_sync:
            torch.cuda.synchronize(dev)
            out.polled = t.poll()
        out.trip, out.loss, out.beta, out.rho = t.finish()
    else:
        t.begin(losses[0])
        last = losses[0]
        for i in range(ITERS):
            give(grads[i + 1])
            if t.after_backward(loss_of(i + 1), LR, RATIO):
                out.trip = i
                break
            loss = t.loss
            if optimizer == "adam":
                t.adam_step(loss, last)
            else:
                t.sgd_step(LR, loss, last)
            last = loss
            out.snaps.append(snapshot())
        out.loss = t.loss
        out.beta, out.rho = t.result()
    out.final = snapshot()
    out.host_syncs = t.host_syncs
    out.tracker = t
    return out


def assert_same_state(a, b, what):
    (pa, sa), (pb, sb) = a, b
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert same(x, y), (what, "parameter", i)
    assert (sa is None) == (sb is None)
    if sa is not None:
        assert same(sa, sb), (what, "adam state")


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
@pytest.mark.parametrize("model", tuple(MODELS))
@pytest.mark.parametrize("key", tuple(DTYPES))
def test_device_guard_equals_host_guard_bit_for_bit(dev, key, model, optimizer):
    w0, grads = seeded(model, key, dev)
    host = run(dev, key, model, optimizer, "host", grads, LOSSES, w0)
    device = run(dev, key, model, optimizer, "device", grads, LOSSES, w0, poll_after_sync=True)
    assert host.trip is None and device.trip is None and device.polled is None
    assert len(host.snaps) == len(device.snaps) == ITERS
    for i in range(ITERS):  # every prefix of the loop
        assert_same_state(host.snaps[i], device.snaps[i], i + 1)
    assert not same(host.snaps[0][0][0], w0[0])  # and the steps did step
    print(f"{key} {model} {optimizer}: beta {device.beta!r} rho {device.rho!r} loss {device.loss!r}")
    assert (device.beta, device.rho, device.loss) == (host.beta, host.rho, host.loss)
    assert device.beta is not None and device.rho is not None and device.loss == LOSSES[-1]
    assert device.host_syncs == 1 and host.host_syncs == ITERS + 1


@pytest.mark.parametrize("how", ("nan_grad", "large_grad", "nan_loss"))
@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
@pytest.mark.parametrize("key", tuple(DTYPES))
def test_a_trip_at_iteration_3_stops_the_steps_there(dev, key, optimizer, how):
    for model in MODELS:
        w0, grads = seeded(model, key, dev)
        grads, losses = poisoned(grads, LOSSES, how, DTYPES[key])
        host = run(dev, key, model, optimizer, "host", grads, losses, w0)
        assert host.trip == 3 and len(host.snaps) == 3
        finals = []
        for ahead in (1, 4):
            device = run(dev, key, model, optimizer, "device", grads, losses, w0, ahead=ahead, poll_after_sync=True)
            assert device.polled == 3 and device.trip == 3, (model, ahead)
            assert_same_state(host.final, device.final, (model, ahead))
            for i in range(ITERS):  # iterations 0-2 stepped, 3-5 wrote nothing
                assert_same_state(host.snaps[min(i, 2)], device.snaps[i], (model, ahead, i))
            assert (device.beta, device.rho) == (host.beta, host.rho)
            assert device.host_syncs == 1 and device.tracker.ring_waits == (ITERS - 1 if ahead == 1 else ITERS - 4)
            assert device.loss is None
            finals.append(device.final)
        assert_same_state(finals[0], finals[1], model)


def test_poll_never_blocks_and_reads_in_order(dev):
    w0, grads = seeded("linear", "f32", dev)
    params = [torch.nn.Parameter(w.clone()) for w in w0]
    t = mfl_amd.ClientStepStats(params, stats="hip", step="fused", guard="device", ahead=2)
    assert t.ahead == 2 and mfl_amd.ClientStepStats(params, step="fused", guard="device").ahead == mfl_amd.DEFAULT_AHEAD
    for p, g in zip(params, grads[0]):
        p.grad = g.clone()
    t.begin(torch.tensor(1.0, device=dev))
    assert t.poll() is None and t.finish() == (None, None, None, None)  # nothing queued yet
    t.guarded_step(torch.tensor(math.nan, device=dev), LR, RATIO)
    torch.cuda.synchronize(dev)
    assert t.poll() == 0 and t.poll() == 0
    with pytest.raises(RuntimeError, match="guarded_step\\(\\) takes its step"):
        t.sgd_step(LR, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="after_backward\\(\\) on an object built with guard='device'"):
        t.after_backward(torch.tensor(1.0, device=dev), LR, RATIO)


# ------------------------------------------------------------------ client_train end to end
def _train(case, dev, dt, optimizer, guard):
    client, net = O.case_client(case, dev)
    client.args = types.SimpleNamespace(**{**vars(client.args), "client_optimizer": optimizer, "wd": 0.001})
    if dt != torch.float32:
        x, labels = client.local_training_data[0]
        client.local_training_data = [(x.to(dt), labels)]
        net = net.to(dt)
    mod = sys.modules[type(client).__module__]
    ticks = itertools.count(0, 5)
    real = mod.count, mod.count_end
    mod.count = mod.count_end = lambda: next(ticks)  # a clock both runs read alike
    try:
        return client_stats.client_train(client, net, case["meta"]["local_iteration"], stats="hip", step="fused",
                                         guard=guard, keep_on_device=True)
    finally:
        mod.count, mod.count_end = real


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
@pytest.mark.parametrize("key", ("f32", "bf16"))
def test_client_train_returns_the_host_guards_six_values(dev, key, optimizer):
    dt = DTYPES[key]
    case = O.load_client_case("mlp_16x24x4_it4")
    host = _train(case, dev, dt, optimizer, "host")
    device = _train(case, dev, dt, optimizer, "device")
    print(f"{key} {optimizer}: host {host[1:]} device {device[1:]}")
    assert host[1] is not None and device[1:] == host[1:]
    for k in host[0]:
        assert same(device[0][k], host[0][k]), k
    for name in ("nan_input_trips", "tiny_weights_trip"):
        trips = O.load_client_case(name)
        host, device = (_train(trips, dev, dt, optimizer, guard) for guard in ("host", "device"))
        assert host[1:] == (None,) * 5 and device[1:] == (None,) * 5, name
        for k in host[0]:
            nan = torch.isnan(host[0][k])
            assert torch.equal(torch.isnan(device[0][k]), nan) and same(device[0][k][~nan], host[0][k][~nan]), (name, k)


def test_client_train_logs_the_trip_epoch_and_patch_plumbs_the_guard(dev):
    case = O.load_client_case("tiny_weights_trip")
    client, net = O.case_client(case, dev)
    mod = sys.modules[type(client).__module__]
    said = []
    mod.logger = types.SimpleNamespace(warning=said.append)
    try:
        with client_stats.patch(type(client), step="fused", stats="hip", guard="device", keep_on_device=True):
            out = client.train(net, case["meta"]["local_iteration"])
    finally:
        del mod.logger
    assert out[1:] == (None,) * 5 and said == ["grads too large than weights or meets nan with epoch 0"]
