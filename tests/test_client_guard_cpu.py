"""ClientStepStats(guard=...) without a GPU: the values the argument takes, the
refusal of guard="device" where the step is not fused, "auto" falling back to
the host guard, the methods of one mode refusing an object of the other, and
patch() / client_train() handing the argument on."""
import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import client_stats


def params():
    net = O.build_model({"sizes": [4, 3]})
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    return list(net.parameters())


def test_guard_takes_three_values_and_defaults_to_host():
    assert mfl_amd.ClientStepStats(params()).guard_mode == "host"
    assert mfl_amd.ClientStepStats(params(), guard="host").guard_mode == "host"
    for bad in ("gpu", "hip", None, 1):
        with pytest.raises(ValueError, match="guard must be 'host', 'device' or 'auto'"):
            mfl_amd.ClientStepStats(params(), guard=bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="ahead must be a positive integer"):
            mfl_amd.ClientStepStats(params(), ahead=bad)
    assert mfl_amd.DEFAULT_AHEAD == client_stats.DEFAULT_AHEAD and client_stats.DEFAULT_AHEAD >= 1


def test_device_guard_needs_fused_stepping_and_names_the_rule():
    for kwargs in (dict(), dict(step="torch"), dict(step="auto"), dict(step="auto", optimizer="adam",
                                                                      adam=dict(lr=0.001))):
        with pytest.raises(TypeError, match="guard='device' needs fused stepping"):
            mfl_amd.ClientStepStats(params(), guard="device", **kwargs)


def test_auto_falls_back_to_the_host_guard():
    for kwargs in (dict(), dict(step="auto"), dict(step="auto", optimizer="adam", adam=dict(lr=0.001))):
        t = mfl_amd.ClientStepStats(params(), guard="auto", **kwargs)
        assert t.guard_mode == "host" and t.step_mode == "torch"


def test_the_device_guards_methods_refuse_a_host_guard_object():
    t = mfl_amd.ClientStepStats(params(), guard="auto")
    t.begin(1.0)
    loss = torch.tensor(0.5)
    for call, name in ((lambda: t.guarded_step(loss, 0.1, 10.0), "guarded_step"), (t.poll, "poll"),
                       (t.finish, "finish")):
        with pytest.raises(RuntimeError, match=rf"{name}\(\) needs an object built with guard='device'"):
            call()
    assert t.after_backward(loss, 0.1, 1e9) is False  # and the host guard's own method still serves it


def test_after_backward_refuses_a_device_guard_object():
    t = mfl_amd.ClientStepStats(params())
    t.begin(1.0)
    t.guard_mode = "device"  # what a GPU object built with guard="device" says
    with pytest.raises(RuntimeError, match=r"after_backward\(\) on an object built with guard='device'"):
        t.after_backward(torch.tensor(0.5), 0.1, 10.0)


def test_begin_under_the_device_guard_takes_a_tensor():
    t = mfl_amd.ClientStepStats(params())
    t.guard_mode = "device"
    with pytest.raises(TypeError, match="takes the prologue's loss tensor"):
        t.begin(1.0)


def test_patch_and_client_train_hand_the_argument_on(monkeypatch):
    case = O.load_client_case("linear_20x5_it3")
    client, net = O.case_client(case, torch.device("cpu"))
    seen = []
    monkeypatch.setattr(client_stats, "client_train", lambda self, net, it, **kw: seen.append(kw) or "ran")
    with client_stats.patch(type(client), guard="device", step="fused"):
        assert client.train(net, 3) == "ran"
    with client_stats.patch(type(client)):
        client.train(net, 3)
    assert [kw["guard"] for kw in seen] == ["device", "host"] and seen[0]["step"] == "fused"
    monkeypatch.undo()
    # client_train itself: refused by the constructor before anything runs; "auto" runs as the host guard does
    with pytest.raises(TypeError, match="guard='device' needs fused stepping"):
        client_stats.client_train(client, net, 3, guard="device")
    with pytest.raises(ValueError, match="guard must be"):
        client_stats.client_train(client, net, 3, guard="gpu")
    out = client_stats.client_train(client, net, 3, guard="auto")
    assert (out[2], out[3]) == (float(case["ret"][1]), float(case["ret"][2]))
