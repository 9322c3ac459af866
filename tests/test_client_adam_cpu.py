"""The ``optimizer`` / ``adam`` arguments of ClientStepStats and what
client_train / patch do for ``client_optimizer="adam"`` without a GPU: the
defaults, the refusals and fall-backs, ``sgd_step()`` and ``adam_step()`` kept
apart, the coefficients as torch forms them."""
import inspect
import types

import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import client_stats


def _params():
    p = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 12))
    p.grad = torch.ones(12)
    return [p]


def test_the_new_keywords_default_to_sgd_and_none():
    par = inspect.signature(client_stats.ClientStepStats.__init__).parameters
    assert par["optimizer"].default == "sgd" and par["adam"].default is None
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("optimizer", "adam"))
    stats = mfl_amd.ClientStepStats(_params())
    assert stats.optimizer == "sgd" and stats.adam is None and stats.step_mode == "torch"
    with pytest.raises(ValueError, match="optimizer must be"):
        mfl_amd.ClientStepStats(_params(), optimizer="rmsprop")
    with pytest.raises(ValueError, match="optimizer='adam' needs adam=dict"):
        mfl_amd.ClientStepStats(_params(), optimizer="adam")
    with pytest.raises(ValueError, match="unknown keys"):
        mfl_amd.ClientStepStats(_params(), optimizer="adam", adam=dict(lr=0.1, momentum=0.9))
    filled = mfl_amd.ClientStepStats(_params(), optimizer="adam", adam=dict(lr=0.1)).adam
    assert filled == dict(lr=0.1, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=True)


def test_exports_and_dtypes():
    assert mfl_amd.adam_form is client_stats.adam_form and mfl_amd.ADAM_DTYPES is client_stats.ADAM_DTYPES
    assert set(client_stats.ADAM_DTYPES) <= set(client_stats.FUSED_DTYPES)
    assert client_stats.adam_form("cuda", torch.int32) is None  # no kernel for the dtype: no probe either
    with pytest.raises(TypeError, match="needs a GPU"):
        client_stats.adam_form_probe("cpu", torch.float32)


def test_cpu_parameters_cannot_step_fused_with_adam_and_fall_back_under_auto():
    for adam in (dict(lr=0.1), dict(lr=0.1, amsgrad=False), dict(lr=0.1, betas=(0.5, 0.999))):
        with pytest.raises(TypeError, match="step='fused' needs .*contiguous parameters on one GPU.*adam_form"):
            mfl_amd.ClientStepStats(_params(), step="fused", optimizer="adam", adam=adam)
        auto = mfl_amd.ClientStepStats(_params(), step="auto", optimizer="adam", adam=adam)
        assert auto.step_mode == "torch" and auto.mode == "torch"


def test_adam_step_and_sgd_step_on_objects_built_for_torch_raise():
    stats = mfl_amd.ClientStepStats(_params(), step="auto", optimizer="adam", adam=dict(lr=0.1))
    stats.begin(1.0)
    with pytest.raises(RuntimeError, match="adam_step.*step='fused'"):
        stats.adam_step(0.5, 1.0)
    with pytest.raises(RuntimeError, match="sgd_step.*step='fused'"):
        stats.sgd_step(0.03, 0.5, 1.0)
    assert not stats.after_backward(torch.tensor(0.5), 0.03, 1e9)
    stats.after_step(0.5, 1.0)  # the torch path is untouched


def test_each_step_refuses_an_object_built_for_the_other():
    """The refusals read ``step_mode`` and ``optimizer`` alone, before any buffer: shown on objects switched to
    "fused" by hand (real ones need the GPU; the GPU tests repeat this on those)."""
    adam = mfl_amd.ClientStepStats(_params(), optimizer="adam", adam=dict(lr=0.1))
    sgd = mfl_amd.ClientStepStats(_params())
    for s in (adam, sgd):
        s.begin(1.0)
        s.step_mode = "fused"
    with pytest.raises(RuntimeError, match="sgd_step.*optimizer='adam'.*adam_step"):
        adam.sgd_step(0.03, 0.5, 1.0)
    with pytest.raises(RuntimeError, match="adam_step.*optimizer='sgd'.*sgd_step"):
        sgd.adam_step(0.5, 1.0)


def test_coefficients_are_formed_as_adam_py_forms_them():
    lr, b1, b2, eps, wd = 0.001, 0.9, 0.999, 1e-8, 0.001
    for t in (1, 2, 3, 100):
        c = client_stats.adam_coef(lr, b1, b2, eps, wd, t)
        step = float(t)
        assert c.tolist() == [wd, 1 - b1, b2, 1 - b2, (1 - b2 ** step) ** 0.5, eps, (lr / (1 - b1 ** step)) * -1]


def _client(optimizer):
    case = O.load_client_case("mlp_16x24x4_it4")
    client, net = O.case_client(case, torch.device("cpu"))
    client.args = types.SimpleNamespace(**{**vars(client.args), "client_optimizer": optimizer, "wd": 0.001})
    return case, client, net


def test_client_train_with_adam_on_the_cpu():
    case, client, net = _client("adam")
    before = O.flat_of(net.parameters()).copy()
    with pytest.raises(TypeError, match="step='fused' needs .*adam_form.*client_optimizer is 'adam'"):
        client_stats.client_train(client, net, 2, step="fused")
    assert (O.flat_of(net.parameters()) == before).all()  # refused before anything ran
    want = client_stats.client_train(client, net, 2)
    case, client, net = _client("adam")
    got = client_stats.client_train(client, net, 2, step="auto")  # torch's Adam, as without the argument
    assert got[1:4] == want[1:4] and got[1] is not None
    for k in want[0]:
        assert torch.equal(got[0][k], want[0][k]), k
