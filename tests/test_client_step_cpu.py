"""The ``step`` argument of ClientStepStats / client_train / patch without a
GPU: the default, what CPU parameters and Adam get, the refusals that keep
``after_step()`` and ``sgd_step()`` apart, and the build description's two
tuples."""
import inspect
import types

import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import build, client_stats


def _params():
    p = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 12))
    p.grad = torch.ones(12)
    return [p]


def test_step_defaults_to_torch_in_all_three_signatures():
    for fn in (client_stats.ClientStepStats.__init__, client_stats.client_train, client_stats.patch):
        par = inspect.signature(fn).parameters["step"]
        assert par.default == "torch" and par.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert mfl_amd.ClientStepStats(_params()).step_mode == "torch"


def test_cpu_parameters_cannot_step_fused():
    with pytest.raises(TypeError, match="step='fused' needs .*contiguous parameters on one GPU.*sgd_form"):
        mfl_amd.ClientStepStats(_params(), step="fused")
    with pytest.raises(TypeError, match="step='fused' needs"):
        mfl_amd.ClientStepStats(_params(), stats="torch", step="fused")
    auto = mfl_amd.ClientStepStats(_params(), step="auto")
    assert auto.step_mode == "torch" and auto.mode == "torch"
    with pytest.raises(ValueError, match="step must be"):
        mfl_amd.ClientStepStats(_params(), step="hip")


def test_sgd_form_has_no_answer_without_a_kernel_or_a_gpu():
    assert client_stats.sgd_form("cuda", torch.int32) is None  # no kernel for the dtype: no probe either
    with pytest.raises(TypeError, match="needs a GPU"):
        client_stats.sgd_form("cpu", torch.float32)
    assert torch.float32 in client_stats.STEP_DTYPES and set(client_stats.STEP_DTYPES) <= set(client_stats.FUSED_DTYPES)


def test_sgd_step_on_an_object_built_for_torch_raises():
    stats = mfl_amd.ClientStepStats(_params(), step="auto")
    stats.begin(1.0)
    with pytest.raises(RuntimeError, match="sgd_step.*step='fused'"):
        stats.sgd_step(0.03, 0.5, 1.0)
    assert not stats.after_backward(torch.tensor(0.5), 0.03, 1e9)
    stats.after_step(0.5, 1.0)  # the torch path is untouched


def test_after_step_on_an_object_built_for_fused_stepping_raises():
    """The refusal reads ``step_mode`` alone, before any buffer: shown here on
    an object switched to "fused" by hand (a real one needs the GPU; the GPU
    tests repeat this on one)."""
    stats = mfl_amd.ClientStepStats(_params())
    stats.begin(1.0)
    stats.step_mode = "fused"
    with pytest.raises(RuntimeError, match="after_step.*fused stepping.*sgd_step"):
        stats.after_step(0.5, 1.0)


def _client(optimizer):
    case = O.load_client_case("mlp_16x24x4_it4")
    client, net = O.case_client(case, torch.device("cpu"))
    client.args = types.SimpleNamespace(**{**vars(client.args), "client_optimizer": optimizer})
    return case, client, net


def test_adam_raises_under_fused_and_steps_with_torch_under_auto():
    case, client, net = _client("adam")
    before = O.flat_of(net.parameters()).copy()
    with pytest.raises(TypeError, match="step='fused' needs .*client_optimizer is 'adam'"):
        client_stats.client_train(client, net, 2, step="fused")
    assert (O.flat_of(net.parameters()) == before).all()  # refused before anything ran
    out = client_stats.client_train(client, net, 2, step="auto")
    assert out[1] is not None and (O.flat_of(net.parameters()) != before).any()


def test_sgd_on_the_cpu_is_todays_path_under_auto_and_refused_under_fused():
    case, client, net = _client("sgd")
    with pytest.raises(TypeError, match="step='fused' needs"):
        client_stats.client_train(client, net, 2, step="fused")
    case, client, net = _client("sgd")
    want = client_stats.client_train(client, net, case["meta"]["local_iteration"])
    case, client, net = _client("sgd")
    got = client_stats.client_train(client, net, case["meta"]["local_iteration"], step="auto")
    assert got[1:4] == want[1:4]
    for k in want[0]:
        assert torch.equal(got[0][k], want[0][k]), k


def test_patch_passes_step_through():
    case, client, net = _client("adam")
    with client_stats.patch(type(client), step="fused"):
        with pytest.raises(TypeError, match="step='fused' needs"):
            client.train(net, 1)
    with client_stats.patch(type(client), step="auto"):
        assert client.train(net, 1)[1] is not None


def test_the_build_description_keeps_five_and_covers_six():
    assert len(build.LIBS) == 5 and len(build.ALL_LIBS) == 6
    assert [lib.key for lib in build.ALL_LIBS][-1] == "clientstep" and set(build.BY_KEY) == {lib.key for lib in build.ALL_LIBS}
    assert (build.LIB_PATH, build.PROBE_LIB_PATH, build.FUSEDVEC_LIB_PATH, build.SEGVEC_LIB_PATH,
            build.CLIENTVEC_LIB_PATH) == tuple(lib.path for lib in build.LIBS)
