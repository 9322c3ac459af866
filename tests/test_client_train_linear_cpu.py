"""client_train(loop="linear"): the TypeError of every rule the host checks, raised before anything runs (CPU
tensors; the step-form rule needs the GPU's probe and is not reached here)."""
import pytest
import torch

from linear_loop_ref import make_client
from mfl_amd import client_stats


class Net(torch.nn.Module):
    def __init__(self, *params):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p, requires_grad=p.dtype.is_floating_point)
                                          for p in params])


def client(x, y, criterion=None):
    return make_client(x, y, torch.device("cpu"), "sgd", 0.05, 0.0, 1e3, criterion)


W, B_, X, Y = torch.zeros(10, 20), torch.zeros(10), torch.zeros(8, 4, 5), torch.zeros(8, dtype=torch.int64)
CE = torch.nn.CrossEntropyLoss


@pytest.mark.parametrize("params, x, y, criterion, words", [
    ((W,), X, Y, None, "1 parameters, not two"),
    ((W.double(), B_), X, Y, None, "no contiguous fp32 [C, D] weight"),
    ((W.t(), B_), X, Y, None, "no contiguous fp32 [C, D] weight"),
    ((W, torch.zeros(9)), X, Y, None, "no contiguous fp32 [C] bias"),
    ((W, B_), torch.zeros(8, 21), Y, None, "no fp32 batch of 20 columns"),
    ((W, B_), X, Y.int(), None, "not int64 of length 8"),
    ((W, B_), X, Y, CE(reduction="sum"), "no default nn.CrossEntropyLoss"),
    ((W, B_), X, Y, CE(weight=torch.ones(10)), "no default nn.CrossEntropyLoss"),
    ((W, B_), X, Y, CE(label_smoothing=0.1), "no default nn.CrossEntropyLoss"),
    ((torch.zeros(17, 20), torch.zeros(17)), X, Y, None, "lie outside"),
    ((W, B_), X, Y, None, "not on one GPU"),
])
def test_each_host_rule_is_a_type_error(params, x, y, criterion, words):
    net = Net(*params)
    before = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(TypeError) as info:
        client_stats.client_train(client(x, y, criterion), net, 3, loop="linear")
    assert words in str(info.value) and "loop='linear'" in str(info.value)
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), before))


def test_an_unknown_loop_is_a_value_error_and_zero_iterations_take_the_torch_path():
    with pytest.raises(ValueError, match="loop must be"):
        client_stats.client_train(client(X, Y), Net(W, B_), 3, loop="eager")
    with pytest.raises(UnboundLocalError):  # client.py:93 reads log_probs, which no iteration bound
        client_stats.client_train(client(X.flatten(1), Y), torch.nn.Linear(20, 10), 0, loop="linear")
