"""Every client's evaluation in one call (``fedavg_client_eval_f32``, ``cohort_test``, ``local_test_all``) against
``x @ W.T + b``, the sigmoid where asked, ``cross_entropy(reduction='sum')`` and ``argmax`` in fp64 torch on the CPU.
Per client: the total, the correct count exactly (the reference's smallest top-two gap is first held to 1e-5; fp32
error in an activation is near 3e-7), and the loss sum's relative deviation within LOSS_BOUND = 4x the largest
deviation of the existing fp32 path (``Client.local_test``'s torch expressions on the GPU, ``criterion(pred, y).item()
* B``) from the same reference over the same CASES x both activations (MI355X, torch 2.10 / ROCm 7.0)."""
import functools
import math
import sys
import types

import numpy as np
import pytest
import torch

from mfl_amd import EvalSet, _lib, cohort_test, local_test_all
from test_gpu_cohort import COHORTS, cohort_inputs
from test_gpu_linear_stream import DEV, Net

pytestmark = pytest.mark.gpu

# measured over CASES x both activations; set by the last case's B = 1 clients under "none", whose loss is a single
# small number (this kernel's largest deviation over the same cases is the same 7.828e-7, on the same client)
EXISTING_PATH_DEVIATION = 7.828e-7
LOSS_BOUND = 4 * EXISTING_PATH_DEVIATION
# (Bs, D, C, seed).  The kernel's edges: row tiles of 16 rows, 64 rows per wave, chunks of 256 rows (4 waves); the
# sixth has D % 16 == 0 and one long client, the seventh many chunks and D % 16 != 0, the eighth each edge - 1, + 0,
# + 1 and two chunks plus one row with D % 4 != 0 (single-float loads), the last more chunks (1200) than the
# persistent grid holds workgroups (3 per CU at 143 registers, 768 in all), so workgroups wrap around
CASES = [(*c, 0) for c in COHORTS] + [
    ((1, 15, 16, 17, 127, 128, 129, 1000), 784, 10, 0), ((2049, 3, 512), 20, 7, 0),
    ((63, 64, 65, 255, 256, 257, 511, 512, 513), 37, 5, 0), (tuple(1 + k % 3 for k in range(1200)), 5, 2, 0)]
PARAMS = [(n, act) for n in range(len(CASES)) for act in ("none", "sigmoid")]


def reference(W, b, x, y, activation):
    """(loss sum, correct count, smallest top-two gap) in fp64 on the CPU."""
    a = x.double().flatten(1) @ W.double().t() + b.double()
    a = torch.sigmoid(a) if activation == "sigmoid" else a
    top = a.topk(2).values
    return (float(torch.nn.functional.cross_entropy(a, y, reduction="sum")), int((a.argmax(-1) == y).sum()),
            float((top[:, 0] - top[:, 1]).min()))


@functools.lru_cache(maxsize=None)
def case(n, activation):
    """The inputs of CASES[n] and their references, computed once."""
    Bs, D, C, seed = CASES[n]
    W, b, batches = cohort_inputs(Bs, D, C, seed)
    return W, b, batches, [reference(W, b, x, y, activation) for x, y in batches]


def eval_entry(W, b, xs, ys, activation, order=None):
    """The C entry on device tensors xs, ys, entry g = client order[g]: the [K, 4] records as int64 bits."""
    lib, K = _lib.load_clienteval(), len(xs)
    model = torch.cat([W.reshape(-1), b]).to(DEV)
    table = torch.tensor([[xs[k].data_ptr(), ys[k].data_ptr(), xs[k].shape[0], k] for k in order or range(K)]).pin_memory()
    need = lib.fedavg_client_eval_workspace_bytes(table.data_ptr(), K, W.shape[1])
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)  # dirty: nothing is read before it is written
    rec = torch.zeros(K, 4, dtype=torch.float64, pin_memory=True)
    name = "fedavg_client_eval_f32"
    _lib.check_clienteval(getattr(lib, name)(model.data_ptr(), table.data_ptr(), K, W.shape[1], W.shape[0],
                                             int(activation == "sigmoid"), rec.data_ptr(), ws.data_ptr(), need, None), name)
    torch.cuda.synchronize()
    return rec.view(torch.int64).clone()


def on_device(batches):
    return [x.to(DEV) for x, _ in batches], [y.to(DEV) for _, y in batches]


@pytest.mark.parametrize("n, activation", PARAMS)
def test_every_client_matches_the_fp64_reference(n, activation):
    W, b, batches, refs = case(n, activation)
    assert min(r[2] for r in refs) >= 1e-5  # what the inputs owe: no argmax within fp32 error of a tie
    xs, ys = on_device(batches)
    rec = eval_entry(W, b, xs, ys, activation)
    worst = 0.0
    for k, ((x, _), (loss, correct, _)) in enumerate(zip(batches, refs)):
        got = rec[k].view(torch.float64).tolist()
        worst = max(worst, abs(got[0] - loss) / abs(loss))
        assert got[1:] == [correct, 0, x.shape[0]], (k, got, correct)
    print(CASES[n][1:], activation, "largest relative loss deviation", worst)  # the figure before it is held
    assert worst <= LOSS_BOUND, (worst, LOSS_BOUND)  # false for a NaN as well
    assert torch.equal(rec, eval_entry(W, b, xs, ys, activation))  # equal inputs, equal bits
    assert torch.equal(rec, eval_entry(W, b, xs, ys, activation, list(reversed(range(len(xs))))))  # any table order
    net = Net(W, b, activation).to(DEV).train()
    res = cohort_test(net, EvalSet([[batch] for batch in batches], DEV), loop="linear_sigmoid" if activation == "sigmoid" else "linear")
    assert not net.training and torch.equal(net.linear.weight.cpu(), W) and torch.equal(net.linear.bias.cpu(), b)
    for k, m in enumerate(res):
        loss, correct, _, total = rec[k].view(torch.float64).tolist()
        assert m == {"test_correct": correct, "test_loss": loss, "test_total": total}
        assert [type(v) for v in m.values()] == [int, float, int]


def test_misaligned_x_takes_the_other_instance_and_leaves_the_same_bits():
    W, b, batches, _ = case(5, "sigmoid")
    xs, ys = on_device(batches)
    shifted = []
    for x in xs:
        buf = torch.empty(x.numel() + 4, device=DEV)
        shifted.append(buf[1:1 + x.numel()].view_as(x).copy_(x))  # a view one float into a larger buffer
    assert all(s.data_ptr() % 16 == 4 for s in shifted) and all(x.data_ptr() % 16 == 0 for x in xs)
    assert torch.equal(eval_entry(W, b, shifted, ys, "sigmoid"), eval_entry(W, b, xs, ys, "sigmoid"))


def test_a_nan_or_a_bad_label_in_one_client_touches_no_other():
    W, b, batches = cohort_inputs((17, 300, 33), 5, 10, 0)
    batches[1][0][299, 2] = math.nan
    batches[2][1][32] = 10
    xs, ys = on_device(batches)
    rec = eval_entry(W, b, xs, ys, "none").view(torch.float64)
    pred = batches[1][0] @ W.t() + b  # torch.max on the CPU: the first NaN wins
    assert math.isnan(rec[1, 0]) and rec[1, 1] == int(torch.max(pred, -1)[1].eq(batches[1][1]).sum()) and rec[1, 2] == 0
    assert rec[2, 2] == 1 and rec[2, 3] == 33 and not math.isnan(rec[2, 0])
    assert torch.equal(rec[0].view(torch.int64), eval_entry(W, b, xs[:1], ys[:1], "none")[0])
    with pytest.raises(IndexError, match=r"client 3: a label lies outside \[0, 10\)"):
        cohort_test(Net(W, b, "none").to(DEV), EvalSet([[batches[0]], None, [batches[1]], [batches[2]]], DEV))
    torch.cuda.synchronize()  # nothing faulted


def test_local_test_all_is_the_trainers_loop_on_the_reference_metrics():
    W, b, test = cohort_inputs((40, 300, 7, 65), 784, 10, 0)
    _, _, train = cohort_inputs((100, 257, 31, 16), 784, 10, 1)
    name = "_cohort_eval_trainer"
    mod = sys.modules[name] = types.ModuleType(name)
    mod.client_num_in_total, infos, logged = "5", [], []  # more than the trainer holds; a string, as argparse may leave it
    mod.logger, mod.wandb = types.SimpleNamespace(info=infos.append), types.SimpleNamespace(log=logged.append)
    trainer = type("FedAvgTrainer", (), {"__module__": name})()
    trainer.__dict__.update(client_num=4, invalid_datasets={3: "empty"}, time_counter=2.0, cycle_num=3, device=DEV,
                            test_data_local_dict={0: [test[0]], 1: None, 2: [test[2]], 3: [test[3]]},
                            train_data_local_dict={k: [train[k]] for k in range(4)})
    net = Net(W, b, "sigmoid").to(DEV).train()
    acc, train_acc = local_test_all(trainer, net, 7, eval_on_train=True, loop="linear_sigmoid")
    assert not net.training and torch.equal(net.linear.weight.cpu(), W) and torch.equal(net.linear.bias.cpu(), b)
    want = {w: [reference(W, b, *data[k], "sigmoid") for k in (0, 2)] for w, data in (("Test", test), ("Train", train))}
    total = {w: sum(data[k][0].shape[0] for k in (0, 2)) for w, data in (("Test", test), ("Train", train))}
    assert acc == sum(r[1] for r in want["Test"]) / total["Test"]
    assert np.array_equal(train_acc, np.array([r[1] for r in want["Train"]]) / np.array([100, 31]))
    stats = logged[-1]
    assert infos[-1] is stats and stats["round"] == 7 and stats["cum_time"] == 2.0 + 3 * 59361
    assert stats["Test/Acc"] == acc and stats["Train/Acc"] == sum(r[1] for r in want["Train"]) / total["Train"]
    for w in ("Test", "Train"):
        ref = sum(r[0] for r in want[w]) / total[w]
        assert abs(stats[w + "/Loss"] - ref) / ref <= LOSS_BOUND
    assert local_test_all(trainer, net, 8, if_log=False) == (acc, None) and len(logged) == 1  # the cached sets
    del sys.modules[name]
