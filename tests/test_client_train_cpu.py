"""client_stats on the CPU: the torch fallback of client_train reproduces the
reference's ``Client.train`` tuple on every fixture (same torch expressions on
the same kind of host: exact equality), patch / undo, and the argument checks
of the two C entries (they run before any HIP call)."""
import numpy as np
import pytest
import torch

import client_stats_oracle as O
import mfl_amd
from mfl_amd import _lib, build, client_stats

CASES = O.client_case_names()


@pytest.mark.parametrize("name", CASES)
def test_client_train_torch_fallback_equals_reference(name):
    case = O.load_client_case(name)
    meta = case["meta"]
    client, net = O.case_client(case, torch.device("cpu"))
    seen = []
    out = client_stats.client_train(client, net, meta["local_iteration"],
                                    trace=lambda stage, w, g, loss: seen.append(stage))
    sd, loss, beta, rho, acc, cycles = out
    assert O.flat_of(sd.values()).tobytes() == case["w_final"].tobytes()  # the state_dict, bit for bit
    if meta["tripped"]:
        assert (loss, beta, rho, acc, cycles) == (None,) * 5
        assert seen == ["begin", "after_backward"]
        return
    ref_loss, ref_beta, ref_rho, ref_acc = (float(v) for v in case["ret"])
    assert (loss, acc) == (ref_loss, ref_acc)
    assert (beta, rho) == (ref_beta, ref_rho)
    assert cycles > 0
    assert seen == ["begin"] + ["after_backward", "after_step"] * meta["local_iteration"]


def test_auto_takes_the_torch_path_on_cpu_and_for_non_fp32():
    net = O.build_model({"sizes": [4, 3]})
    assert mfl_amd.ClientStepStats(net.parameters()).mode == "torch"
    assert mfl_amd.ClientStepStats(net.double().parameters()).mode == "torch"
    with pytest.raises(TypeError):
        mfl_amd.ClientStepStats(net.parameters(), stats="hip")
    with pytest.raises(ValueError):
        mfl_amd.ClientStepStats(net.parameters(), stats="eager")


def test_none_grad_raises():
    net = O.build_model({"sizes": [4, 3]})
    with pytest.raises(RuntimeError, match="no grad"):
        mfl_amd.ClientStepStats(net.parameters()).begin(0.0)


def test_zero_local_iterations_raise_as_the_reference_does():
    case = O.load_client_case("linear_20x5_it1")
    client, net = O.case_client(case, torch.device("cpu"))
    with pytest.raises(UnboundLocalError):  # client.py:93 reads log_probs, which no iteration bound
        client_stats.client_train(client, net, 0)


def test_patch_and_undo_restore_the_class():
    case = O.load_client_case("linear_20x5_it3")
    client, net = O.case_client(case, torch.device("cpu"))
    cls = type(client)
    original = cls.__dict__["train"]
    handle = client_stats.patch(cls)
    assert cls.__dict__["train"] is not original
    out = client.train(net, case["meta"]["local_iteration"])
    assert (out[2], out[3]) == (float(case["ret"][1]), float(case["ret"][2]))
    handle.undo()
    assert cls.__dict__["train"] is original
    handle.undo()  # idempotent
    assert cls.__dict__["train"] is original

    class Sub(cls):  # a class that inherits train gets it back by deletion
        pass

    with client_stats.patch(Sub):
        assert "train" in vars(Sub)
    assert "train" not in vars(Sub) and Sub.train is original


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _stats_args(n_keys=2, P=16, ws=64, parts=6, snap=1024, ptrs=(4096, 8192), numel=(5, 7), offset=(0, 8)):
    keep = [np.array(ptrs, np.int64), np.array(numel, np.int64), np.array(offset, np.int64)]
    buf = np.zeros(64, np.float64)  # a host address where only non-null matters (rejected before any use)
    args = [keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, n_keys, snap, P, 1, buf.ctypes.data,
            parts, buf.ctypes.data, 4096, 8192, ws, None]
    return args, keep + [buf]


def test_stats_sizes_without_gpu(lib):
    numel = np.array([1, 0, 4096, 4097, 3 * 4096 + 5], np.int64)
    assert lib.fedavg_client_stats_partials(numel.ctypes.data, len(numel)) == 3 * (1 + 0 + 1 + 2 + 4)
    assert lib.fedavg_client_stats_partials(None, 3) == 0
    assert lib.fedavg_client_stats_workspace(5) == 5 * 32 and lib.fedavg_client_stats_workspace(0) == 0


@pytest.mark.parametrize("change,code", [
    (dict(n_keys=-1), "EINVAL"),
    (dict(P=-1), "EINVAL"),
    (dict(ws=63), "EINVAL"),               # workspace too small for 2 keys
    (dict(parts=5), "EINVAL"),             # partials too small for 2 units
    (dict(snap=1028), "EALIGN"),           # snapshot not 16-B aligned
    (dict(offset=(0, 6)), "EALIGN"),       # snapshot key offset not a multiple of 4
    (dict(offset=(0, 12)), "EINVAL"),      # key runs past P
    (dict(ptrs=(4096, 8194)), "EINVAL"),   # tensor not 4-B aligned
    (dict(ptrs=(0, 8192)), "EINVAL"),      # null tensor
    (dict(snap=None), "EINVAL"),
])
def test_stats_rejects_bad_arguments_without_gpu(lib, change, code):
    args, keep = _stats_args(**change)
    rc = lib.fedavg_client_stats_f32(*args)
    assert rc == getattr(_lib, "FEDAVG_" + code), lib.fedavg_last_error()
    assert lib.fedavg_last_error().startswith(b"fedavg_client_stats_f32")


def test_stats_null_tables_and_buffers_rejected(lib):
    for idx in (0, 1, 2, 7, 9, 10, 11):  # cur_ptrs, key_numel, key_offset, partials, stats, host_ws, dev_ws
        args, keep = _stats_args()
        args[idx] = None
        assert lib.fedavg_client_stats_f32(*args) == _lib.FEDAVG_EINVAL, idx


def test_track_rejects_bad_arguments_without_gpu(lib):
    buf = np.zeros(8, np.float64)
    p = buf.ctypes.data
    assert lib.fedavg_client_track(None, p, p, 0.5, None) == _lib.FEDAVG_EINVAL
    assert lib.fedavg_client_track(p, None, p, 0.5, None) == _lib.FEDAVG_EINVAL
    assert lib.fedavg_client_track(p, p, None, 0.5, None) == _lib.FEDAVG_EINVAL
    assert lib.fedavg_last_error().startswith(b"fedavg_client_track")
    assert lib.fedavg_client_track(p + 4, p, p, 0.5, None) == _lib.FEDAVG_EALIGN
    # host memory is not device memory: refused before any launch
    assert lib.fedavg_client_track(p, p, p, 0.5, None) == _lib.FEDAVG_EINVAL
