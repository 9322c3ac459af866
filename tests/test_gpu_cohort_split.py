"""A round's cohort with each client's batch split across workgroups (``fedavg_client_cohort_split_f32``,
``cohort_train(split=True)``): every client against the loop of client.py:52-96 in fp64 torch on the CPU
(linear_loop_ref.py) at the batch sizes at which slicing can go wrong; alone and in company, bit for bit; one client's
NaN or bad label touching no other; a guard that trips after the first epoch; the round's fused aggregate on the rows.
Bounds: 4x the largest deviation from the same reference of the existing fp32 path (``loop="torch"`` on the GPU, per
client, same inputs).  W and b: largest absolute difference; loss, beta, rho: relative difference."""
import functools
import math

import pytest
import torch

from linear_loop_ref import linear_loop_ref, make_client
from mfl_amd import ALIGN_ELEMS, _lib, client_stats, cohort_train, reduce_with_sqdist, sample_weights, weights_tensor
from mfl_amd.client_passes import adam_coef, cosplit_workspace_bytes, split_slice_rows
from test_gpu_linear_stream import DEV, HYPER, RATIO, Net, deviations

pytestmark = pytest.mark.gpu

ITERS = 3
# the fp32 torch loop's largest deviations over CASES, every client (torch 2.10.0 / ROCm 7.0, MI355X), times 4.  The
# split cohort's own largest over the same: w 1.479e-6, loss 9.490e-8, beta 2.538e-4, rho 2.665e-4.
BOUND = {"w": 4 * 1.982e-6, "loss": 4 * 1.228e-7, "beta": 4 * 2.962e-4, "rho": 4 * 8.848e-4}
# (D, C, [B_k] from R = split_slice_rows(D), x offset in floats): slices full, one row over or short, a one-row client,
# many slices; the range's corner; one partial slice; the staged path (D % 4 != 0; every x 4 B off a 16-B boundary)
COHORTS = [(784, 10, lambda R: [R, R + 1, 1, 2 * R + 1, 5 * R + 3], 0), (1024, 16, lambda R: [R - 1, 2 * R + 1], 0),
           (7, 2, lambda R: [1, 1, 5], 0), (250, 5, lambda R: [R + 6, 3], 0),
           (784, 10, lambda R: [R, R + 1, 1, 2 * R + 1, 5 * R + 3], 1)]
# q = 2 and q = 1 in turn: a workgroup with two slices, a client whose last workgroup has one
CASES = [(n, act, opt, 1 + (n + i + j) % 2) for n in range(len(COHORTS)) for i, act in enumerate(("none", "sigmoid"))
         for j, opt in enumerate(("sgd", "adam"))]
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(W, b, [(x, y)]) on the CPU.  x is scaled as test_gpu_client_split.inputs scales it; a client of fewer than four
    rows by a fifth of that, or lr |x|^2 fits its rows within the three steps and its loss collapses."""
    D, C, sizes, _ = COHORTS[n]
    g = torch.Generator().manual_seed(100 * n + 7 * D + 13 * C)
    W, b = torch.randn(C, D, generator=g) / math.sqrt(D), torch.randn(C, generator=g)
    return W, b, [((0.25 if B >= 4 else 0.05) * torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g))
                  for B in sizes(split_slice_rows(D))]


def on_device(batches, offset=0):
    """The batches on the GPU, every x ``offset`` floats past a 16-B boundary."""
    out = []
    for x, y in batches:
        flat = torch.empty(x.numel() + offset, device=DEV)
        flat[offset:] = x.reshape(-1)
        out.append((flat[offset:].view(x.shape), y.to(DEV)))
    return out


@functools.lru_cache(maxsize=None)
def reference(n, k, activation, optimizer, iters=ITERS):
    W, b, batches = inputs(n)
    return linear_loop_ref(W, b, *batches[k], iters=iters, activation=activation, optimizer=optimizer, ratio=RATIO,
                           **HYPER[optimizer])


def train(W, b, batches, activation, optimizer, q, iters=ITERS, ratio=RATIO, **kw):
    clients = [make_client(x, y, DEV, optimizer, ratio=ratio, **HYPER[optimizer]) for x, y in batches]
    net = Net(W, b, activation).to(DEV)
    res = cohort_train(clients, net, iters, loop="linear_sigmoid" if activation == "sigmoid" else "linear", split=True,
                       slices_per_group=q, **kw)
    assert torch.equal(net.linear.weight.cpu(), W) and torch.equal(net.linear.bias.cpu(), b)  # net is not modified
    return res


@pytest.mark.parametrize("case", CASES, ids=str)
def test_split_cohort_matches_the_fp64_reference_per_client(case):
    n, activation, optimizer, q = case
    W, b, batches = inputs(n)
    res = train(W, b, on_device(batches, COHORTS[n][3]), activation, optimizer, q)
    assert res.P == W.numel() + b.numel() and res.sample_numbers == [x.shape[0] for x, _ in batches]
    for k in range(len(batches)):
        ref = reference(n, k, activation, optimizer)
        # what the inputs owe: no trip, and a loss far from 0 at every epoch, so that no relative bound is vacuous
        assert ref["trip"] == -1 and max(ref["guard_ratio"]) <= 0.5
        assert min(reference(n, k, activation, optimizer, it)["loss"] for it in range(1, ITERS + 1)) > 0.05
        sd, (loss, beta, rho, acc) = res.state_dict(k, cpu=True), res.results[k]
        dev = deviations((sd["1.weight"], sd["1.bias"], loss, beta, rho, None), ref)
        print(case, k, dev)  # each figure before it is held to its bound
        for name, bound in BOUND.items():
            assert dev[name] <= bound, (k, name, dev[name], bound)  # false for a NaN as well
        if ref["top2_gap"] > 1e-3:
            assert round(acc * batches[k][0].shape[0]) == ref["correct"], k


def entry(W, b, batches, optimizer, q, order, iters=ITERS, lr_ratio=None):
    """The C entry on device batches, entry g = client order[g], row = the client's position: (rows incl. pad, records
    as int64, the 4096 bytes after the workspace, which no launch may touch)."""
    h, adam, K, P = HYPER[optimizer], optimizer == "adam", len(batches), W.numel() + b.numel()
    form = (client_stats.adam_form if adam else client_stats.sgd_form)(DEV, torch.float32)
    model = torch.cat([W.reshape(-1), b]).to(DEV)
    rows = torch.full((K, -(-P // ALIGN_ELEMS) * ALIGN_ELEMS), SENTINEL, device=DEV)
    table = torch.tensor([[batches[k][0].data_ptr(), batches[k][1].data_ptr(), batches[k][0].shape[0], k] for k in order]).pin_memory()
    rec = torch.zeros(K, 8, dtype=torch.float64, pin_memory=True)
    coef = torch.zeros(16, 7, dtype=torch.float64, pin_memory=True)
    for t in range(iters):
        coef[t] = torch.from_numpy(adam_coef(h["lr"], 0.9, 0.999, 1e-8, h["wd"], t + 1))
    nbytes = cosplit_workspace_bytes([batches[k][0].shape[0] for k in order], W.shape[1], W.shape[0], q, adam)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    name = "fedavg_client_cohort_split_f32"
    _lib.check_clientcosplit(getattr(_lib.load_clientcosplit(), name)(
        model.data_ptr(), rows.data_ptr(), rows.stride(0), table.data_ptr(), K, W.shape[1], W.shape[0], iters, 0,
        int(adam), h["lr"], h["lr"] * RATIO if lr_ratio is None else lr_ratio, form, coef.data_ptr(), rec.data_ptr(), q,
        ws.data_ptr(), nbytes, None), name)
    torch.cuda.synchronize()
    return rows.cpu().view(torch.int32), rec.view(torch.int64).clone(), ws[nbytes:].cpu()


@pytest.mark.parametrize("n, optimizer, q", [(0, "sgd", 2), (4, "adam", 1)])
def test_a_client_alone_and_in_company_leaves_the_same_bits(n, optimizer, q):
    W, b, batches = inputs(n)
    dev, K, P = on_device(batches, COHORTS[n][3]), len(batches), W.numel() + b.numel()
    rows, rec, tail = entry(W, b, dev, optimizer, q, list(range(K)))
    assert bool((rows[:, P:] == torch.tensor(SENTINEL).view(torch.int32)).all()) and bool((tail == 0xA5).all())
    assert rec.view(torch.float64)[:, 6].tolist() == [ITERS] * K
    for other in (entry(W, b, dev, optimizer, q, list(range(K))), entry(W, b, dev, optimizer, q, list(range(K))[::-1])):
        assert torch.equal(rows, other[0]) and torch.equal(rec, other[1])  # a second call; the table reversed
    for k in range(K):
        solo = entry(W, b, dev[k:k + 1], optimizer, q, [0])
        assert torch.equal(rows[k, :P], solo[0][0, :P]) and torch.equal(rec[k], solo[1][0]), k


def test_one_clients_trouble_stays_its_own():
    W, b, batches = inputs(0)
    R, dev, P = split_slice_rows(784), on_device(batches), W.numel() + b.numel()
    clean = entry(W, b, dev, "adam", 1, [4, 3, 2, 1, 0])
    dev[1][0][R, 5] = math.nan  # client 1's last row
    dev[3][1][R + 2] = 10       # C = 10, in client 3's second slice
    rows, rec, tail = entry(W, b, dev, "adam", 1, [4, 3, 2, 1, 0])
    model, fields = torch.cat([W.reshape(-1), b]).view(torch.int32), rec.view(torch.float64)
    assert fields[1].tolist()[:1] + fields[1].tolist()[5:] == [0, 0, 0, 0] and torch.equal(rows[1, :P], model)
    assert fields[3].tolist() == [-1, 0, 0, 0, 0, 1, 0, 0] and torch.equal(rows[3, :P], model)
    for k in (0, 2, 4):
        assert torch.equal(rows[k], clean[0][k]) and torch.equal(rec[k], clean[1][k]), k
    assert bool((tail == 0xA5).all())
    with pytest.raises(IndexError, match=r"client 3: a label lies outside \[0, 10\)"):
        train(W, b, dev, "none", "adam", 1)
    torch.cuda.synchronize()  # nothing faulted


@functools.lru_cache(maxsize=None)
def trip_inputs():
    """A cohort of three clients at D = 252, C = 2 under SGD whose client 1 (three slices) alone trips, at epoch 1:
    its rows are one x under both labels, so its loss is a function of u = z_0 - z_1 alone with its minimum at u = 0,
    and x is long enough that lr (|x|^2 + 1) / 2 = 9: from u = 0.2 the first step lands near u = -1.6 and the
    gradient grows sixfold.  Returns (W, b, batches, lr_ratio, the factor left on either side of the threshold)."""
    D, R, lr = 252, split_slice_rows(252), HYPER["sgd"]["lr"]
    g = torch.Generator().manual_seed(71)
    W, b = torch.randn(2, D, generator=g, dtype=torch.float64) / math.sqrt(D), torch.randn(2, generator=g, dtype=torch.float64)
    d, x = W[0] - W[1], torch.randn(D, generator=g, dtype=torch.float64)
    x = x - (x @ d) / (d @ d) * d  # the part of x that leaves u alone, at the length wanted, then u = 0.2
    x = x * math.sqrt(18 / lr - 1) / x.norm() + (0.2 - float(b[0] - b[1])) / (d @ d) * d
    W, b = W.float(), b.float()
    batches = [(0.25 * torch.randn(R + 1, D, generator=g), torch.randint(0, 2, (R + 1,), generator=g)),
               (x.float().repeat(2 * R + 2, 1), torch.arange(2 * R + 2) % 2),
               (0.25 * torch.randn(5, D, generator=g), torch.randint(0, 2, (5,), generator=g))]
    # |g| / |last_w| per client and epoch from the fp64 reference, one iteration more than the test runs
    ratios = [[r * lr * RATIO for r in linear_loop_ref(W, b, x, y, iters=ITERS + 1, activation="none", optimizer="sgd",
                                                       ratio=RATIO, **HYPER["sgd"])["guard_ratio"]] for x, y in batches]
    low = max(ratios[0] + ratios[1][:1] + ratios[2])
    thr = math.sqrt(low * ratios[1][1])
    return W, b, batches, thr, min(thr / low, ratios[1][1] / thr)


def test_a_trip_after_the_first_epoch_leaves_the_row_at_the_trip():
    W, b, batches, lr_ratio, factor = trip_inputs()
    assert factor >= 2  # on both sides of the threshold, for every client and epoch
    ratio = lr_ratio / HYPER["sgd"]["lr"]
    ref = linear_loop_ref(W, b, *batches[1], iters=ITERS, activation="none", optimizer="sgd", ratio=ratio, **HYPER["sgd"])
    assert ref["trip"] == 1
    dev = on_device(batches)
    rows, rec, _ = entry(W, b, dev, "sgd", 2, [0, 1, 2], lr_ratio=lr_ratio)
    fields = rec.view(torch.float64)
    assert fields[:, 0].tolist() == [-1, 1, -1] and fields[:, 6].tolist() == [ITERS, 1, ITERS]
    row = rows[1].view(torch.float32)
    w_dev = max(float((row[:504].view(2, 252).double() - ref["W"]).abs().max()), float((row[504:506].double() - ref["b"]).abs().max()))
    print("tripped client, w after one step:", w_dev)
    assert w_dev <= BOUND["w"]
    longer = entry(W, b, dev, "sgd", 2, [0, 1, 2], iters=ITERS + 1, lr_ratio=lr_ratio)
    assert torch.equal(longer[0][1], rows[1]) and torch.equal(longer[1][1], rec[1])  # later launches leave it alone
    res = train(W, b, dev, "none", "sgd", 2, ratio=ratio)
    assert res.results[1] == (None,) * 4 and None not in res.results[0] + res.results[2]


def test_the_round_on_the_split_rows_has_the_bits_of_the_round_on_rows_packed_from_the_state_dicts():
    W, b, batches = inputs(0)
    res = train(W, b, on_device(batches), "none", "sgd", 2)
    packed = torch.zeros_like(res.rows)
    for k in range(len(batches)):
        sd = res.state_dict(k)
        packed[k, :res.P] = torch.cat([sd["1.weight"].reshape(-1), sd["1.bias"]])
    weights = weights_tensor(sample_weights(res.sample_numbers), torch.float32, DEV)
    (out, sumsq), (want, want_sq) = reduce_with_sqdist(res.rows, weights, res.P), reduce_with_sqdist(packed, weights, res.P)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert torch.equal(sumsq.view(torch.int64), want_sq.view(torch.int64))
