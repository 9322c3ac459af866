"""The fused client Adam step against torch.optim.Adam itself on the MI355X,
three ways and bit for bit after every step of a chain, on w, exp_avg,
exp_avg_sq and max_exp_avg_sq:

    T  torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad=True),
       built as client.py:43-44 builds it (no foreach= or fused= argument)
    K  mfl_amd.ClientStepStats(params, step="fused", optimizer="adam", ...):
       begin(), then adam_step() per step, the state read through the
       object's own planes and offsets
    H  client_adam_ref.reference under client_stats.adam_form's mask, chained

The assertion is K == T in every bit of every element (NaN at the same
positions; payloads are not compared).  H says whose fault a difference is:
K != H is a kernel bug, K == H != T means the definition is not torch's in
that regime.

The chains are client_adam_cases.chain's: twelve steps at the reference's own
hyperparameters (a), without weight decay (b), with an eps fp16 keeps (c) and
at the form probe's (d); gradient scales from 1 down to where the second
moment is subnormal or underflows in the model's type, divided by 32 from step
7 on so that amsgrad engages; nine keys of 1 to two units + 3 elements, as
separate tensors and as views of one flat buffer at every sub-16-B offset
with sentinels around every key.  tests/test_client_adam_torch_cases_cpu.py
holds those inputs to their conditions on H; here the same conditions are
asserted on torch's own state.  Then the special values against torch, and
client_train on a small convolutional net whose key sizes are 27, 3, 135, 5.

fp16 failed that comparison (K == H != T) and is not in ADAM_DTYPES; the
finding is kept executable on the C entry of the fp16 kernel: the kernel
equals its definition, torch does not, and torch equals the step with four of
its ops rounded once."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.optim.adam as torch_adam

import client_adam_cases as C
import client_adam_ref as A
import client_stats_oracle as O
import mfl_amd
from mfl_amd import _lib, client_stats

pytestmark = pytest.mark.gpu

KEYS = [k for k, dt in C.DTYPES.items() if dt in client_stats.ADAM_DTYPES]
LAYOUTS = ("separate", "flat")
CHAINS = [pytest.param(key, hyper, scale, id=f"{key}-{hyper}-{C.scale_id(scale)}")
          for key in KEYS for hyper in C.HYPERS for scale in C.CHAIN_SCALES[key]]


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture
def chosen(monkeypatch):
    """The implementations of torch/optim/adam.py that torch's steps went through, in order of first use."""
    seen = []
    for name in ("_single_tensor_adam", "_multi_tensor_adam", "_fused_adam"):
        real = getattr(torch_adam, name, None)
        if real is None:
            continue

        def spy(*args, _real=real, _name=name, **kwargs):
            if _name not in seen:
                seen.append(_name)
            return _real(*args, **kwargs)

        monkeypatch.setattr(torch_adam, name, spy)
    return seen


def _differ(a, b):
    """Elements whose bits differ, or of which one alone is NaN."""
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    return (nan_a != nan_b) | ((A.bits(a) != A.bits(b)) & ~(nan_a & nan_b))


def _first(mask):
    return torch.nonzero(mask).view(-1)[:8].tolist()


class Side:
    """The parameters and gradients of one optimizer (torch's or the fused step's) on the device: one tensor per key
    ("separate": torch's own, aligned allocations) or Parameter views of one flat buffer with the gradients views
    of a second one ("flat": client_adam_cases.Case's offsets, sentinels around every key)."""

    def __init__(self, c, layout, dev):
        self.c, self.layout, self.dev = c, layout, dev
        self.first = (np.cumsum(c.numel) - c.numel).tolist()
        es = torch.empty(0, dtype=c.dt).element_size()
        if layout == "flat":
            self.w_buf = c.host_buffer("w", c.w).to(dev)
            self.g_buf = torch.full((c.size["g"],), C.SENTINEL, dtype=c.dt, device=dev)
            assert self.w_buf.data_ptr() % 16 == 0 and self.g_buf.data_ptr() % 16 == 0
            self.params = [torch.nn.Parameter(v) for v in c.views(self.w_buf, "w")]
            grads = c.views(self.g_buf, "g")
            for p, g, sw, sg in zip(self.params, grads, c.start["w"].tolist(), c.start["g"].tolist()):
                assert p.data_ptr() == self.w_buf.data_ptr() + sw * es  # the parameter IS the view
                assert g.data_ptr() == self.g_buf.data_ptr() + sg * es
        else:
            self.params = [torch.nn.Parameter(c.w[a:a + n].clone().to(dev))
                           for a, n in zip(self.first, c.numel.tolist())]
            grads = [torch.empty(n, dtype=c.dt, device=dev) for n in c.numel.tolist()]
            assert all(t.data_ptr() % 16 == 0 for t in (*self.params, *grads))
        for p, g in zip(self.params, grads):
            p.grad = g
        self.gap = torch.ones(c.size["w"], dtype=torch.bool)
        self.gap[torch.from_numpy(c.pos["w"])] = False

    def set_grad(self, t):
        if self.layout == "flat":
            self.g_buf.copy_(self.c.host_buffer("g", self.c.g[t]))
        else:
            for p, a, n in zip(self.params, self.first, self.c.numel.tolist()):
                p.grad.copy_(self.c.g[t][a:a + n])

    def weights(self):
        if self.layout == "flat":
            return self.w_buf.cpu()[torch.from_numpy(self.c.pos["w"])]
        return torch.cat([p.detach().cpu() for p in self.params])

    def untouched(self, t):
        """Nothing outside a key was written, and the gradients (and their sentinels) are as they were set."""
        if self.layout == "flat":
            return bool((self.w_buf.cpu()[self.gap] == C.SENTINEL).all()) and \
                torch.equal(A.bits(self.g_buf.cpu()), A.bits(self.c.host_buffer("g", self.c.g[t])))
        return torch.equal(A.bits(torch.cat([p.grad.cpu() for p in self.params])), A.bits(self.c.g[t]))


def _adam_kwargs(hyper):
    h = C.HYPERS[hyper]
    return dict(lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"], amsgrad=True)


class Torch:
    def __init__(self, c, hyper, layout, dev):
        self.side = Side(c, layout, dev)
        self.opt = torch.optim.Adam(self.side.params, **_adam_kwargs(hyper))

    def step(self, t):
        self.side.set_grad(t)
        self.opt.step()
        state = [self.opt.state[p] for p in self.side.params]
        return (self.side.weights(), *(torch.cat([s[name].cpu() for s in state]) for name in C.STORED[1:]))


class Fused:
    def __init__(self, c, hyper, layout, dev):
        self.side = Side(c, layout, dev)
        self.side.set_grad(0)
        self.stats = mfl_amd.ClientStepStats(self.side.params, step="fused", optimizer="adam",
                                             adam=_adam_kwargs(hyper))
        assert self.stats.step_mode == "fused"
        self.stats.begin(1.0)
        # the state through the object's own planes and key offsets
        numel, offset = self.stats._numel, self.stats._offset
        assert numel.tolist() == c.numel.tolist()
        self.pos = torch.from_numpy(np.concatenate([o + np.arange(n) for o, n in zip(offset, numel)]))

    def step(self, t):
        self.side.set_grad(t)
        self.stats.adam_step(0.5, 1.0)
        return (self.side.weights(), *(self.stats._step.plane(i).cpu()[self.pos] for i in range(3)))


def _compare(tag, got_k, got_t, want_h):
    """K == T on all four tensors; a difference is reported with H's verdict on whose it is."""
    wrong = []
    for name, k, t, h in zip(C.STORED, got_k, got_t, want_h):
        kt, kh = _differ(k, t), _differ(k, h)
        if bool(kt.any()):
            whose = (f"K != H on {int(kh.sum())} (first {_first(kh)}): a kernel bug" if bool(kh.any())
                     else "K == H != T: the definition differs from torch in this regime")
            wrong.append(f"{tag} {name}: {int(kt.sum())} of {kt.numel()} elements differ from torch's, "
                         f"first {_first(kt)}; {whose}")
        elif bool(kh.any()):
            wrong.append(f"{tag} {name}: K == T, but the host reference differs on {int(kh.sum())} elements, "
                         f"first {_first(kh)}: the reference is not the definition here")
    assert not wrong, "\n".join(wrong)


def _run(dev, c, key, hyper, layout, what):
    form = client_stats.adam_form(dev, C.DTYPES[key])
    assert form is not None
    ref = [res for res, _ in c.reference(form, **C.HYPERS[hyper])]
    fused, torch_ = Fused(c, hyper, layout, dev), Torch(c, hyper, layout, dev)
    for t in range(c.steps):
        tag = f"{key} set ({hyper}) {what} {layout} step {t + 1}"
        got_k, got_t = fused.step(t), torch_.step(t)
        _compare(tag, got_k, got_t, ref[t])
        assert fused.side.untouched(t) and torch_.side.untouched(t), tag
    return fused


# ------------------------------------------------------------------ the chains
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key, hyper, scale", CHAINS)
def test_twelve_steps_equal_torch_in_every_bit(dev, chosen, key, hyper, scale, layout):
    c = C.chain(key, scale)
    if layout == "flat":  # all four (aligned, misaligned) pairs of w and g
        assert set(zip((c.off["w"] == 0).tolist(), (c.off["g"] == 0).tolist())) == \
            {(True, True), (True, False), (False, True), (False, False)}
    fused = _run(dev, c, key, hyper, layout, f"scale {C.scale_id(scale)}")
    print(f"torch.optim.Adam stepped through {chosen}")
    assert fused.stats._t == C.CHAIN_STEPS  # step 1 took the first path, 2-12 read the state


@pytest.mark.parametrize("key", KEYS)
def test_torchs_own_state_meets_the_conditions(dev, key):
    """The conditions of tests/test_client_adam_torch_cases_cpu.py on torch's state: what the comparison above is
    meant to see (amsgrad engaged, subnormal and underflowed second moments, a finite chain) is there in T."""
    counts = {}
    for hyper in C.condition_sets(key):
        counts[hyper] = {}
        for scale in C.CHAIN_SCALES[key]:
            c = C.chain(key, scale)
            torch_ = Torch(c, hyper, "separate", dev)
            got = counts[hyper][scale] = C.chain_counts([torch_.step(t) for t in range(c.steps)], c.g)
            print(f"{key} ({hyper}) {C.scale_id(scale)}: vmax' > v' {got['vmax_gt_v']} subnormal v' "
                  f"{got['subnormal_v']} underflowed v' {got['underflowed_v']} finite {all(got['finite'])}")
    C.check_conditions(key, counts)


def test_fp16_is_refused_under_fused_and_steps_with_torch_under_auto(dev):
    """fp16 failed this file's comparison at the reference's hyperparameters (K == H != T in step 1: exp_avg on 16,
    exp_avg_sq and max_exp_avg_sq on 77 of 32,862 elements at g ~ N(0, 1); 5, 9 and 9, and w on 2, at g ~ 2^-6 N(0,
    1); exp_avg on 20 at g ~ 2^-10 N(0, 1)), so it is not in ADAM_DTYPES: no form, no fused step."""
    dt = torch.float16
    assert dt not in client_stats.ADAM_DTYPES and "f16" not in KEYS and len(KEYS) == 3
    assert client_stats.adam_form(dev, dt) is None
    p = torch.nn.Parameter(torch.full((16,), 0.5, device=dev, dtype=dt))
    with pytest.raises(TypeError, match="step='fused' needs .*adam_form"):
        mfl_amd.ClientStepStats([p], step="fused", optimizer="adam", adam=dict(lr=0.001))
    assert mfl_amd.ClientStepStats([p], step="auto", optimizer="adam", adam=dict(lr=0.001)).step_mode == "torch"


# The ops torch's fp16 kernels round ONCE, from the exact result straight to fp16, where the kernel's definition
# rounds to fp32 first (scripts/probe_adam_ops.py --fp16-ties: g + wd w off the definition on 25, v * beta2 on 21,
# v1 + value g^2 on 38 of 32,862 elements at g ~ N(0, 1) and on none of the single rounding; the lerp the other way
# round, 0 and 666; the other ops equal both on those values).  That the addcdiv is of the first kind shows on
# whole steps: with it rounded once torch's w is matched on every element, with it rounded twice missed on 11 to 44
# per chain.
F16_TORCH_ONCE = ("A", "mul", "C", "E")


@pytest.mark.parametrize("scale", C.CHAIN_SCALES["f16"], ids=C.scale_id)
@pytest.mark.parametrize("hyper", ("a", "b", "c"))
def test_fp16_kernel_equals_its_definition_and_torch_rounds_four_ops_once(dev, hyper, scale):
    """Why fp16 is not in ADAM_DTYPES, on fedavg_client_adam_step_f16 itself: twelve steps of torch's fp16 Adam, and
    after each, from the state torch had before it, the kernel under mask 15 (K), the definition (H) and the step
    with F16_TORCH_ONCE rounded once (client_adam_ref.step_f16_once).  K == H in every bit; T equals the
    once-rounded step in every bit; and at the reference's hyperparameters T differs from K at every scale."""
    from test_gpu_client_adam_ref import Adam

    key = "f16"
    c = C.chain(key, scale)
    torch_ = Torch(c, hyper, "separate", dev)
    adam = Adam(_lib.load_clientadam(), dev, c)
    pos_w, pos_s = torch.from_numpy(c.pos["w"]), torch.from_numpy(c.pos["s"]).to(dev)
    planes = adam.state.view(3, c.state_elems)
    prev = (c.w, *(torch.zeros_like(c.w) for _ in range(3)))
    off_k, off_once = [0] * 4, [0] * 4
    for t in range(c.steps):
        coef = A.coef_of(**C.HYPERS[hyper], t=t + 1)
        got_t = torch_.step(t)
        w_buf, g_buf = c.host_buffer("w", prev[0]).to(dev), c.host_buffer("g", c.g[t]).to(dev)
        for i in range(3):
            planes[i, pos_s] = prev[i + 1].to(dev)
        adam.run(c.views(w_buf, "w"), c.views(g_buf, "g"), coef, t == 0, 15)
        got_k = (w_buf.cpu()[pos_w], *adam.planes())
        want_h = A.step(key, 15, coef, prev[0], c.g[t], *prev[1:])
        once = A.step_f16_once(coef, prev[0], c.g[t], *prev[1:], once=F16_TORCH_ONCE)
        for i, name in enumerate(C.STORED):
            kh = _differ(got_k[i], want_h[i])
            assert not bool(kh.any()), (hyper, C.scale_id(scale), t + 1, name, int(kh.sum()), _first(kh))
            off_k[i] += int(_differ(got_t[i], got_k[i]).sum())
            off_once[i] += int(_differ(got_t[i], once[i]).sum())
        prev = got_t
    print(f"f16 ({hyper}) {C.scale_id(scale)}: over 12 steps torch differs from the kernel on {off_k} elements of "
          f"{C.STORED}, from the step with {F16_TORCH_ONCE} rounded once on {off_once}")
    assert off_once == [0] * 4
    assert hyper != "a" or sum(off_k) > 0


# -------------------------------------------------------------- special values
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hyper", ("a", "d"))
@pytest.mark.parametrize("key", KEYS)
def test_special_values_equal_torch(dev, key, hyper, layout):
    """NaN and +-inf in g, g = w = 0 (0 / eps), -0.0, subnormal g, w and g^2, a NaN in the ragged last slice: two
    steps, the second from inf and NaN in m, v and vmax."""
    _run(dev, C.specials(key), key, hyper, layout, "special values")


# ------------------------------------------------- client_train, odd key sizes
CONV_RATIO = 10000.0


def _conv_net():
    torch.manual_seed(20254)
    return torch.nn.Sequential(torch.nn.Conv2d(1, 3, 3), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(27, 5))


def _train_conv(dev, dt, step, net, batch, iters):
    base, _ = O.case_client(O.load_client_case("mlp_16x24x4_it4"), dev)
    args = types.SimpleNamespace(**{**vars(base.args), "client_optimizer": "adam", "lr": 0.001, "wd": 0.001})
    x, labels = batch
    # the fixture's client with the batch replaced, under a guard ratio at which lr = 0.001 steps at all (:71 gives
    # up when norm(g) > lr * ratio * norm(w); the fixture's 50 was set for its lr = 0.03)
    client = O.make_client_class(CONV_RATIO)((x.to(dt), labels), args, dev)
    net = copy.deepcopy(net).to(dt).to(dev)
    seen = []
    out = client_stats.client_train(client, net, iters, stats="hip", step=step,
                                    trace=lambda stage, w, g, loss: seen.append((stage, w, g, loss)))
    return out, seen


@pytest.mark.parametrize("key", KEYS)
def test_client_train_on_odd_key_sizes_fused_equals_torch(dev, key, monkeypatch):
    """Conv2d(1, 3, 3) + Linear(27, 5) on a (6, 1, 5, 5) batch, keys of 27, 3, 135 and 5 elements, at the reference's
    lr = wd = 0.001 for 12 local iterations: under test_client_train_fused_equals_torch's rules the traced weights
    and gradients of every stage are bit-equal between step="fused" and step="torch", the stages, loss and accuracy
    the same, rho and beta within 1e-6 relative, and no torch optimizer is built under fused stepping."""
    dt, iters = C.DTYPES[key], 12
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    net = _conv_net()
    assert [p.numel() for p in net.parameters()] == [27, 3, 135, 5]
    gen = torch.Generator().manual_seed(20255)
    batch = (torch.randn(6, 1, 5, 5, generator=gen), torch.randint(0, 5, (6,), generator=gen))
    (sd_t, loss_t, beta_t, rho_t, acc_t, _), seen_t = _train_conv(dev, dt, "torch", net, batch, iters)
    built = []
    real_adam = torch.optim.Adam
    monkeypatch.setattr(torch.optim, "Adam", lambda *a, **k: built.append(1) or real_adam(*a, **k))
    (sd_f, loss_f, beta_f, rho_f, acc_f, _), seen_f = _train_conv(dev, dt, "fused", net, batch, iters)
    assert loss_t is not None and built == []  # the guard never trips: all twelve steps are taken and compared
    assert [s[0] for s in seen_f] == [s[0] for s in seen_t] and len(seen_f) == 1 + 2 * iters
    assert sum(s[0] == "after_step" for s in seen_f) == iters
    for i, (a, b) in enumerate(zip(seen_f, seen_t)):
        for j in (1, 2):
            if a[j] is not None:
                wrong = _differ(a[j], b[j])
                assert not bool(wrong.any()), (key, i, a[0], "wg"[j - 1], int(wrong.sum()), _first(wrong))
        assert a[3] == b[3] or (a[3] != a[3] and b[3] != b[3]), (i, a[0])
    print(f"{key}: beta {beta_f!r} torch {beta_t!r}; rho {rho_f!r} torch {rho_t!r}; stages {len(seen_f)}")
    assert loss_f == loss_t and acc_f == acc_t
    assert O.rel(beta_f, beta_t) <= 1e-6 and O.rel(rho_f, rho_t) <= 1e-6
    for k in sd_t:
        assert torch.equal(sd_f[k], sd_t[k]), k
