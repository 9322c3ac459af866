"""The client's per-iteration statistics (``Client.train``, client.py:52-86) on the GPU.

Next to forward and backward the reference's local loop flattens the
gradients and the weights every iteration (``torch.cat``, :69, :76), tests
them (:71: NaN count, ``norm(grads)`` against ``lr * ratio * norm(last_w)``)
and tracks ``rho`` and ``beta`` (:78-84) from ``norm(w - last_w)`` and
``norm(grads - last_grads)``: about a dozen passes over the model and six to
eight blocking tensor truth tests.  :class:`ClientStepStats` does the same
bookkeeping with one fused pass over the gradients and one over the weights
(``fedavg_client_stats_f32``: NaN count, sum of squares, squared distance to
the previous step's snapshot, snapshot update) and keeps rho / beta on the
device (``fedavg_client_track``), with ONE host sync per local iteration (the
:71 guard, which decides whether the optimizer steps).

The norms are fl32(sqrt()) of fp64 sums of exact squares, i.e. the exactly
rounded values of what the reference's fp32 ``torch.norm`` approximates; rho
and beta then follow in the reference's fp32 arithmetic.

The dtype rule: the fused pass takes parameters that are all contiguous, on
one GPU and all of ONE dtype among fp32, bf16, fp16 and fp64.  bf16, fp16 and
fp64 models go through ``libfedavg_amd_clientvec.so``
(``fedavg_client_stats_{bf16,f16,f64}`` / ``fedavg_client_track_{bf16,f16,f64}``):
snapshots in the model's own type, the difference formed in that type, norms
``rT(fl32(sqrt()))`` (fp64: ``sqrt()``) and every scalar operation after them
as ATen does it, in opmath and then rounded once to the type.

``stats="torch"`` computes the same quantities with the reference's own torch
expressions on whatever device the parameters are on; it is what CPU
parameters, models of mixed dtypes and any other dtype get under
``stats="auto"``.

``step="fused"`` (opt in; the default ``"torch"`` is ``optimizer.step()`` and
the weight pass above) replaces the plain SGD step of :74 and the weight pass
by ONE kernel (``libfedavg_amd_clientstep.so``, ``fedavg_client_sgd_step_*``):
it reads ``w`` and ``g``, writes ``w' = w - lr * g`` and sums ``w'^2`` and
``rT(w' - w)^2`` on the way, since ``last_w`` of :78 is always the weight the
step started from.  No weight snapshot is read or written: 12 B per fp32
element instead of 24.  The bits it leaves must be torch's, and whether ATen's
kernel fuses the multiply and the add is a property of the torch build:
:func:`sgd_form` finds out on the GPU, once per (device, dtype).

``optimizer="adam"`` with fused stepping does the same for the reference's
default optimizer, ``torch.optim.Adam(lr, weight_decay=wd, amsgrad=True)``
(``libfedavg_amd_clientadam.so``, ``fedavg_client_adam_step_*``): one kernel
reads ``w``, ``g`` and the state ``m, v, vmax`` and writes ``w, m, v, vmax``
where torch's multi-tensor Adam makes nine launches.  Four of its operations
have the shape ``x + s * y``; which of them torch's kernels fuse is found by
:func:`adam_form`, once per (device, dtype).

``guard="device"`` (opt in, with fused stepping) removes the one sync per
iteration that is left: the :71 guard is decided on the device and the step is
gated on it (``libfedavg_amd_clientloop.so``: ``fedavg_client_guard_*``,
``fedavg_client_{sgd,adam}_step_gated_*``), so the host queues iterations
without waiting and reads ONE record at the end of ``train``.

:func:`client_train` is ``Client.train`` written against this class and
:func:`patch` binds it to a ``Client`` class (opt in; ``install()`` does not).
"""
from __future__ import annotations

import math
import sys

import numpy as np
import torch

from . import _lib

ALIGN = 4  # fp32 snapshot key offsets are multiples of 4 elements (16 B)

# dtype -> (entry suffix, numpy type of the snapshot's bits); fp32 is the product library's
_VEC_DTYPES = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float64: "f64"}
FUSED_DTYPES = (torch.float32, *_VEC_DTYPES)
_RULE = "contiguous parameters on one GPU, all of one dtype among fp32, bf16, fp16 and fp64"

# rec: one device record of doubles, read back in one D2H.  The device guard adds the previous loss, the gate and
# the epoch of the first trip (include/fedavg_amd_clientloop.h: loss = rec[_LOSS:_LOSS + 2], gate = rec[_GATE:_GATE + 2])
_W, _G, _STATE, _LOSS, _LAST, _GATE, _EPOCH, _REC = 0, 4, 8, 12, 13, 14, 15, 16
# guard="device": how many iterations the host may queue before it waits for the oldest one's record
DEFAULT_AHEAD = 1
_GUARD_RULE = ("fused stepping (step='fused', or 'auto' where it applies): the step is gated on the device, which "
               "optimizer.step() cannot be")


def _fused_ok(params) -> bool:
    return bool(params) and all(p.is_cuda and p.is_contiguous() for p in params) and \
        len({p.device for p in params}) == 1 and len({p.dtype for p in params}) == 1 and \
        params[0].dtype in FUSED_DTYPES


def _round_to(x, dtype):
    """rT(fl32(x)) as a Python float: x rounded to fp32, then to ``dtype``
    (nearest even both times), as ATen casts an opmath result.  fp64: x."""
    if dtype == torch.float64:
        return float(x)
    with np.errstate(all="ignore"):
        f = np.float32(x)
        if dtype == torch.float32:
            return float(f)
        if dtype == torch.float16:
            return float(np.float16(f))
    if math.isnan(f):
        return math.nan
    u = int(f.view(np.uint32))
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000  # bf16: the upper half of the fp32 word
    return float(np.uint32(u).view(np.float32))


def _norm_of(sumsq, dtype):
    """norm(S) = rT(fl32(sqrt(S))) (fp64: sqrt(S)): the exactly rounded value
    of what ATen's norm approximates in opmath."""
    if math.isnan(sumsq):
        return math.nan
    return _round_to(math.sqrt(sumsq), dtype)


def _guard_bound(n_w, lr_ratio, dtype):
    """``lr * ratio * norm(last_w)`` (:71): python_float * tensor, the scalar
    rounded to opmath, the product to the tensor's type."""
    if dtype == torch.float64:
        return n_w * lr_ratio
    with np.errstate(all="ignore"):
        # the fp64 product of two fp32 values is exact: one rounding to fp32
        return _round_to(np.float64(n_w) * np.float64(np.float32(lr_ratio)), dtype)


# ------------------------------------------------------------------ fused step
# The dtypes the fused step is offered for: those sgd_form() found a form for on the MI355X (torch 2.10 / ROCm 7.0:
# form 1 for fp32, bf16 and fp64).  Not fp16: there torch's kernel rounds fma(alpha, g, w) ONCE, to fp16 (a
# mixed-precision fma), while both forms round to fp32 first; on sgd_form's probe form 1 differs from torch on 2 of
# 571 elements, form 0 on 61.  fedavg_client_sgd_step_f16 stays in the C ABI; nothing here calls it.
STEP_DTYPES = (torch.float32, torch.bfloat16, torch.float64)
_STEP_SUFFIX = {torch.float32: "f32", **_VEC_DTYPES}
_STEP_RULE = (f"the fused statistics ({_RULE}), fp32, bf16 or fp64 parameters, a plain SGD step (client_optimizer "
              "'sgd': no momentum, no weight decay) and a form of the step kernel that leaves torch.optim.SGD's bits "
              "on this GPU (sgd_form)")
_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_PROBE_LR = 0.03
_PROBE_N = 512
_PROBE_POOL = 1 << 21
_probes = {}  # (device index, dtype) -> the probe's findings


class _StepPass:
    """The buffers of ``fedavg_client_sgd_step_*`` calls over tensors of
    ``numel`` elements, and the call.  The pinned key table is reused under
    ``ClientStepStats._pass``'s rule: new bytes only after the stream has
    passed the last call that shipped the old ones."""

    def __init__(self, numel, dtype, device):
        self.lib = _lib.load_clientstep()
        self.name = f"fedavg_client_sgd_step_{_STEP_SUFFIX[dtype]}"
        self.fn = getattr(self.lib, self.name)
        self.device = device
        self.numel = np.ascontiguousarray(numel, dtype=np.int64)
        n = len(self.numel)
        es = torch.empty(0, dtype=dtype).element_size()
        nparts = int(self.lib.fedavg_client_step_partials(self.numel.ctypes.data, n, es))
        ws = int(self.lib.fedavg_client_step_workspace(n))
        with torch.cuda.device(device):
            self.partials = torch.empty(max(nparts, 1), dtype=torch.float64, device=device)
            self.host_ws = torch.empty(max(ws, 16), dtype=torch.uint8, pin_memory=True)
            self.dev_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=device)
        self._free = None    # event: the stream has passed the last use of host_ws
        self._staged = None  # the pointer tables host_ws holds
        self._gated = None

    def launch(self, w_ptrs, g_ptrs, lr, form, stats_ptr, st, gated=None):
        """w -= lr * g over the tensors at w_ptrs / g_ptrs on torch stream
        ``st``; the record goes to the 4 device doubles at ``stats_ptr``.
        ``gated``: the device addresses ``(g_stats, gate, state, loss)`` of
        ``fedavg_client_sgd_step_gated_*``, which then takes the call."""
        table = w_ptrs.tobytes() + g_ptrs.tobytes()
        if self._free is not None and table != self._staged:
            self._free.synchronize()  # host_ws gets new bytes below (already passed after an iteration's sync)
        self._staged = table
        fn, name, check, more = self.fn, self.name, _lib.check_clientstep, ()
        if gated is not None:
            if self._gated is None:
                self._gated = self.name.replace("_step_", "_step_gated_")
                self._gated = (getattr(_lib.load_clientloop(), self._gated), self._gated)
            (fn, name), check, more = self._gated, _lib.check_clientloop, gated
        with torch.cuda.device(self.device):
            rc = fn(w_ptrs.ctypes.data, g_ptrs.ctypes.data, self.numel.ctypes.data, len(self.numel), float(lr),
                    form, self.partials.data_ptr(), self.partials.numel(), stats_ptr, self.host_ws.data_ptr(),
                    self.dev_ws.data_ptr(), self.host_ws.numel(), st.cuda_stream, *more)
            check(rc, name)
            if self._free is None:
                self._free = torch.cuda.Event()
            self._free.record(st)


def _probe_values(dtype):
    """Seeded model-like weights N(0, 0.05^2) and gradients N(0, 1) of type
    ``dtype`` for the probe.  In fp32 and fp64 the two forms differ on about
    every third random element.  In a 16-bit type they differ only where the
    fp32 results lie on either side of a rounding boundary of the type (one
    element in tens of thousands), so the first _PROBE_N values of a larger
    seeded pool are joined by those of its elements at which a host
    computation of the two forms differs; whether they differ on the device
    is sgd_form's own check."""
    wide = dtype in (torch.float32, torch.float64)
    rng = np.random.default_rng(20250)
    n = _PROBE_N if wide else _PROBE_POOL
    w = torch.from_numpy(rng.normal(0.0, 0.05, n)).to(dtype)
    g = torch.from_numpy(rng.normal(0.0, 1.0, n)).to(dtype)
    if wide:
        return w, g
    wf, gf = w.float().numpy(), g.float().numpy()
    alpha = np.float32(-_PROBE_LR)
    with np.errstate(all="ignore"):
        apart = torch.from_numpy(wf + alpha * gf).to(dtype)  # two fp32 roundings, then the type's
        once = torch.from_numpy((wf.astype(np.float64) + np.float64(alpha) * gf.astype(np.float64))
                                .astype(np.float32)).to(dtype)  # the product is exact in fp64
    picked = torch.nonzero(apart.view(torch.int16) != once.view(torch.int16)).view(-1).numpy()[:_PROBE_N]
    idx = torch.from_numpy(np.union1d(np.arange(_PROBE_N), picked))
    return w[idx].clone(), g[idx].clone()


def _probe_sgd_form(device, dtype):
    w, g = _probe_values(dtype)
    bits = _BITS[w.element_size()]
    with torch.cuda.device(device):
        w, g = w.to(device), g.to(device)
        p = torch.nn.Parameter(w.clone())
        p.grad = g.clone()
        torch.optim.SGD([p], lr=_PROBE_LR).step()
        want = p.detach().view(bits)
        step = _StepPass([w.numel()], dtype, device)
        rec = torch.empty(4, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream(device)
        got = []
        for form in (0, 1):
            c = w.clone()
            step.launch(np.array([c.data_ptr()], dtype=np.int64), np.array([g.data_ptr()], dtype=np.int64),
                        _PROBE_LR, form, rec.data_ptr(), st)
            got.append(c.view(bits))
        differ = int((got[0] != got[1]).sum())
        match = tuple(bool(torch.equal(c, want)) for c in got)
    form = None
    if differ:  # equal outputs would say nothing about which one torch computes
        form = 0 if match[0] else 1 if match[1] else None
    return {"form": form, "differ": differ, "match": match, "n": int(w.numel())}


def sgd_form_probe(device, dtype):
    """What :func:`sgd_form` found for (device, dtype), cached: ``form``, the
    number of probe elements on which the kernel's two forms ``differ``,
    ``match`` (form 0 / form 1 equal to torch on every element) and ``n``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError(f"sgd_form needs a GPU, not {device}")
    index = torch.cuda.current_device() if device.index is None else device.index
    key = (index, dtype)
    if key not in _probes:
        _probes[key] = _probe_sgd_form(torch.device("cuda", index), dtype)
    return _probes[key]


def sgd_form(device, dtype):
    """Which form of ``fedavg_client_sgd_step_*`` leaves the bits of
    ``torch.optim.SGD(params, lr=lr).step()`` on this GPU: 1 (``fma(-lr, g,
    w)``), 0 (product and sum rounded separately) or ``None`` (neither, or no
    kernel for the dtype).  Found by running torch's own step and both forms
    on the same seeded values, once per (device, dtype)."""
    if dtype not in STEP_DTYPES:
        return None
    return sgd_form_probe(device, dtype)["form"]


# ------------------------------------------------------------------ fused Adam step
# The dtypes the fused Adam step is offered for.  Two findings on the MI355X (torch 2.10 / ROCm 7.0) decide it: the
# probe below finds one mask that equals torch (mask 15, all four sites one fma, for fp32, bf16, fp16 and fp64), AND
# the kernel under that mask equals torch.optim.Adam bit for bit over twelve-step chains at the reference's own
# hyperparameters and three other sets, down to subnormal second moments (tests/test_gpu_client_adam_torch.py;
# DESIGN.md §3).  fp16 passes the first and fails the second: torch's fp16 kernels round g + wd * w, v * beta2,
# v1 + value * g1^2 and w + step * (m' / s3) ONCE, from the exact result straight to fp16 (scripts/probe_adam_ops.py
# --fp16-ties, profiles/client_adam/ops_probe_fp16_ties.json; tests/test_gpu_client_adam_torch.py), where every
# form of the kernel rounds to fp32 first.  The two part
# where the exact result lies within half an fp32 ulp of an fp16 rounding midpoint, which the decimal scalars 0.001
# and 0.999 make common for fp16 operands and the probe's scalars do not.  The same test file holds that finding on
# the kernel's C entry.  fedavg_client_adam_step_f16 stays in the C ABI; nothing here calls it.  For a dtype outside
# this tuple adam_form() answers None without probing; adam_form_probe() still runs the probe and reports what it
# finds (for fp16: mask 15), which says that the mask matches torch on the probe's values and no more.
ADAM_DTYPES = (torch.float32, torch.bfloat16, torch.float64)
ADAM_SITES = 4  # A g + wd w, B the lerp, C the addcmul, E the addcdiv: bit i of a form mask fuses site i
_ADAM_RULE = (f"the fused statistics ({_RULE}), a dtype of ADAM_DTYPES (fp32, bf16, fp64), torch.optim.Adam with "
              "amsgrad=True and beta1 > 0.5 over parameters that all require grad, and a form of the Adam step kernel that leaves "
              "torch.optim.Adam's bits on this GPU (adam_form)")
# The form is a property of torch's compiled kernels, not of the hyperparameters, so the probe picks hyperparameters
# and values at which both terms of every site are of one magnitude (w, g ~ N(0, 1)): there two forms of a site leave
# different fp32 bits on about every third element.  At the reference's own (wd = 0.001 against g ~ 1) they hardly
# ever do.
_ADAM_PROBE = dict(lr=0.3, betas=(0.6, 0.7), eps=1e-8, weight_decay=0.3)
_ADAM_PROBE_STEPS = 3
_adam_probes = {}  # (device index, dtype) -> the probe's findings


def adam_coef(lr, beta1, beta2, eps, weight_decay, t):
    """The seven coefficients of ``fedavg_client_adam_step_*`` for step ``t``
    (from 1), in Python floats exactly as torch/optim/adam.py forms them."""
    t = float(t)
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    step_size = (lr / bias_correction1) * -1
    return np.array([weight_decay, 1 - beta1, beta2, 1 - beta2, bias_correction2 ** 0.5, eps, step_size],
                    dtype=np.float64)


class _AdamPass:
    """The optimizer state (three planes ``m, v, vmax`` of ``state_elems``
    elements in one zeroed buffer, key j at ``offset[j]``), the buffers of
    ``fedavg_client_adam_step_*`` calls and the call.  The pinned key table is
    reused under ``_StepPass``'s rule."""

    def __init__(self, numel, offset, state_elems, dtype, device):
        self.lib = _lib.load_clientadam()
        self.name = f"fedavg_client_adam_step_{_STEP_SUFFIX[dtype]}"
        self.fn = getattr(self.lib, self.name)
        self.device = device
        self.numel = np.ascontiguousarray(numel, dtype=np.int64)
        self.offset = np.ascontiguousarray(offset, dtype=np.int64)
        n = len(self.numel)
        es = torch.empty(0, dtype=dtype).element_size()
        self.state_elems = int(state_elems)
        nparts = int(self.lib.fedavg_client_adam_partials(self.numel.ctypes.data, n, es))
        ws = int(self.lib.fedavg_client_adam_workspace(n))
        with torch.cuda.device(device):
            self.state = torch.zeros(3 * max(self.state_elems, 16 // es), dtype=dtype, device=device)
            self.partials = torch.empty(max(nparts, 1), dtype=torch.float64, device=device)
            self.host_ws = torch.empty(max(ws, 16), dtype=torch.uint8, pin_memory=True)
            self.dev_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=device)
        self._free = None    # event: the stream has passed the last use of host_ws
        self._staged = None  # the pointer tables host_ws holds
        self._gated = None

    def plane(self, i):
        """Plane i (0 ``m``, 1 ``v``, 2 ``vmax``) as a view of the state."""
        return self.state[i * self.state_elems:(i + 1) * self.state_elems]

    def launch(self, w_ptrs, g_ptrs, coef, first, form, stats_ptr, st, gated=None):
        """``gated``: as ``_StepPass.launch``'s (``fedavg_client_adam_step_gated_*``)."""
        table = w_ptrs.tobytes() + g_ptrs.tobytes()
        if self._free is not None and table != self._staged:
            self._free.synchronize()  # host_ws gets new bytes below (already passed after an iteration's sync)
        self._staged = table
        fn, name, check, more = self.fn, self.name, _lib.check_clientadam, ()
        if gated is not None:
            if self._gated is None:
                self._gated = self.name.replace("_step_", "_step_gated_")
                self._gated = (getattr(_lib.load_clientloop(), self._gated), self._gated)
            (fn, name), check, more = self._gated, _lib.check_clientloop, gated
        with torch.cuda.device(self.device):
            rc = fn(w_ptrs.ctypes.data, g_ptrs.ctypes.data, self.numel.ctypes.data, self.offset.ctypes.data,
                    len(self.numel), self.state.data_ptr(), self.state_elems, coef.ctypes.data, int(bool(first)),
                    form, self.partials.data_ptr(), self.partials.numel(), stats_ptr, self.host_ws.data_ptr(),
                    self.dev_ws.data_ptr(), self.host_ws.numel(), st.cuda_stream, *more)
            check(rc, name)
            if self._free is None:
                self._free = torch.cuda.Event()
            self._free.record(st)


def _adam_probe_values(dtype):
    """Seeded weights and gradients N(0, 1), the pool of 2^21: in a 16-bit
    type the two forms of site A, B or E leave different bits on tens to
    hundreds of its elements."""
    rng = np.random.default_rng(20251)
    return (torch.from_numpy(rng.normal(0.0, 1.0, _PROBE_POOL)).to(dtype),
            torch.from_numpy(rng.normal(0.0, 1.0, _PROBE_POOL)).to(dtype))


def _mine_site_c(dtype, most=64):
    """``(beta2, g, v)`` for a 16-bit ``dtype`` on which site C's two forms,
    ``v' = rT(v1 + value * g^2)`` with ``v1 = rT(v * beta2)`` and ``value = 1
    - beta2``, store different bits: a Python float, one gradient value and up
    to ``most`` second moments.

    Random values never reach this site in a 16-bit type.  Both terms are
    non-negative and ``v1`` is a value of the type, so the forms part only
    when ``fl32(value * g^2)`` is inexact and lies half an fp32 ulp of the
    sum from a rounding boundary of the type: its low 24 - p bits are all
    ones with the exact product below it, or 0...01 with it above (p the
    type's precision).  That is a property of ``(value, g)`` alone, one pair
    in 2^(25 - p); a seeded search over ``value`` in (0.2, 0.4) and ``g ~ N(0,
    1)`` finds such pairs, and for one of them every ``v`` of the type in
    [2^-6, 16) is tried.  The forms are computed here in fp64 (the product
    exact, the sum rounded once more): a filter, as in ``_probe_values``;
    whether they differ on the device is adam_form's own check."""
    prec = {torch.float16: 11, torch.bfloat16: 8}[dtype]
    rng = np.random.default_rng(20253)
    n = 1 << 21
    value = rng.uniform(0.2, 0.4, n).astype(np.float32)
    g = torch.from_numpy(rng.normal(0.0, 1.0, n)).to(dtype).float().numpy()
    exact = value.astype(np.float64) * (g * g).astype(np.float64)  # g * g is exact in fp32 for a 16-bit g
    with np.errstate(all="ignore"):
        c = exact.astype(np.float32)
    low = c.view(np.uint32) & np.uint32((1 << (24 - prec)) - 1)
    cand = np.flatnonzero(((low == (1 << (24 - prec)) - 1) & (exact < c)) | ((low == 1) & (exact > c)))
    every = torch.arange(0, 1 << 15, dtype=torch.int16).view(dtype).float().numpy()
    every = every[(every >= 2.0 ** -6) & (every < 16.0)]
    to_type = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dtype).float().numpy()  # noqa: E731
    for i in cand:
        beta2 = 1.0 - float(value[i])
        if np.float32(1.0 - beta2) != value[i]:
            continue
        with np.errstate(all="ignore"):
            v1 = to_type(every * np.float32(beta2))
            apart = to_type(v1 + c[i])
            once = to_type((v1.astype(np.float64) + exact[i]).astype(np.float32))
        hit = np.flatnonzero(apart != once)[:most]
        if len(hit):
            return beta2, torch.tensor(float(g[i]), dtype=dtype), torch.from_numpy(every[hit]).to(dtype)
    raise RuntimeError(f"no pair found for site C in {dtype}")


def _probe_adam_form(device, dtype):
    h = dict(_ADAM_PROBE)
    w, g = _adam_probe_values(dtype)
    mined = None
    if dtype in (torch.float16, torch.bfloat16):
        # the last elements of the probe are site C's: w = 0 (so g1 = g), and before step 2 their v and vmax are
        # set to the mined second moments, in torch's state and in the kernel's alike
        beta2, g_c, v_c = _mine_site_c(dtype)
        h["betas"] = (h["betas"][0], beta2)
        mined = slice(w.numel() - v_c.numel(), w.numel())
        w[mined] = 0.0
    bits = _BITS[w.element_size()]
    n = w.numel()
    with torch.cuda.device(device):
        w, g = w.to(device), g.to(device)
        grads = [torch.roll(g, 7 * t) for t in range(_ADAM_PROBE_STEPS)]  # another gradient every step
        if mined is not None:
            v_c = v_c.to(device)
            grads[1][mined] = g_c.to(device)

        def inject(w_t, v_t, vmax_t):
            w_t[mined] = 0.0
            v_t[mined] = v_c
            vmax_t[mined] = v_c

        p = torch.nn.Parameter(w.clone())
        opt = torch.optim.Adam([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"],
                               amsgrad=True)
        want = []
        for t in range(_ADAM_PROBE_STEPS):
            if mined is not None and t == 1:
                with torch.no_grad():
                    inject(p, opt.state[p]["exp_avg_sq"], opt.state[p]["max_exp_avg_sq"])
            p.grad = grads[t].clone()
            opt.step()
            state = opt.state[p]
            want.append([x.detach().view(bits).clone() for x in
                         (p, state["exp_avg"], state["exp_avg_sq"], state["max_exp_avg_sq"])])
        rec = torch.empty(4, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream(device)
        numel, offset = np.array([n], dtype=np.int64), np.zeros(1, dtype=np.int64)
        step = _AdamPass(numel, offset, n, dtype, device)
        off = []
        for form in range(1 << ADAM_SITES):
            c = w.clone()
            differ = torch.zeros((), dtype=torch.int64, device=device)
            for t in range(_ADAM_PROBE_STEPS):
                if mined is not None and t == 1:
                    inject(c, step.plane(1), step.plane(2))
                coef = adam_coef(h["lr"], *h["betas"], h["eps"], h["weight_decay"], t + 1)
                step.launch(np.array([c.data_ptr()], dtype=np.int64), np.array([grads[t].data_ptr()], dtype=np.int64),
                            coef, t == 0, form, rec.data_ptr(), st)
                for a, b in zip([c.view(bits)] + [step.plane(i).view(bits) for i in range(3)], want[t]):
                    differ += (a != b).sum()
            off.append(int(differ))  # the one read per mask
    # two masks that both equal torch equal each other on the whole probe: it cannot tell them apart, and a mask that
    # equals torch differs from every one that does not.  So the answer is the ONE mask at 0, if there is exactly one.
    match = tuple(o == 0 for o in off)
    form = match.index(True) if sum(match) == 1 else None
    return {"form": form, "match": match, "off": tuple(off), "n": int(n), "steps": _ADAM_PROBE_STEPS,
            "mined_site_c": 0 if mined is None else int(v_c.numel()), "betas": h["betas"]}


def adam_form_probe(device, dtype):
    """What :func:`adam_form` found for (device, dtype), cached: ``form``,
    ``match`` (per mask: equal to torch on every element of ``p, exp_avg,
    exp_avg_sq, max_exp_avg_sq`` after each of ``steps`` steps), ``off`` (per
    mask: the number of elements that differ from torch's) and ``n``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError(f"adam_form needs a GPU, not {device}")
    index = torch.cuda.current_device() if device.index is None else device.index
    key = (index, dtype)
    if key not in _adam_probes:
        _adam_probes[key] = _probe_adam_form(torch.device("cuda", index), dtype)
    return _adam_probes[key]


def adam_form(device, dtype):
    """Which form mask of ``fedavg_client_adam_step_*`` leaves the bits of
    ``torch.optim.Adam(params, lr, weight_decay=wd, amsgrad=True).step()`` on
    this GPU, or ``None``.  Found by running torch's own optimizer for three
    steps and the kernel under all 16 masks on the same seeded values (for a
    16-bit type joined by pairs mined for site C, which random values never
    reach there); the
    answer is a mask that equals torch on every element of the parameter and
    of the three state tensors at every step and differs from every other
    mask somewhere on the probe.  Once per (device, dtype).  ``None``
    without a probe for a dtype outside ``ADAM_DTYPES``: that tuple leaves
    out fp16, whose mask equals torch on the probe but not at the
    reference's hyperparameters (see the comment at ``ADAM_DTYPES``)."""
    if dtype not in ADAM_DTYPES:
        return None
    return adam_form_probe(device, dtype)["form"]


def _adam_hyper(adam):
    """``adam`` with torch.optim.Adam's defaults filled in; ``lr`` is required."""
    if adam is None or "lr" not in adam:
        raise ValueError("optimizer='adam' needs adam=dict(lr=..., betas=(0.9, 0.999), eps=1e-8, weight_decay=0, "
                         "amsgrad=True)")
    unknown = set(adam) - {"lr", "betas", "eps", "weight_decay", "amsgrad"}
    if unknown:
        raise ValueError(f"adam: unknown keys {sorted(unknown)}")
    h = {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "amsgrad": True, **adam}
    h["betas"] = (float(h["betas"][0]), float(h["betas"][1]))
    return h


class ClientStepStats:
    """Snapshots, key tables, workspaces and the running rho / beta of one
    ``Client.train`` call.

    ``begin()`` after the prologue's backward (:52-57), then per local
    iteration ``after_backward()`` (:69-71, the one sync; ``True`` = the guard
    trips) and ``after_step()`` (:76-86, no sync); ``result()`` at the end.
    ``trace(stage, w, g, loss)`` receives clones of the flattened weights and
    gradients at every call (``g`` is ``None`` where there is none yet).

    ``step="fused"``: ``sgd_step()`` takes the place of the caller's
    ``optimizer.step()`` and of ``after_step()`` (one kernel, no sync); it
    needs the fused statistics and a form from :func:`sgd_form`, else
    ``TypeError``.  ``step="auto"`` falls back to ``"torch"`` instead;
    ``step_mode`` says which of the two the object was built for.

    ``optimizer="adam"`` with ``adam=dict(lr, betas=(0.9, 0.999), eps=1e-8,
    weight_decay=0, amsgrad=True)``: under fused stepping the object owns the
    zeroed optimizer state and the step count, and ``adam_step()`` takes the
    place of ``optimizer.step()`` and ``after_step()``.  ``amsgrad=False``, a
    parameter that does not require grad, ``beta1 <= 0.5`` or a dtype without
    a form from :func:`adam_form` are a ``TypeError`` under ``"fused"`` and
    torch under ``"auto"``.

    ``guard="device"`` (opt in; the default ``"host"`` is everything above, to
    the bit) decides :71 on the device (``libfedavg_amd_clientloop.so``) and
    gates the fused step on that decision, so an iteration is
    ``guarded_step()`` alone, with no host sync: it queues the gradient pass,
    the guard, the gated step (whose finalize also tracks rho / beta) and an
    asynchronous copy of the record into a pinned ring of ``ahead`` slots.
    ``poll()`` reads whichever slots have arrived, never blocking, and
    ``finish()`` is the one sync of the whole loop.  It needs fused stepping
    (``TypeError`` otherwise; ``guard="auto"`` falls back to ``"host"``);
    ``guard_mode`` says which one the object got.  A tripped guard leaves the
    parameters and the optimizer state exactly as the host guard does (no
    gated launch writes once the gate is set), but the host may have queued up
    to ``ahead`` more forward / backward passes before it noticed: module
    buffers (BatchNorm running statistics) and the RNG stream dropout draws
    from can be ahead of the reference's.  ``trace`` receives ``loss=None``.
    """

    def __init__(self, params, *, stream=None, stats="auto", trace=None, step="torch", optimizer="sgd", adam=None,
                 guard="host", ahead=None):
        self.params = list(params)
        if guard not in ("host", "device", "auto"):
            raise ValueError(f"guard must be 'host', 'device' or 'auto', not {guard!r}")
        if ahead is not None and (int(ahead) != ahead or ahead < 1):
            raise ValueError(f"ahead must be a positive integer, not {ahead!r}")
        if optimizer not in ("sgd", "adam"):
            raise ValueError(f"optimizer must be 'sgd' or 'adam', not {optimizer!r}")
        self.optimizer = optimizer
        self.adam = _adam_hyper(adam) if optimizer == "adam" else None
        if stats not in ("auto", "hip", "torch"):
            raise ValueError(f"stats must be 'auto', 'hip' or 'torch', not {stats!r}")
        if step not in ("torch", "fused", "auto"):
            raise ValueError(f"step must be 'torch', 'fused' or 'auto', not {step!r}")
        fused = _fused_ok(self.params)
        if stats == "hip" and not fused:
            raise TypeError(f"stats='hip' needs {_RULE}")
        self.mode = "hip" if (fused and stats != "torch") else "torch"
        self.trace = trace
        self.stream = stream
        self.host_syncs = 0
        self.loss = None  # the current iteration's loss as a Python float (after after_backward)
        self._begun = False
        if self.mode == "hip":
            self._init_hip()
        else:
            self._last_w = self._last_grads = self._grads = None
            self._rho = self._beta = None
        self.step_mode = "torch"
        if step != "torch" and optimizer == "sgd":
            self._form = sgd_form(self.device, self.dtype) if self.mode == "hip" else None
            if self._form is not None:
                self.step_mode = "fused"
                self._step = _StepPass(self._numel, self.dtype, self.device)
            elif step == "fused":
                raise TypeError(f"step='fused' needs {_STEP_RULE}")
        elif step != "torch":
            h = self.adam
            plain = h["amsgrad"] is True and h["betas"][0] > 0.5 and all(p.requires_grad for p in self.params)
            self._form = adam_form(self.device, self.dtype) if self.mode == "hip" and plain else None
            if self._form is not None:
                self.step_mode = "fused"
                self._t = 0
                self._step = _AdamPass(self._numel, self._offset, self.P, self.dtype, self.device)
            elif step == "fused":
                raise TypeError(f"step='fused' needs {_ADAM_RULE}")
        self.guard_mode = "host"
        if guard != "host":
            if self.step_mode == "fused":
                self.guard_mode = "device"
                self._init_device_guard(DEFAULT_AHEAD if ahead is None else int(ahead))
            elif guard == "device":
                raise TypeError(f"guard='device' needs {_GUARD_RULE}")

    # ------------------------------------------------------------------ fused
    def _init_device_guard(self, ahead):
        lib = _lib.load_clientloop()
        self._guard_name = f"fedavg_client_guard_{_STEP_SUFFIX[self.dtype]}"
        self._guard_fn = getattr(lib, self._guard_name)
        self.ahead = ahead
        with torch.cuda.device(self.device):
            self._ring = torch.zeros(ahead, _REC, dtype=torch.float64, pin_memory=True)
        self._ring_np = self._ring.numpy()
        self._ring_ev = [None] * ahead
        self._issued = 0      # guarded_step() calls so far: the next epoch
        self._seen = 0        # ring records read so far, in order
        self._trip = None     # the epoch of the first trip a record showed
        self.ring_waits = 0   # times a full ring made guarded_step() wait for its oldest record

    def _see(self, i):
        """Read the arrived record of iteration i."""
        rec = self._ring_np[i % self.ahead]
        if self._trip is None and rec[_GATE] != 0.0:
            self._trip = int(rec[_EPOCH])
        self._seen = i + 1

    def _init_hip(self):
        self.device = self.params[0].device
        self.dtype = dt = self.params[0].dtype
        es = self.params[0].element_size()
        if dt == torch.float32:
            self.lib, self._check = _lib.load(), lambda rc, what: _lib.check(rc, what, self.lib)
            self._stats_name, self._track_name = "fedavg_client_stats_f32", "fedavg_client_track"
        else:
            self.lib, self._check = _lib.load_clientvec(), _lib.check_clientvec
            self._stats_name = f"fedavg_client_stats_{_VEC_DTYPES[dt]}"
            self._track_name = f"fedavg_client_track_{_VEC_DTYPES[dt]}"
        self._stats_fn, self._track_fn = getattr(self.lib, self._stats_name), getattr(self.lib, self._track_name)
        ALIGN = 16 // es  # snapshot key offsets are multiples of 16 B
        n = len(self.params)
        self._numel = np.array([p.numel() for p in self.params], dtype=np.int64)
        padded = (self._numel + (ALIGN - 1)) // ALIGN * ALIGN
        self._offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self.P = int(padded.sum())
        self._ptrs = {"w": np.array([p.data_ptr() for p in self.params], dtype=np.int64),
                      "g": np.zeros(n, dtype=np.int64)}
        with torch.cuda.device(self.device):
            if dt == torch.float32:
                nparts = int(self.lib.fedavg_client_stats_partials(self._numel.ctypes.data, n))
                self._ws_bytes = int(self.lib.fedavg_client_stats_workspace(n))
            else:
                nparts = int(self.lib.fedavg_client_stats_vec_partials(self._numel.ctypes.data, n, es))
                self._ws_bytes = int(self.lib.fedavg_client_stats_vec_workspace(n))
            self._snap = {k: torch.zeros(max(self.P, ALIGN), dtype=dt, device=self.device) for k in "wg"}
            self._partials = {k: torch.empty(max(nparts, 1), dtype=torch.float64, device=self.device) for k in "wg"}
            self._host_ws = {k: torch.empty(max(self._ws_bytes, 16), dtype=torch.uint8, pin_memory=True) for k in "wg"}
            self._dev_ws = {k: torch.empty(max(self._ws_bytes, 16), dtype=torch.uint8, device=self.device)
                            for k in "wg"}
            self._rec = torch.zeros(_REC, dtype=torch.float64, device=self.device)
            self._rec_host = torch.zeros(_REC, dtype=torch.float64, pin_memory=True)
            self._ws_free = {k: None for k in "wg"}  # event: the stream has passed the last use of host_ws[k]
            self._staged = {k: None for k in "wg"}   # the pointer table host_ws[k] holds
        self._nparts = nparts

    def _torch_stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.device)

    def _grad_ptrs(self):
        out = self._ptrs["g"]
        for j, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise RuntimeError(f"parameter {j} has no grad (client.py:57 / :69 read every param.grad)")
            if not (g.is_cuda and g.dtype == self.dtype and g.is_contiguous() and g.device == self.device
                    and g.numel() == self._numel[j]):
                raise TypeError(f"parameter {j}: the fused statistics need a contiguous grad of the parameters' "
                                f"dtype ({self.dtype}) on {self.device}")
            out[j] = g.data_ptr()
        return out

    def _pass(self, which: str, has_snap: int):
        """One fused pass over the weights ('w') or the gradients ('g') on the stream."""
        ptrs = self._ptrs["w"] if which == "w" else self._grad_ptrs()
        st = self._torch_stream()
        ev = self._ws_free[which]
        table = ptrs.tobytes()
        if ev is not None and table != self._staged[which]:
            ev.synchronize()  # host_ws gets new bytes below (already passed after an iteration's sync)
        self._staged[which] = table
        with torch.cuda.device(self.device):
            rc = self._stats_fn(
                ptrs.ctypes.data, self._numel.ctypes.data, self._offset.ctypes.data, len(self.params),
                self._snap[which].data_ptr(), self.P, has_snap, self._partials[which].data_ptr(),
                self._partials[which].numel(), self._rec.data_ptr() + 8 * (_W if which == "w" else _G),
                self._host_ws[which].data_ptr(), self._dev_ws[which].data_ptr(), self._host_ws[which].numel(),
                st.cuda_stream)
            self._check(rc, self._stats_name)
            if ev is None:
                ev = self._ws_free[which] = torch.cuda.Event()
            ev.record(st)

    def _read_record(self):
        st = self._torch_stream()
        with torch.cuda.stream(st):
            self._rec_host.copy_(self._rec, non_blocking=True)
        st.synchronize()
        self.host_syncs += 1
        return self._rec_host.numpy()

    # ----------------------------------------------------------------- common
    def _flat(self, grads: bool):
        ts = []
        for j, p in enumerate(self.params):
            t = p.grad if grads else p
            if t is None:
                raise RuntimeError(f"parameter {j} has no grad (client.py:57 / :69 read every param.grad)")
            ts.append(t.view(-1))
        return torch.cat(ts)

    def _emit(self, stage, loss, with_grads=True):
        if self.trace is not None:
            with torch.no_grad():
                self.trace(stage, self._flat(False).detach().clone(),
                           self._flat(True).detach().clone() if with_grads else None, loss)

    def begin(self, loss=None):
        """client.py:52-57: the first snapshots of the weights and, after the
        caller's first backward, of the gradients.  Under the device guard
        ``loss`` is the prologue's loss TENSOR, copied into the record on the
        stream (no ``.item()``)."""
        if self.guard_mode == "device":
            if not torch.is_tensor(loss):
                raise TypeError("begin() under guard='device' takes the prologue's loss tensor: the record keeps it "
                                "on the device as the first last_loss")
            st = self._torch_stream()
            with torch.cuda.stream(st), torch.no_grad():
                self._rec[_LAST:_LAST + 1].copy_(loss.detach().reshape(1))
            loss = None
        if self.mode == "hip":
            self._pass("w", 0)
            self._pass("g", 0)
        else:
            self._last_w = self._flat(False)
            self._last_grads = self._flat(True)
        self._begun = True
        self._emit("begin", loss)

    def after_backward(self, loss_tensor, lr, ratio) -> bool:
        """client.py:69-71: the gradient pass and the guard.  ``True`` when the
        reference would give up: a NaN in the gradients, a NaN loss, or
        ``norm(grads) > lr * ratio * norm(last_w)``."""
        if self.guard_mode == "device":
            raise RuntimeError("after_backward() on an object built with guard='device': guarded_step() takes the "
                               "guard, the step and the bookkeeping of the iteration")
        if not self._begun:
            raise RuntimeError("begin() first")
        if self.mode == "hip":
            self._pass("g", 1)
            st = self._torch_stream()
            with torch.cuda.stream(st), torch.no_grad():
                self._rec[_LOSS:_LOSS + 1].copy_(loss_tensor.detach().reshape(1))
            rec = self._read_record()
            self.loss = float(rec[_LOSS])
            if self.dtype == torch.float32:
                n_g = np.float32(math.sqrt(rec[_G + 1])) if not math.isnan(rec[_G + 1]) else np.float32("nan")
                n_w = np.float32(math.sqrt(rec[_W + 1])) if not math.isnan(rec[_W + 1]) else np.float32("nan")
                with np.errstate(all="ignore"):
                    bound = np.float32(lr * ratio) * n_w  # python_float * fp32 tensor: the scalar rounded to fp32
            else:
                n_g, n_w = _norm_of(float(rec[_G + 1]), self.dtype), _norm_of(float(rec[_W + 1]), self.dtype)
                bound = _guard_bound(n_w, lr * ratio, self.dtype)
            self.grad_norm, self.weight_norm = float(n_g), float(n_w)
            trip = bool(rec[_G] > 0 or math.isnan(self.loss) or n_g > bound)
        else:
            with torch.no_grad():
                grads = self._grads = self._flat(True)
                trip = bool(torch.isnan(grads).sum() > 0 or torch.isnan(loss_tensor)
                            or torch.norm(grads) > lr * ratio * torch.norm(self._last_w))
            self.loss = None if trip else loss_tensor.item()
        self._emit("after_backward", self.loss)
        return trip

    def after_step(self, loss, last_loss):
        """client.py:76-86 after ``optimizer.step()``: the weight pass and the
        running rho / beta; ``loss`` and ``last_loss`` are the Python floats of
        :75 and :56 / :86."""
        if self.step_mode == "fused":
            raise RuntimeError("after_step() on an object built for fused stepping: sgd_step() takes the step and "
                               "keeps no weight snapshot for this pass to compare with")
        if self.mode == "hip":
            self._pass("w", 1)
            base = self._rec.data_ptr()
            with torch.cuda.device(self.device):
                rc = self._track_fn(base + 8 * _STATE, base + 8 * _W, base + 8 * _G, abs(loss - last_loss),
                                    self._torch_stream().cuda_stream)
            self._check(rc, self._track_name)
        else:
            with torch.no_grad():
                w = self._flat(False)
                rho_tmp = abs(loss - last_loss) / torch.norm(w - self._last_w)
                if not self._rho or rho_tmp > self._rho:
                    self._rho = rho_tmp
                beta_tmp = torch.norm(self._grads - self._last_grads) / torch.norm(w - self._last_w)
                if not self._beta or beta_tmp > self._beta:
                    self._beta = beta_tmp
                self._last_w, self._last_grads = w, self._grads
        self._emit("after_step", loss)

    def sgd_step(self, lr, loss, last_loss):
        """client.py:74-86 in one kernel, in place of ``optimizer.step()`` and
        ``after_step()``: ``w -= lr * g`` with torch.optim.SGD's bits, the
        weight record (``sum w'^2`` for the next guard, ``sum rT(w' - w)^2``
        for :78 / :82) and the running rho / beta.  No host sync."""
        if self.step_mode != "fused":
            raise RuntimeError("sgd_step() needs an object built with step='fused' (or 'auto' where it applies): "
                               f"this one steps with torch ({self.step_mode=})")
        if self.optimizer != "sgd":
            raise RuntimeError("sgd_step() on an object built with optimizer='adam': adam_step() takes its step")
        if self.guard_mode == "device":
            raise RuntimeError("sgd_step() on an object built with guard='device': guarded_step() takes its step")
        if not self._begun:
            raise RuntimeError("begin() first")
        st = self._torch_stream()
        base = self._rec.data_ptr()
        self._step.launch(self._ptrs["w"], self._grad_ptrs(), lr, self._form, base + 8 * _W, st)
        torch.autograd.graph.increment_version(self.params)  # the in-place update autograd did not see
        with torch.cuda.device(self.device):
            rc = self._track_fn(base + 8 * _STATE, base + 8 * _W, base + 8 * _G, abs(loss - last_loss), st.cuda_stream)
        self._check(rc, self._track_name)
        self._emit("after_step", loss)

    def adam_step(self, loss, last_loss):
        """client.py:74-86 in one kernel, in place of ``optimizer.step()`` and
        ``after_step()``: the Adam step with torch.optim.Adam's bits on ``w``
        and on the state this object owns, the weight record and the running
        rho / beta.  The first call of an object does not read the state.  No
        host sync."""
        if self.step_mode != "fused":
            raise RuntimeError("adam_step() needs an object built with step='fused' (or 'auto' where it applies): "
                               f"this one steps with torch ({self.step_mode=})")
        if self.optimizer != "adam":
            raise RuntimeError("adam_step() on an object built with optimizer='sgd': sgd_step() takes its step")
        if self.guard_mode == "device":
            raise RuntimeError("adam_step() on an object built with guard='device': guarded_step() takes its step")
        if not self._begun:
            raise RuntimeError("begin() first")
        st = self._torch_stream()
        base = self._rec.data_ptr()
        h = self.adam
        self._t += 1
        coef = adam_coef(h["lr"], *h["betas"], h["eps"], h["weight_decay"], self._t)
        self._step.launch(self._ptrs["w"], self._grad_ptrs(), coef, self._t == 1, self._form, base + 8 * _W, st)
        torch.autograd.graph.increment_version(self.params)  # the in-place update autograd did not see
        with torch.cuda.device(self.device):
            rc = self._track_fn(base + 8 * _STATE, base + 8 * _W, base + 8 * _G, abs(loss - last_loss), st.cuda_stream)
        self._check(rc, self._track_name)
        self._emit("after_step", loss)

    # ------------------------------------------------------------ device guard
    def _need_device_guard(self, what):
        if self.guard_mode != "device":
            raise RuntimeError(f"{what} needs an object built with guard='device' (or 'auto' where it applies): "
                               f"this one decides the guard on the host ({self.guard_mode=})")

    def guarded_step(self, loss_tensor, lr, ratio):
        """client.py:69-86 of one iteration, queued on the stream with no host
        sync: the gradient pass, the loss into the record, the :71 guard on
        the device, the step behind its gate (the finalize also tracks rho /
        beta and moves ``loss`` to ``last_loss``) and a copy of the record
        into slot ``i % ahead`` of the pinned ring.  With the ring full it
        first waits for the oldest record alone, so the host is never more
        than ``ahead`` iterations in front."""
        self._need_device_guard("guarded_step()")
        if not self._begun:
            raise RuntimeError("begin() first")
        i, slot = self._issued, self._issued % self.ahead
        if i - self._seen >= self.ahead:  # the slot's last record (iteration i - ahead) has not been read
            self._ring_ev[slot].synchronize()
            self.ring_waits += 1
            self._see(i - self.ahead)
        st = self._torch_stream()
        self._pass("g", 1)
        with torch.cuda.stream(st), torch.no_grad():
            self._rec[_LOSS:_LOSS + 1].copy_(loss_tensor.detach().reshape(1))
        self._emit("after_backward", None)
        base = self._rec.data_ptr()
        with torch.cuda.device(self.device):
            rc = self._guard_fn(base + 8 * _G, base + 8 * _W, base + 8 * _LOSS, base + 8 * _GATE, float(lr * ratio), i,
                                st.cuda_stream)
        _lib.check_clientloop(rc, self._guard_name)
        gated = (base + 8 * _G, base + 8 * _GATE, base + 8 * _STATE, base + 8 * _LOSS)
        if self.optimizer == "sgd":
            self._step.launch(self._ptrs["w"], self._grad_ptrs(), lr, self._form, base + 8 * _W, st, gated=gated)
        else:
            h = self.adam
            self._t += 1  # past a trip the count runs on, and no gated launch reads the state it counts for
            coef = adam_coef(h["lr"], *h["betas"], h["eps"], h["weight_decay"], self._t)
            self._step.launch(self._ptrs["w"], self._grad_ptrs(), coef, self._t == 1, self._form, base + 8 * _W, st,
                              gated=gated)
        torch.autograd.graph.increment_version(self.params)  # the in-place update autograd did not see
        with torch.cuda.stream(st):
            self._ring[slot].copy_(self._rec, non_blocking=True)
            if self._ring_ev[slot] is None:
                self._ring_ev[slot] = torch.cuda.Event()
            self._ring_ev[slot].record(st)
        self._issued = i + 1
        self._emit("after_step", None)

    def poll(self):
        """The epoch of the first trip among the records that have arrived,
        else ``None``.  Never blocks: ``event.query()`` on the ring slots not
        yet read, in order."""
        self._need_device_guard("poll()")
        while self._seen < self._issued and self._ring_ev[self._seen % self.ahead].query():
            self._see(self._seen)
        return self._trip

    def finish(self):
        """The one sync of the loop: ``(trip_epoch_or_None, loss, beta, rho)``
        from the record as the stream leaves it.  ``loss`` is the last
        iteration's; ``None`` before any ``guarded_step()`` and after a trip
        (iterations queued behind the tripping one have overwritten its slot,
        and the reference returns none either)."""
        self._need_device_guard("finish()")
        rec = self._read_record()
        self._seen = self._issued
        if rec[_GATE] != 0.0:
            self._trip = int(rec[_EPOCH])
        self.loss = float(rec[_LOSS]) if self._issued and self._trip is None else None
        rho = float(rec[_STATE]) if rec[_STATE + 2] else None
        beta = float(rec[_STATE + 1]) if rec[_STATE + 3] else None
        return self._trip, self.loss, beta, rho

    def result(self):
        """``(beta, rho)`` as Python floats (``None`` where no step was taken)."""
        if self.mode == "hip":
            rec = self._read_record()
            rho = float(rec[_STATE]) if rec[_STATE + 2] else None
            beta = float(rec[_STATE + 1]) if rec[_STATE + 3] else None
            return beta, rho
        return (None if self._beta is None else self._beta.item(),
                None if self._rho is None else self._rho.item())


def client_train(self, net, local_iteration, *, keep_on_device=False, stats="auto", trace=None, step="torch",
                 guard="host"):
    """``Client.train(self, net, local_iteration)`` (client.py:38-96) with the
    bookkeeping of :52-86 done by :class:`ClientStepStats`.

    Returns ``(state_dict, loss, beta, rho, acc, cycles)``, or the state_dict
    and five ``None`` when the :71 guard trips.  ``count`` / ``count_end`` and
    ``THRESHOLD_GRADS_RATIO`` are the ones of the module that defines
    ``type(self)`` (the reference's ``client`` module).  ``keep_on_device``
    returns ``net.state_dict()`` without the ``.cpu()`` of :73 / :96.
    ``step`` is :class:`ClientStepStats`'s: with fused stepping and
    ``args.client_optimizer == "sgd"`` one ``sgd_step(args.lr, ...)`` replaces
    ``optimizer.step()`` and ``after_step()``.  Any other
    ``args.client_optimizer`` is the reference's Adam (``lr``, ``wd``,
    amsgrad): with fused stepping one ``adam_step()`` per iteration and no
    torch optimizer at all; where the fused Adam step does not apply it is a
    ``TypeError`` under ``"fused"`` and steps with torch under ``"auto"``.
    ``guard`` is :class:`ClientStepStats`'s: under the device guard an
    iteration is forward, backward and ``guarded_step()``, the loop leaves as
    soon as ``poll()`` shows a trip and ``finish()`` after it is the one host
    sync of the bookkeeping.  The return values are the host guard's to the
    bit; after a trip the parameters are too, while module buffers and the
    RNG stream may be up to ``ahead`` iterations further (see the class).
    """
    mod = sys.modules[type(self).__module__]
    count, count_end, ratio = mod.count, mod.count_end, mod.THRESHOLD_GRADS_RATIO
    sgd = self.args.client_optimizer == "sgd"
    tracker = None
    if not sgd and step != "torch":  # refused, if it is, before anything runs
        try:
            tracker = ClientStepStats(net.parameters(), stats=stats, trace=trace, step=step, optimizer="adam",
                                      adam=dict(lr=self.args.lr, weight_decay=self.args.wd, amsgrad=True), guard=guard)
        except TypeError as e:
            raise TypeError(f"{e}; args.client_optimizer is {self.args.client_optimizer!r}") from None
    if sgd:
        optimizer = torch.optim.SGD(net.parameters(), lr=self.args.lr)
    elif tracker is None or tracker.step_mode != "fused":
        optimizer = torch.optim.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=self.args.lr,
                                     weight_decay=self.args.wd, amsgrad=True)
    cycles = []
    x, labels = next(iter(self.local_training_data))
    x, labels = x.to(self.device), labels.to(self.device)
    net.train()
    if tracker is None:
        tracker = ClientStepStats(net.parameters(), stats=stats, trace=trace, step=step if sgd else "torch",
                                  guard=guard)
    fused = tracker.step_mode == "fused"
    last_loss = self.criterion(net(x), labels)
    torch.nn.utils.clip_grad_norm_(net.parameters(), self.args.clip)
    last_loss.backward()
    done = lambda: net.state_dict() if keep_on_device else net.cpu().state_dict()  # noqa: E731

    def gave_up(epoch):
        logger = getattr(mod, "logger", None)
        if logger is not None:
            logger.warning("grads too large than weights or meets nan with epoch {}".format(epoch))
        return done(), None, None, None, None, None

    if tracker.guard_mode == "device":
        tracker.begin(last_loss.detach())
        for epoch in range(local_iteration):
            start = count()
            net.zero_grad()
            log_probs = net(x)
            loss = self.criterion(log_probs, labels)
            torch.nn.utils.clip_grad_norm_(net.parameters(), self.args.clip)
            loss.backward()
            cycles.append(count_end() - start)
            tracker.guarded_step(loss, self.args.lr, ratio)
            if tracker.poll() is not None:
                break
        trip, loss, beta, rho = tracker.finish()
        if trip is not None:
            return gave_up(trip)
        _, predicted = torch.max(log_probs, -1)
        correct = predicted.eq(labels).sum()
        return done(), loss, beta, rho, correct.item() / labels.size(0), sum(cycles) / len(cycles)
    last_loss = last_loss.item()
    tracker.begin(last_loss)
    for epoch in range(local_iteration):
        start = count()
        net.zero_grad()
        log_probs = net(x)
        loss = self.criterion(log_probs, labels)
        torch.nn.utils.clip_grad_norm_(net.parameters(), self.args.clip)
        loss.backward()
        cycles.append(count_end() - start)
        if tracker.after_backward(loss, self.args.lr, ratio):
            return gave_up(epoch)
        loss = tracker.loss
        if fused and sgd:
            tracker.sgd_step(self.args.lr, loss, last_loss)
        elif fused:
            tracker.adam_step(loss, last_loss)
        else:
            optimizer.step()
            tracker.after_step(loss, last_loss)
        last_loss = loss
    # local_iteration == 0 leaves log_probs unbound, as in the reference (:93)
    _, predicted = torch.max(log_probs, -1)
    correct = predicted.eq(labels).sum()
    beta, rho = tracker.result()
    return done(), loss, beta, rho, correct.item() / labels.size(0), sum(cycles) / len(cycles)


class _Patch:
    """Undo handle of :func:`patch` (also a context manager)."""

    def __init__(self, cls, had, old):
        self.cls, self._had, self._old, self.active = cls, had, old, True

    def undo(self):
        if self.active:
            if self._had:
                setattr(self.cls, "train", self._old)
            else:
                delattr(self.cls, "train")
            self.active = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.undo()
        return False


def patch(cls, *, keep_on_device=False, stats="auto", step="torch", guard="host"):
    """Replace ``cls.train`` (the reference's ``Client.train``) with
    :func:`client_train`; returns a handle whose ``undo()`` restores the class."""
    had = "train" in vars(cls)
    old = vars(cls).get("train")

    def train(self, net, local_iteration):
        return client_train(self, net, local_iteration, keep_on_device=keep_on_device, stats=stats, step=step,
                            guard=guard)

    train.__wrapped_by__ = "mfl_amd.client_stats"
    setattr(cls, "train", train)
    return _Patch(cls, had, old)
