"""The keyed passes behind :mod:`client_stats`: the buffers of a native call
over a model's tensors and the reuse rule of its pinned key table
(:class:`_KeyPass`), the fused SGD and Adam steps as its users, the statistics
library per dtype, the host side of the :71 guard's arithmetic and the whole
local loop of a linear softmax client as one launch (:class:`_LinearLoop`), or of a
round's whole cohort of them (:class:`_Cohort`), the evaluation of a linear
model on every client's dataset as one call (:class:`EvalSet`), and central
training's chain of steps over every client's batch (:class:`_Chain`)."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib

# dtype -> entry suffix of the clientvec library; fp32 is the product library's
_VEC_DTYPES = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float64: "f64"}
FUSED_DTYPES = (torch.float32, *_VEC_DTYPES)
_RULE = "contiguous parameters on one GPU, all of one dtype among fp32, bf16, fp16 and fp64"
_STEP_SUFFIX = {torch.float32: "f32", **_VEC_DTYPES}
ADAM_SITES = 4  # A g + wd w, B the lerp, C the addcmul, E the addcdiv: bit i of a form mask fuses site i

# The statistics pass per dtype, the product library against clientvec: (loader, check, statistics entry, track entry,
# stem of the ``_partials`` / ``_workspace`` sizing entries, whether ``_partials`` also takes the element size).
# _lib.check reports from the product library once that is loaded, which the loader has done by then.
_STATS_LIBS = {torch.float32: (_lib.load, _lib.check, "fedavg_client_stats_f32", "fedavg_client_track",
                               "fedavg_client_stats", False),
               **{dt: (_lib.load_clientvec, _lib.check_clientvec, f"fedavg_client_stats_{s}",
                       f"fedavg_client_track_{s}", "fedavg_client_stats_vec", True) for dt, s in _VEC_DTYPES.items()}}


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


class _KeyPass:
    """What a native call over ``n`` keys needs besides its own arguments: the
    ``partials`` doubles and the pinned ``host_ws`` / device ``dev_ws`` pair
    its key table is staged through.  Every client entry ends in ``partials,
    partial_elems, stats, host_ws, dev_ws, ws_bytes, stream`` (a gated one adds
    its four gate pointers), writes its table into ``host_ws`` on the host and
    queues the copy to ``dev_ws``.  The reuse rule: new bytes go into
    ``host_ws`` only after the stream has passed the last call that shipped
    the old ones; a call with the same pointer tables rewrites the same bytes
    and need not wait."""

    def __init__(self, nparts, ws_bytes, device):
        self.device = device
        with torch.cuda.device(device):
            self.partials = torch.empty(max(nparts, 1), dtype=torch.float64, device=device)
            self.host_ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, pin_memory=True)
            self.dev_ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
        self._free = None    # event: the stream has passed the last use of host_ws
        self._staged = None  # the pointer tables host_ws holds

    def stage(self, table) -> bool:
        """The reuse rule for a call that ships ``table`` (bytes); ``True``
        when it had to wait for the last call."""
        wait = self._free is not None and table != self._staged
        if wait:
            self._free.synchronize()  # already passed after an iteration's host sync
        self._staged = table
        return wait

    def call(self, fn, name, check, table, head, stats_ptr, st, gated=()):
        """``fn(*head, <the common tail>, *gated)`` on torch stream ``st``,
        its status through ``check``; the record goes to the device doubles
        at ``stats_ptr``."""
        self.stage(table)
        with torch.cuda.device(self.device):
            rc = fn(*head, self.partials.data_ptr(), self.partials.numel(), stats_ptr, self.host_ws.data_ptr(),
                    self.dev_ws.data_ptr(), self.host_ws.numel(), st.cuda_stream, *gated)
            check(rc, name)
            if self._free is None:
                self._free = torch.cuda.Event()
            self._free.record(st)


class _FusedStep(_KeyPass):
    """A step entry ``name`` of ``lib`` over keys of ``numel`` elements, sized
    by ``lib``'s ``{sizing}_partials`` / ``{sizing}_workspace``, and its gated
    twin in the loop library (``..._step_gated_*``, looked up when first used)."""

    def __init__(self, lib, check, name, sizing, numel, dtype, device):
        self.name, self.fn, self.check = name, getattr(lib, name), check
        self.numel = np.ascontiguousarray(numel, dtype=np.int64)
        n = len(self.numel)
        es = torch.empty(0, dtype=dtype).element_size()
        super().__init__(int(getattr(lib, sizing + "_partials")(self.numel.ctypes.data, n, es)),
                         int(getattr(lib, sizing + "_workspace")(n)), device)
        self._gated = None

    def _launch(self, w_ptrs, g_ptrs, head, stats_ptr, st, gated):
        fn, name, check = self.fn, self.name, self.check
        if gated is not None:
            if self._gated is None:
                name = self.name.replace("_step_", "_step_gated_")
                self._gated = (getattr(_lib.load_clientloop(), name), name, _lib.check_clientloop)
            fn, name, check = self._gated
        self.call(fn, name, check, w_ptrs.tobytes() + g_ptrs.tobytes(),
                  (w_ptrs.ctypes.data, g_ptrs.ctypes.data, self.numel.ctypes.data, *head), stats_ptr, st, gated or ())


class _StepPass(_FusedStep):
    """The buffers of ``fedavg_client_sgd_step_*`` calls over tensors of
    ``numel`` elements, and the call."""

    def __init__(self, numel, dtype, device):
        super().__init__(_lib.load_clientstep(), _lib.check_clientstep,
                         f"fedavg_client_sgd_step_{_STEP_SUFFIX[dtype]}", "fedavg_client_step", numel, dtype, device)

    def launch(self, w_ptrs, g_ptrs, lr, form, stats_ptr, st, gated=None):
        """w -= lr * g over the tensors at w_ptrs / g_ptrs on torch stream
        ``st``; the record goes to the 4 device doubles at ``stats_ptr``.
        ``gated``: the device addresses ``(g_stats, gate, state, loss)`` of
        ``fedavg_client_sgd_step_gated_*``, which then takes the call."""
        self._launch(w_ptrs, g_ptrs, (len(self.numel), float(lr), form), stats_ptr, st, gated)


def adam_coef(lr, beta1, beta2, eps, weight_decay, t):
    """The seven coefficients of ``fedavg_client_adam_step_*`` for step ``t``
    (from 1), in Python floats exactly as torch/optim/adam.py forms them."""
    t = float(t)
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    step_size = (lr / bias_correction1) * -1
    return np.array([weight_decay, 1 - beta1, beta2, 1 - beta2, bias_correction2 ** 0.5, eps, step_size],
                    dtype=np.float64)


class _AdamPass(_FusedStep):
    """The optimizer state (three planes ``m, v, vmax`` of ``state_elems``
    elements in one zeroed buffer, key j at ``offset[j]``), the buffers of
    ``fedavg_client_adam_step_*`` calls and the call."""

    def __init__(self, numel, offset, state_elems, dtype, device):
        super().__init__(_lib.load_clientadam(), _lib.check_clientadam,
                         f"fedavg_client_adam_step_{_STEP_SUFFIX[dtype]}", "fedavg_client_adam", numel, dtype, device)
        self.offset = np.ascontiguousarray(offset, dtype=np.int64)
        self.state_elems = int(state_elems)
        es = torch.empty(0, dtype=dtype).element_size()
        with torch.cuda.device(device):
            self.state = torch.zeros(3 * max(self.state_elems, 16 // es), dtype=dtype, device=device)

    def plane(self, i):
        """Plane i (0 ``m``, 1 ``v``, 2 ``vmax``) as a view of the state."""
        return self.state[i * self.state_elems:(i + 1) * self.state_elems]

    def launch(self, w_ptrs, g_ptrs, coef, first, form, stats_ptr, st, gated=None):
        """``coef``: :func:`adam_coef`'s; ``first``: the state is not read;
        ``gated``: as ``_StepPass.launch``'s (``fedavg_client_adam_step_gated_*``)."""
        self._launch(w_ptrs, g_ptrs, (self.offset.ctypes.data, len(self.numel), self.state.data_ptr(), self.state_elems,
                                      coef.ctypes.data, int(bool(first)), form), stats_ptr, st, gated)


# ------------------------------------------------------------------ the fused local loop of a linear client
LINEAR_LOOPS = {"linear": 0, "linear_sigmoid": 1}  # client_train's ``loop`` -> the library's activation code
_LINEAR_RULE = ("loop='linear' / 'linear_sigmoid' needs a model of exactly two parameters, a contiguous fp32 [C, D] "
                "weight and a [C] bias that both require grad, on one GPU; a batch whose x.flatten(1) has D columns "
                "with int64 labels of its length; a default nn.CrossEntropyLoss (mean reduction, no class weights, "
                "no label smoothing); sizes inside fedavg_client_linear_limits (B <= 64, one resident batch) or "
                "fedavg_client_stream_limits (longer batches, streamed in groups of rows); and a form of the step "
                "kernel that leaves torch's bits on this GPU (sgd_form / adam_form)")


def linear_limits():
    """``(max B, max D, max C, resident bytes)`` of ``fedavg_client_linear_limits``."""
    out = [ctypes.c_int64() for _ in range(4)]
    _lib.load_clientlinear().fedavg_client_linear_limits(*[ctypes.byref(v) for v in out])
    return tuple(v.value for v in out)


def linear_stream_limits():
    """``(max B, max D, max C, LDS bytes of the two row buffers)`` of ``fedavg_client_stream_limits``."""
    out = [ctypes.c_int64() for _ in range(4)]
    _lib.load_clientstream().fedavg_client_stream_limits(*[ctypes.byref(v) for v in out])
    return tuple(v.value for v in out)


class _LinearLoop:
    """One ``fedavg_client_linear_loop_f32`` call, or for a batch of more than
    ``linear_limits()[0]`` samples one ``fedavg_client_linear_stream_f32``
    call (the same arguments and record): the checks of what the
    caller asserts by choosing the loop (``TypeError`` naming the rule, before
    anything runs) and the launch.  The record and Adam's coefficient table
    lie in pinned host memory kept per device: the kernel writes the one and
    reads the other where they lie, and ``run`` returns only after the stream
    has passed the launch, so the next call may reuse both."""

    _pinned = {}  # device -> [record of 8 doubles, coefficient table [rows, 7]]

    def __init__(self, params, x, labels, criterion, form_of, wide=False):
        """``form_of(device)``: the step form for fp32 on ``device``, or ``None``.  ``wide``: the sizes are held to
        :func:`wide_limits` (the plan is then :class:`_Cohort`'s, which alone may run it)."""
        def refuse(why):
            raise TypeError(f"{why}: {_LINEAR_RULE}")

        params = list(params)
        if len(params) != 2:
            refuse(f"the model has {len(params)} parameters, not two")
        w, b = params
        if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous():
            refuse("the first parameter is no contiguous fp32 [C, D] weight")
        if b.dtype != torch.float32 or b.shape != (w.shape[0],) or not b.is_contiguous():
            refuse("the second parameter is no contiguous fp32 [C] bias")
        if not (w.requires_grad and b.requires_grad):
            refuse("a parameter does not require grad")
        C, D = w.shape
        if x.dim() < 2 or x.dtype != torch.float32 or x.flatten(1).shape[1] != D:
            refuse(f"x.flatten(1) is no fp32 batch of {D} columns")
        B = x.shape[0]
        if labels.dtype != torch.int64 or labels.shape != (B,):
            refuse(f"the labels are not int64 of length {B}")
        if not (type(criterion) is torch.nn.CrossEntropyLoss and criterion.reduction == "mean"
                and criterion.weight is None and criterion.label_smoothing == 0.0 and criterion.ignore_index == -100):
            refuse("the criterion is no default nn.CrossEntropyLoss")
        self.resident_b = linear_limits()[0]
        max_b, max_d, max_c, _ = linear_stream_limits()
        if wide:
            _, max_b, max_d, max_c, _ = wide_limits()
            if not (1 <= B <= max_b and 1 <= D <= max_d and 2 <= C <= max_c):
                refuse(f"B = {B}, D = {D}, C = {C} lie outside the wide cohort's B <= {max_b}, D <= {max_d}, "
                       f"2 <= C <= {max_c}")
        elif not (1 <= B <= max_b and 1 <= D <= max_d and 2 <= C <= max_c):
            refuse(f"B = {B}, D = {D}, C = {C} lie outside B <= {max_b} (resident up to {self.resident_b}, streamed "
                   f"above), D <= {max_d}, 2 <= C <= {max_c}")
        if not (w.is_cuda and b.device == w.device and x.device == w.device and labels.device == w.device):
            refuse("the parameters and the batch are not on one GPU")
        self.form = form_of(w.device)
        if self.form is None:
            refuse("no form of the step kernel leaves torch's bits on this GPU")
        self.w, self.b, self.x, self.labels = w, b, x.flatten(1).contiguous(), labels.contiguous()
        self.B, self.D, self.C, self.device = B, D, C, w.device

    def _buffers(self, rows):
        held = self._pinned.get(self.device)
        if held is None or held[1].shape[0] < rows:
            with torch.cuda.device(self.device):
                held = [torch.zeros(8, dtype=torch.float64, pin_memory=True),
                        torch.zeros(max(rows, 16), 7, dtype=torch.float64, pin_memory=True)]
            self._pinned[self.device] = held
        return held

    def run(self, iters, activation, lr, lr_ratio, adam=None):
        """The loop on the current stream and the one host sync; returns the
        record as 8 floats.  ``adam``: ``(beta1, beta2, eps, weight_decay)``
        of the reference's Adam, else plain SGD."""
        rec, table = self._buffers(iters if adam else 0)
        if adam:
            for t in range(iters):
                table[t] = torch.from_numpy(adam_coef(lr, *adam, t + 1))
        st = torch.cuda.current_stream(self.device)
        if self.B <= self.resident_b:
            name, load, check = "fedavg_client_linear_loop_f32", _lib.load_clientlinear, _lib.check_clientlinear
        else:
            name, load, check = "fedavg_client_linear_stream_f32", _lib.load_clientstream, _lib.check_clientstream
        with torch.cuda.device(self.device), torch.no_grad():
            rc = getattr(load(), name)(
                self.w.data_ptr(), self.b.data_ptr(), self.x.data_ptr(), self.labels.data_ptr(), self.B, self.D,
                self.C, iters, activation, 1 if adam else 0, float(lr), float(lr_ratio), self.form,
                table.data_ptr() if adam else None, rec.data_ptr(), st.cuda_stream)
        check(rc, name)
        torch.autograd.graph.increment_version([self.w, self.b])  # the in-place update autograd did not see
        st.synchronize()
        return rec.tolist()


# ------------------------------------------------------------------ a round's cohort of linear clients, one launch
def cohort_limits():
    """``(max K, max B, max D, max C)`` of ``fedavg_client_cohort_limits``."""
    out = [ctypes.c_int64() for _ in range(4)]
    _lib.load_clientcohort().fedavg_client_cohort_limits(*[ctypes.byref(v) for v in out])
    return tuple(v.value for v in out)


class _Cohort:
    """One ``fedavg_client_cohort_f32`` call: every client of ``batches`` trained from the same model, client ``k``
    into row ``k``.  The :class:`_LinearLoop` rules are checked once for the model (with the first batch) and per
    client for the batch (``TypeError`` naming the rule, before anything runs).  The client table, the records and
    Adam's coefficient table lie in pinned host memory kept per device; ``run`` returns only after the stream has
    passed the launch, so the next call may reuse them.  ``split``: the call is ``fedavg_client_cohort_split_f32``'s,
    each client's batch split across workgroups that walk ``slices_per_group`` slices each (``None``:
    :func:`cosplit_default_slices`), and the plan owns that entry's workspace, allocated by ``run`` after
    :func:`_fits` has let its size pass.  ``wide``: the call is ``fedavg_client_cohort_wide_f32``'s, with the sizes
    held to :func:`wide_limits` instead, ``slices_per_group`` at most :func:`wide_max_slices` (``None``:
    :func:`wide_default_slices`) and a workspace kept the same way."""

    _pinned = {}  # device -> [client table [K, 4] int64, records [K, 8], coefficient table [rows, 7]]

    def __init__(self, params, batches, criterion, form_of, split=False, slices_per_group=None, wide=False):
        if wide and split:
            raise ValueError("wide=True and split=True are two entries: choose one")
        first = _LinearLoop(params, *batches[0], criterion, form_of, wide=wide)
        self.w, self.b, self.form, self.D, self.C, self.device = first.w, first.b, first.form, first.D, first.C, first.device
        max_k, max_b = wide_limits()[:2] if wide else cohort_limits()[:2]
        if len(batches) > max_k:
            raise TypeError(f"a cohort of {len(batches)} clients exceeds {max_k}: {_LINEAR_RULE}")
        self.x, self.labels = [first.x], [first.labels]
        for k, (x, labels) in enumerate(batches[1:], 1):
            B = x.shape[0] if x.dim() >= 2 else 0
            if not (x.dtype == torch.float32 and 1 <= B <= max_b and x.flatten(1).shape[1] == self.D
                    and labels.dtype == torch.int64 and labels.shape == (B,)
                    and x.device == self.device and labels.device == self.device):
                raise TypeError(f"client {k}: no fp32 batch of 1 to {max_b} rows of {self.D} columns with int64 labels "
                                f"of its length on {self.device}: {_LINEAR_RULE}")
            self.x.append(x.flatten(1).contiguous())
            self.labels.append(labels.contiguous())
        self.K, self.P = len(batches), self.C * self.D + self.C
        self.B = [x.shape[0] for x in self.x]
        self.split, self.wide, self.workspace = bool(split), bool(wide), None
        if split:
            if slices_per_group is None:
                slices_per_group = cosplit_default_slices(self.B, self.D)
            if not (isinstance(slices_per_group, int) and slices_per_group >= 1):
                raise ValueError(f"slices_per_group must be an int >= 1, not {slices_per_group!r}")
            self.q = slices_per_group
        if wide:
            most = wide_max_slices(self.C)
            if slices_per_group is None:
                slices_per_group = wide_default_slices(self.B, self.C)
            if not (isinstance(slices_per_group, int) and 1 <= slices_per_group <= most):
                raise ValueError(f"slices_per_group must be an int in [1, {most}] at C = {self.C}, not {slices_per_group!r}")
            self.q = slices_per_group

    def _buffers(self, iters):
        held = self._pinned.get(self.device)
        if held is None or held[0].shape[0] < self.K or held[2].shape[0] < iters:
            with torch.cuda.device(self.device):
                held = [torch.zeros(max(self.K, 16), 4, dtype=torch.int64, pin_memory=True),
                        torch.zeros(max(self.K, 16), 8, dtype=torch.float64, pin_memory=True),
                        torch.zeros(max(iters, 16), 7, dtype=torch.float64, pin_memory=True)]
            self._pinned[self.device] = held
        return held

    def run(self, rows, iters, activation, lr, lr_ratio, adam=None):
        """The launch on the current stream and the one host sync; returns the ``[K, 8]`` records as lists, record
        ``k`` client ``k``'s.  ``rows``: the device ``[K, ld]`` fp32 buffer.  Entries go longest batch first (the
        hardware starts workgroups in order), each with ``row`` = its client's position."""
        table, rec, coef = self._buffers(iters if adam else 0)
        order = sorted(range(self.K), key=lambda k: -self.B[k])
        table.numpy()[:self.K] = [(self.x[k].data_ptr(), self.labels[k].data_ptr(), self.B[k], k) for k in order]
        if adam:
            for t in range(iters):
                coef[t] = torch.from_numpy(adam_coef(lr, *adam, t + 1))
        st = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.no_grad():
            model = torch.cat([self.w.detach().reshape(-1), self.b.detach()])
            args = (model.data_ptr(), rows.data_ptr(), rows.stride(0), table.data_ptr(), self.K, self.D, self.C, iters,
                    activation, 1 if adam else 0, float(lr), float(lr_ratio), self.form,
                    coef.data_ptr() if adam else None, rec.data_ptr())
            if self.split or self.wide:
                sizes = [self.B[k] for k in order]
                nbytes = (wide_workspace_bytes if self.wide else cosplit_workspace_bytes)(sizes, self.D, self.C, self.q,
                                                                                         bool(adam))
                if self.workspace is None or self.workspace.numel() < nbytes:
                    self.workspace = None  # the old one first
                    _fits(nbytes, self.device, "wide" if self.wide else "batch-split")
                    self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                if self.wide:
                    name, check, load = "fedavg_client_cohort_wide_f32", _lib.check_clientwide, _lib.load_clientwide
                else:
                    name, check, load = "fedavg_client_cohort_split_f32", _lib.check_clientcosplit, _lib.load_clientcosplit
                rc = getattr(load(), name)(*args, self.q, self.workspace.data_ptr(), self.workspace.numel(), st.cuda_stream)
            else:
                name, check = "fedavg_client_cohort_f32", _lib.check_clientcohort
                rc = _lib.load_clientcohort().fedavg_client_cohort_f32(*args, st.cuda_stream)
        check(rc, name)
        st.synchronize()
        return rec[:self.K].tolist()


COSPLIT_MANY_GROUPS, COSPLIT_MANY_SLICES = 1024, 4  # the default slices_per_group (the sweep behind it)


def cosplit_groups(B, D, slices_per_group):
    """The workgroups of the batch-split cohort's gradient launch for clients of ``B`` rows of ``D`` columns: with
    ``R = split_slice_rows(D)``, ``sum_k ceil(ceil(B_k / R) / slices_per_group)``."""
    R = split_slice_rows(D)
    return sum(-(-(-(-b // R)) // slices_per_group) for b in B)


def cosplit_default_slices(B, D):
    """The ``slices_per_group`` of ``cohort_train(split=True)`` when none is given: 1 while one slice a workgroup
    keeps the gradient launch at or below ``COSPLIT_MANY_GROUPS`` workgroups, else ``COSPLIT_MANY_SLICES``."""
    return 1 if cosplit_groups(B, D, 1) <= COSPLIT_MANY_GROUPS else COSPLIT_MANY_SLICES


def cosplit_workspace_bytes(B, D, C, slices_per_group, adam):
    """``fedavg_client_cosplit_workspace_bytes`` for clients of ``B`` rows; ``ValueError`` outside its ranges."""
    sizes = np.ascontiguousarray(B, dtype=np.int64)
    nbytes = _lib.load_clientcosplit().fedavg_client_cosplit_workspace_bytes(
        sizes.ctypes.data, len(sizes), D, C, slices_per_group, 1 if adam else 0)
    if nbytes <= 0:
        raise ValueError(f"no workspace for {len(sizes)} clients, D = {D}, C = {C}, slices_per_group = "
                         f"{slices_per_group}: outside the ranges of fedavg_client_cohort_split_f32")
    return nbytes


def _fits(nbytes, device, kind="batch-split"):
    """Refuse, before any launch, a workspace that ``torch.cuda.mem_get_info`` says cannot fit (memory torch holds
    cached and unused counts as free)."""
    free = torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    if nbytes > free:
        raise ValueError(f"the {kind} cohort needs a workspace of {nbytes} bytes and {device} has {free} free: "
                         f"raise slices_per_group, or train without {'wide' if kind == 'wide' else 'split'}=True")


# ------------------------------------------------------------------ the cohort at up to 128 classes and 4096 columns
def wide_limits():
    """``(max K, max B, max D, max C, max P)`` of ``fedavg_client_wide_limits``."""
    out = [ctypes.c_int64() for _ in range(5)]
    _lib.load_clientwide().fedavg_client_wide_limits(*[ctypes.byref(v) for v in out])
    return tuple(v.value for v in out)


def wide_slice_rows():
    """The rows of one slice of ``fedavg_client_cohort_wide_f32``, at every shape."""
    return _lib.load_clientwide().fedavg_client_wide_slice_rows()


def wide_max_slices(C):
    """The largest ``slices_per_group`` of ``fedavg_client_cohort_wide_f32`` at ``C`` classes (0 outside its range)."""
    return _lib.load_clientwide().fedavg_client_wide_max_slices(C)


def wide_default_slices(B, C):
    """The ``slices_per_group`` of ``cohort_train(wide=True)`` when none is given: 1 while one slice a workgroup keeps
    the gradient launch at or below ``COSPLIT_MANY_GROUPS`` workgroups, else ``COSPLIT_MANY_SLICES`` or the most
    ``C`` allows."""
    R = wide_slice_rows()
    if sum(-(-b // R) for b in B) <= COSPLIT_MANY_GROUPS:
        return 1
    return min(COSPLIT_MANY_SLICES, wide_max_slices(C))


def wide_workspace_bytes(B, D, C, slices_per_group, adam):
    """``fedavg_client_wide_workspace_bytes`` for clients of ``B`` rows; ``ValueError`` outside its ranges."""
    sizes = np.ascontiguousarray(B, dtype=np.int64)
    nbytes = _lib.load_clientwide().fedavg_client_wide_workspace_bytes(
        sizes.ctypes.data, len(sizes), D, C, slices_per_group, 1 if adam else 0)
    if nbytes <= 0:
        raise ValueError(f"no workspace for {len(sizes)} clients, D = {D}, C = {C}, slices_per_group = "
                         f"{slices_per_group}: outside the ranges of fedavg_client_cohort_wide_f32")
    return nbytes


# ------------------------------------------------------------------ central_train's chain of steps, one launch
def chain_limits():
    """``(max K, max B, max D, max C)`` of ``fedavg_client_chain_limits``."""
    out = [ctypes.c_int64() for _ in range(4)]
    _lib.load_clientchain().fedavg_client_chain_limits(*[ctypes.byref(v) for v in out])
    return tuple(v.value for v in out)


def split_limits():
    """``(max K, max B, max D, max C)`` of the batch-split chain: the chain's, which its entry checks first."""
    return chain_limits()


def split_slice_rows(D):
    """The rows of one slice of ``fedavg_client_chain_split_f32`` at ``D`` columns (0 outside its range)."""
    return _lib.load_clientsplit().fedavg_client_split_slice_rows(D)


def adam_coef_rows(lr, beta1, beta2, eps, weight_decay, first, n):
    """Rows ``[n, 7]`` of :func:`adam_coef` for the steps ``first .. first + n - 1`` (from 1): the constant columns
    filled at once, the three powers of a row in Python floats exactly as torch/optim/adam.py forms them."""
    rows = np.empty((n, 7), dtype=np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 5] = weight_decay, 1 - beta1, beta2, 1 - beta2, eps
    ts = [float(t) for t in range(first, first + n)]
    rows[:, 4] = [(1 - beta2 ** t) ** 0.5 for t in ts]
    rows[:, 6] = [(lr / (1 - beta1 ** t)) * -1 for t in ts]
    return rows


class _Chain:
    """The ``fedavg_client_chain_f32`` calls of one chain: one model stepped on every batch of ``batches`` in their
    order, round after round.  The :class:`_LinearLoop` rules are checked once for the model (with the first batch)
    and per client for the batch (``TypeError`` naming the rule, before anything runs).  The plan keeps the pinned
    client table in client order, the pinned losses and record, and on the device Adam's coefficient rows and its
    ``m, v, vmax``.  ``split``: the calls are ``fedavg_client_chain_split_f32``'s, each step's batch split across
    workgroups, and the plan also keeps that entry's workspace, sized from the table's largest batch."""

    def __init__(self, params, batches, form_of, split=False):
        first = _LinearLoop(params, *batches[0], torch.nn.CrossEntropyLoss(), form_of)
        self.w, self.b, self.form, self.D, self.C, self.device = first.w, first.b, first.form, first.D, first.C, first.device
        max_k, max_b, _, _ = chain_limits()
        if len(batches) > max_k:
            raise TypeError(f"a chain over {len(batches)} clients exceeds {max_k}: {_LINEAR_RULE}")
        self.x, self.labels = [first.x], [first.labels]
        for k, (x, labels) in enumerate(batches[1:], 1):
            B = x.shape[0] if x.dim() >= 2 else 0
            if not (x.dtype == torch.float32 and 1 <= B <= max_b and x.flatten(1).shape[1] == self.D
                    and labels.dtype == torch.int64 and labels.shape == (B,)
                    and x.device == self.device and labels.device == self.device):
                raise TypeError(f"client {k}: no fp32 batch of 1 to {max_b} rows of {self.D} columns with int64 labels "
                                f"of its length on {self.device}: {_LINEAR_RULE}")
            self.x.append(x.flatten(1).contiguous())
            self.labels.append(labels.contiguous())
        self.K, self.P = len(batches), self.C * self.D + self.C
        with torch.cuda.device(self.device):
            self.table = torch.zeros(self.K, 4, dtype=torch.int64, pin_memory=True)
            self.rec = torch.zeros(8, dtype=torch.float64, pin_memory=True)
        self.table.numpy()[:] = [(x.data_ptr(), y.data_ptr(), x.shape[0], 0) for x, y in zip(self.x, self.labels)]
        self.workspace = None
        if split:
            nbytes = _lib.load_clientsplit().fedavg_client_split_workspace_bytes(
                max(x.shape[0] for x in self.x), self.D, self.C)
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def _call(self, *args, stream):
        """One call of the plan's entry: the chain's arguments, and for the split entry its workspace after them."""
        if self.workspace is None:
            _lib.check_clientchain(_lib.load_clientchain().fedavg_client_chain_f32(*args, stream),
                                   "fedavg_client_chain_f32")
        else:
            rc = _lib.load_clientsplit().fedavg_client_chain_split_f32(*args, self.workspace.data_ptr(),
                                                                       self.workspace.numel(), stream)
            _lib.check_clientsplit(rc, "fedavg_client_chain_split_f32")

    def run(self, rounds, per_launch, activation, lr, adam=None):
        """``rounds`` rounds in launches of ``per_launch`` rounds on the current stream, one host sync per launch,
        ``state`` and ``step0`` carried from launch to launch; the parameters are updated in place after the last one.
        Returns ``(losses, None)``, or ``(None, k)`` when client ``k`` has a label outside ``[0, C)`` (nothing was
        stepped then).  ``adam``: ``(beta1, beta2, eps, weight_decay)`` of the reference's Adam, else plain SGD."""
        st = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.no_grad():
            losses = torch.zeros(rounds, dtype=torch.float64, pin_memory=True)
            model = torch.cat([self.w.detach().reshape(-1), self.b.detach()])
            state = coef = None
            if adam:
                state = torch.zeros(3 * self.P, dtype=torch.float32, device=self.device)
                coef = torch.from_numpy(adam_coef_rows(lr, *adam, 1, rounds * self.K)).to(self.device)
            for r0 in range(0, rounds, per_launch):
                n = min(per_launch, rounds - r0)
                self._call(
                    model.data_ptr(), state.data_ptr() if adam else None, self.table.data_ptr(), self.K, self.D,
                    self.C, n, r0 * self.K, activation, 1 if adam else 0, float(lr), self.form,
                    coef[r0 * self.K:].data_ptr() if adam else None, losses[r0:].data_ptr(), self.rec.data_ptr(),
                    stream=st.cuda_stream)
                st.synchronize()
                if self.rec[0]:
                    return None, int(self.rec[1])
            self.w.copy_(model[:self.C * self.D].view(self.C, self.D))
            self.b.copy_(model[self.C * self.D:])
        return losses.tolist(), None


# ------------------------------------------------------------------ every client's evaluation, one call
EVAL_CHUNK_ROWS = 256  # the kernel's unit of work: a run of at most this many rows of one client
_EVAL_RULE = ("the one-call evaluation needs a model of exactly two parameters, a contiguous fp32 [C, D] weight and a "
              "[C] bias on the set's GPU; per client one batch whose x.flatten(1) is fp32 with D columns and whose "
              "labels are int64 of its length; a default nn.CrossEntropyLoss; sizes inside fedavg_client_eval_limits")


def eval_limits():
    """``(max K, max B, max D, max C)`` of ``fedavg_client_eval_limits``."""
    out = [ctypes.c_int64() for _ in range(4)]
    _lib.load_clienteval().fedavg_client_eval_limits(*[ctypes.byref(v) for v in out])
    return tuple(v.value for v in out)


class EvalSet:
    """The datasets one ``fedavg_client_eval_f32`` call evaluates a model on: each loader's one batch, drawn as
    client.py:108-109 draws it (the batch is the client's whole dataset, main_fedavg.py:232), flattened and uploaded
    to ``device``; the pinned client table, longest batch first, each entry's ``slot`` its position among the loaders
    that are not ``None`` (those are skipped, as fedavg_trainer.py:483 skips them); the workspace and the pinned
    records.  Built once and reused for every later evaluation.  The batch rules are checked here and the model's in
    :meth:`run` (``TypeError`` naming the rule, before anything runs)."""

    def __init__(self, loaders, device, criterion=None):
        def refuse(why):
            raise TypeError(f"{why}: {_EVAL_RULE}")

        self.device = torch.device(device)
        if self.device.type != "cuda":
            refuse(f"{self.device} is no GPU")
        if criterion is not None and not (
                type(criterion) is torch.nn.CrossEntropyLoss and criterion.reduction == "mean" and criterion.weight is None
                and criterion.label_smoothing == 0.0 and criterion.ignore_index == -100):
            refuse("the criterion is no default nn.CrossEntropyLoss")
        max_k, max_b, max_d, _ = eval_limits()
        loaders = list(loaders)
        self.n, self.positions, self.x, self.labels, self.D = len(loaders), [], [], [], None
        for pos, loader in enumerate(loaders):
            if loader is None:
                continue
            x, labels = next(iter(loader))
            B = x.shape[0] if x.dim() >= 2 else 0
            if self.D is None and B:
                self.D = x.flatten(1).shape[1]
            if not (x.dtype == torch.float32 and 1 <= B <= max_b and 1 <= self.D <= max_d
                    and x.flatten(1).shape[1] == self.D and labels.dtype == torch.int64 and labels.shape == (B,)):
                refuse(f"client {pos}: no fp32 batch of 1 to {max_b} rows of {self.D} (at most {max_d}) columns with "
                       "int64 labels of its length")
            self.positions.append(pos)
            self.x.append(x.to(self.device).flatten(1).contiguous())
            self.labels.append(labels.to(self.device).contiguous())
        self.K = len(self.x)
        if not 1 <= self.K <= max_k:
            refuse(f"{self.K} clients with data lie outside 1 to {max_k}")
        self.B = [x.shape[0] for x in self.x]
        order = sorted(range(self.K), key=lambda k: -self.B[k])
        with torch.cuda.device(self.device):
            self.table = torch.zeros(self.K, 4, dtype=torch.int64, pin_memory=True)
            self.rec = torch.zeros(self.K, 4, dtype=torch.float64, pin_memory=True)
        self.table.numpy()[:] = [(self.x[k].data_ptr(), self.labels[k].data_ptr(), self.B[k], k) for k in order]
        need = _lib.load_clienteval().fedavg_client_eval_workspace_bytes(self.table.data_ptr(), self.K, self.D)
        if need < 0:
            _lib.check_clienteval(int(need), "fedavg_client_eval_workspace_bytes")
        self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)

    def run(self, params, activation):
        """One call on the current stream and the one host sync; returns ``(C, records)``, record ``k`` =
        ``[loss sum, correct count, label flag, B]`` of the ``k``-th loader that is not ``None``."""
        params = list(params)
        if len(params) != 2:
            raise TypeError(f"the model has {len(params)} parameters, not two: {_EVAL_RULE}")
        w, b = params
        _, _, _, max_c = eval_limits()
        if not (w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.shape[1] == self.D
                and 2 <= w.shape[0] <= max_c and b.dtype == torch.float32 and b.shape == (w.shape[0],)
                and b.is_contiguous() and w.device == self.device and b.device == self.device):
            raise TypeError(f"the parameters are no contiguous fp32 [C, {self.D}] weight and [C] bias with "
                            f"2 <= C <= {max_c} on {self.device}: {_EVAL_RULE}")
        st = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.no_grad():
            model = torch.cat([w.detach().reshape(-1), b.detach()])
            rc = _lib.load_clienteval().fedavg_client_eval_f32(
                model.data_ptr(), self.table.data_ptr(), self.K, self.D, w.shape[0], activation, self.rec.data_ptr(),
                self.workspace.data_ptr(), self.workspace.numel(), st.cuda_stream)
        _lib.check_clienteval(rc, "fedavg_client_eval_f32")
        st.synchronize()
        return w.shape[0], self.rec.tolist()
