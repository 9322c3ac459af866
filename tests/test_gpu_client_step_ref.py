"""fedavg_client_sgd_step_{f32,bf16,f16,f64} on the MI355X, BOTH forms of each,
against the exact host reference of tests/client_step_ref.py (itself checked
against rational arithmetic in tests/test_client_step_ref_cpu.py): the w' bits
and the record, on the launches of tests/client_step_cases.py (one ragged
key; 130 and 4100 keys at mixed alignments, each side in one buffer; a key of
more than 256 units), on the special values, and what torch's own fp16 step
is next to the two forms.

Every launch that claims to tell the forms apart first asserts, on the host,
that the reference's forms differ on 32 or more of its elements and on one or
more in every place of the launch (Case.assert_discriminates).

The sums: the reference's are math.fsum, exact.  The kernel adds at most 32
squares per thread in order, then 6 DPP steps, 3 waves, and in the finalize
kernel at most ceil(units / 256) partials per thread and 8 tree steps: under
64 roundings on any path, so it is within 64 * 2^-53 < 1e-14 of the exact
sum, inside the suite's SUM_RTOL = 1e-11 for every case here."""
import math

import pytest
import torch

import client_step_cases as C
import client_step_ref as R
from mfl_amd import _lib, client_stats
from test_gpu_client_step import SUM_RTOL, Step, _torch_sgd

pytestmark = pytest.mark.gpu

FORMS = (0, 1)


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    return _lib.load_clientstep()


def _same_sum(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == want or abs(got - want) <= SUM_RTOL * abs(want)


def _assert_bits(got, want, what):
    """Equal bits; NaN where the reference has NaN (payloads are not compared)."""
    nan_got, nan_want = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_got, nan_want), what
    wrong = (R.bits(got) != R.bits(want)) & ~nan_want
    assert not bool(wrong.any()), (what, int(wrong.sum()), torch.nonzero(wrong).view(-1)[:8].tolist())


def _assert_record(stats, want, what):
    nans, s_w, s_d = want
    print(f"{what}: got {stats.tolist()} want {(nans, s_w, s_d, 0)}")
    assert stats[0] == float(nans) and stats[3] == 0.0, what
    assert _same_sum(float(stats[1]), s_w) and _same_sum(float(stats[2]), s_d), what


def _run(lib, dev, key, form, lr, numel, w_buf, g_buf, w_views, g_views):
    """One call; returns the record and the two buffers back on the host."""
    stats = Step(lib, dev, numel, key).run(w_views, g_views, lr, form)
    return stats, w_buf.cpu(), g_buf.cpu()


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", C.CASES)
@pytest.mark.parametrize("key", C.KEYS)
def test_bits_and_record_equal_the_reference(lib, dev, key, name, form):
    c = C.case(name, key)
    c.assert_discriminates()  # before anything runs: this launch can tell form 0 from form 1
    if name in ("k130", "k4100"):
        assert len(c.branches()) == 4
    want, rec = c.reference(form)
    host_w, host_g = c.host_buffer("w"), c.host_buffer("g")
    w_buf, g_buf = host_w.to(dev), host_g.to(dev)
    assert w_buf.data_ptr() % 16 == 0 and g_buf.data_ptr() % 16 == 0
    stats, w_out, g_out = _run(lib, dev, key, form, C.LR, c.numel.tolist(), w_buf, g_buf, c.views(w_buf, "w"),
                               c.views(g_buf, "g"))
    what = f"{name} {key} form {form}"
    _assert_bits(w_out[torch.from_numpy(c.pos["w"])], want, what)
    assert bool((w_out[c.gaps("w")] == C.SENTINEL).all()), what  # nothing stored outside a key
    assert torch.equal(R.bits(g_out), R.bits(host_g)), what      # g and its sentinels unchanged
    _assert_record(stats, rec, what)


# ------------------------------------------------------------- special values
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nonfinite", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("key", C.KEYS)
def test_special_values_equal_the_reference(lib, dev, key, offset, nonfinite, form):
    """test_gpu_client_step.test_special_values' inputs (and the same without
    NaN and inf in g, so that the sums are numbers, or inf), the expected bits
    and record from the reference: subnormal results in every type, overflow
    to inf in fp16 at lr 40."""
    w, g = C.specials(key, nonfinite)
    n, lead = len(w), C.PAD + offset
    for lr in (0.03, 40.0):
        want, rec = R.reference(key, form, R.alpha_of(key, lr), w, g)
        bufs = []
        for t in (w, g):
            host = torch.full((lead + n + C.PAD,), C.SENTINEL, dtype=t.dtype)
            host[lead:lead + n] = t
            bufs.append((host, host.to(dev)))
        (host_w, w_buf), (host_g, g_buf) = bufs
        assert w_buf.data_ptr() % 16 == 0 and g_buf.data_ptr() % 16 == 0
        stats, w_out, g_out = _run(lib, dev, key, form, lr, [n], w_buf, g_buf, [w_buf[lead:lead + n]],
                                   [g_buf[lead:lead + n]])
        what = f"specials {key} offset {offset} nonfinite {nonfinite} form {form} lr {lr}"
        _assert_bits(w_out[lead:lead + n], want, what)
        assert bool((w_out[:lead] == C.SENTINEL).all()) and bool((w_out[lead + n:] == C.SENTINEL).all()), what
        assert torch.equal(torch.isnan(g_out), torch.isnan(host_g)), what
        same = ~torch.isnan(host_g)
        assert torch.equal(R.bits(g_out)[same], R.bits(host_g)[same]), what
        _assert_record(stats, rec, what)
        tiny = torch.finfo(w.dtype).smallest_normal
        assert bool(((want.abs() < tiny) & (want != 0)).any()), what  # a subnormal result
        if nonfinite:
            assert rec[0] >= 2 and math.isnan(rec[1]) and math.isnan(rec[2])
        else:
            assert rec[0] == 0
        if key == "f16" and lr == 40.0:
            assert bool(torch.isinf(want[8:11]).any()), what  # the step overflowed fp16
            if not nonfinite:
                assert rec[1] == math.inf


# ------------------------------------------------------------- the fp16 finding
def test_fp16_torch_is_neither_form_but_the_single_rounding(lib, dev):
    """Why fp16 is not in client_stats.STEP_DTYPES: torch's own fp16 SGD step on
    this GPU equals neither form of the kernel, and equals r16(exact(alpha g +
    w)), one rounding (client_step_ref.step_f16_once): the specification of a
    form the kernel does not have.  On the first 512 elements of the seeded
    pool, the elements on which the reference's forms differ, and 256 of those
    on which one rounding and form 1 part."""
    assert torch.float16 not in client_stats.STEP_DTYPES
    alpha = R.alpha_of("f16", C.LR)
    pw, pg = C.pool("f16")
    once_all = R.step_f16_once(alpha, pw, pg)
    parts = torch.nonzero(R.bits(once_all) != R.bits(R.step("f16", 1, alpha, pw, pg))).view(-1)[:256]
    idx = torch.unique(torch.cat([torch.arange(512), torch.from_numpy(C.pool_differ("f16", C.LR)), parts]))
    w, g = pw[idx].clone(), pg[idx].clone()
    ref = [R.step("f16", form, alpha, w, g) for form in FORMS]
    once = once_all[idx]
    assert int((R.bits(ref[0]) != R.bits(ref[1])).sum()) >= C.MIN_DIFFER
    assert int((R.bits(once) != R.bits(ref[1])).sum()) >= C.MIN_DIFFER
    torch_w = _torch_sgd([w], [g], C.LR, dev)[0].cpu()
    g_dev = g.to(dev)
    kernel = []
    for form in FORMS:
        w_dev = w.to(dev)
        Step(lib, dev, [len(w)], "f16").run([w_dev], [g_dev], C.LR, form)
        kernel.append(w_dev.cpu())
        _assert_bits(kernel[form], ref[form], f"fp16 form {form}")
    off = [int((R.bits(torch_w) != R.bits(k)).sum()) for k in kernel]
    off_once = int((R.bits(torch_w) != R.bits(once)).sum())
    print(f"fp16, {len(w)} elements: torch differs from form 0 on {off[0]}, from form 1 on {off[1]}, "
          f"from the single rounding on {off_once}")
    assert off[0] > 0 and off[1] > 0
    assert off_once == 0
