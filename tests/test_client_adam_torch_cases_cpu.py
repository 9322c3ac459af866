"""The chains tests/test_gpu_client_adam_torch.py sends through torch.optim.Adam
and the fused step (client_adam_cases.chain) meet the conditions they were
built for, shown on the host reference alone: amsgrad engaged (vmax' > v'), a
subnormal and an underflowed second moment in the model's type, a chain that
stays finite, every (aligned, misaligned) pair of w and g in the flat layout,
and inputs on which the form mask still matters.  The GPU test asserts the
same conditions on torch's own state."""
import pytest
import torch

import client_adam_cases as C


def _counts(key, hyper):
    return {s: C.chain_counts(C.chain_reference(key, s, hyper), C.chain(key, s).g) for s in C.CHAIN_SCALES[key]}


@pytest.mark.parametrize("key", C.KEYS)
def test_the_chains_meet_their_conditions(key):
    counts = {hyper: _counts(key, hyper) for hyper in C.condition_sets(key)}
    for hyper, by_scale in counts.items():
        for scale, c in by_scale.items():
            print(f"{key} ({hyper}) {C.scale_id(scale)}: vmax' > v' {c['vmax_gt_v']} subnormal v' {c['subnormal_v']} "
                  f"underflowed v' {c['underflowed_v']} finite {all(c['finite'])}")
    C.check_conditions(key, counts)


@pytest.mark.parametrize("key", C.KEYS)
def test_the_chain_is_twelve_steps_of_nine_odd_keys_and_the_gradient_shrinks(key):
    U, P = C.UNIT[key], C.KPER[key]
    for scale in C.CHAIN_SCALES[key]:
        c = C.chain(key, scale)
        assert c.numel.tolist() == [1, 3, P - 1, P, P + 1, 63, U - 1, U + 1, 2 * U + 3] and c.numel.sum() < 50_000
        assert c.steps == len(c.g) == C.CHAIN_STEPS == 12
        early = torch.stack([g.double().abs().mean() for g in c.g[:6]])
        late = torch.stack([g.double().abs().mean() for g in c.g[6:]])
        assert 28 < float(early.mean() / late.mean()) < 36  # s, then s / 32
        assert len({tuple(g[:64].tolist()) for g in c.g}) == 12  # a fresh gradient every step
    # the flat layout: every sub-16-B offset of w, and all four (aligned, misaligned) pairs of w and g
    assert set(c.off["w"].tolist()) == set(range(P))
    assert set(zip((c.off["w"] == 0).tolist(), (c.off["g"] == 0).tolist())) == \
        {(True, True), (True, False), (False, True), (False, False)}
    for side in "wg":
        assert all((c.start[side] - c.off[side]) % P == 0)
        ends = c.start[side] + c.numel
        assert all(c.start[side][1:] - ends[:-1] >= C.PAD) and c.start[side][0] >= C.PAD \
            and c.size[side] - ends[-1] >= C.PAD  # sentinels around every key


@pytest.mark.parametrize("key", ("f32", "f64"))
def test_every_bit_of_the_mask_still_matters_under_the_probes_hyperparameters(key):
    """Set (d): mask 15 against each 15 ^ bit stores different bits somewhere in the chains, so the comparison with
    torch stays sensitive to the form and not just to the values; in fp32 also in the small-model chain, where every
    magnitude is one the probe never sees.  fp64's small-model chain is left out here (every fma of it goes
    through rational arithmetic on the host, seconds per mask), so fp64's smallest magnitudes are not shown to be
    sensitive to the form; a difference is required at g ~ N(0, 1) and, summed, over the other scales."""
    scales = C.CHAIN_SCALES[key] if key == "f32" else C.CHAIN_SCALES[key][:-1]
    for bit in (1, 2, 4, 8):
        n = {s: C.stored_differ(C.chain(key, s), 15, 15 ^ bit, **C.HYPERS["d"]) for s in scales}
        print(f"{key} (d) bit {bit}: " + ", ".join(f"{C.scale_id(s)} {v}" for s, v in n.items()))
        assert n[scales[0]] > 0 and sum(n.values()) > 0
        if key == "f32":
            assert n[scales[-1]] > 0


@pytest.mark.parametrize("key", C.KEYS)
def test_the_special_values_reach_what_they_are_planted_for(key):
    c = C.specials(key)
    for hyper in ("a", "d"):
        ref = [res for res, _ in c.reference(15, **C.HYPERS[hyper])]
        w1, m1, v1, x1 = ref[0]
        assert torch.isnan(w1[0]) and torch.isnan(w1[-1]) and torch.isinf(v1[1]) and torch.isinf(v1[2])
        assert float(v1[3]) == 0.0
        # the planted g^2 = 2^-130 (bf16, fp32) times value = 0.001 is below bf16's least subnormal: there it underflows
        assert bool(C.subnormal(v1).any()) or (key, hyper) == ("bf16", "a")
        # step 2 starts from inf and NaN in m, v and vmax
        assert not torch.isfinite(m1).all() and not torch.isfinite(v1).all() and not torch.isfinite(x1).all()
        assert torch.isnan(ref[1][0][0]) and c.steps == 2
        if key == "f16":
            assert torch.isinf(v1[7])  # 6e4 squared
