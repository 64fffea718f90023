"""The reference side of test_gpu_sparse_core.py, tested without a GPU.

The GPU tests are only as good as their checkers, so each checker is shown
here to reject a wrong result of the kind it exists for: the tolerance rule
against mutated float32 optimizers (the mutations the engine parity test in
test_gpu_numerics.py lets through), the dedup property checker against
corrupted (uk, inverse, u) triples, and the colliding-key search against
``rng.splitmix64`` itself."""

import pytest
import torch

import sparse_core_ref as ref
from openembedding_amd.core import rng
from openembedding_amd.core.optimizers import (AdamOptimizer, OPTIMIZERS,
                                               make_optimizer)


class _AdamStaleBeta2(AdamOptimizer):
    """Adam whose beta_2^t power is never advanced."""

    def update(self, w, s, counts, g):
        dim = w.shape[1]
        keep = s[:, 2 * dim + 1].clone()
        s[:, 2 * dim + 1] = keep / self.cfg["beta_2"]
        super().update(w, s, counts, g)   # lr_t sees the stale power
        s[:, 2 * dim + 1] = keep


def _mutant(variant):
    cat, hyper = ref.VARIANTS[variant]
    if variant == "adagrad":
        return make_optimizer(cat, **dict(
            hyper, epsilon=hyper["initial_accumulator_value"]))
    if variant == "adam":
        return _AdamStaleBeta2(**hyper)
    if variant == "ftrl_pow":
        return make_optimizer(cat, **dict(hyper, learning_rate_power=-0.5))
    raise KeyError(variant)


def _judge(case, w1, s1, t=0):
    slots, grads, counts = case.step(t)
    return ref.check_step(case, case.weights, case.state, w1, s1, slots,
                          grads, counts, ref.MAX_MARGIN)


def _fp32_step(case, opt=None, t=0):
    slots, grads, counts = case.step(t)
    return ref.step_reference(opt or case.opt, case.weights, case.state,
                              slots, grads, counts, torch.float32)


@pytest.mark.parametrize("dim", [9, 33])
@pytest.mark.parametrize("variant", list(ref.VARIANTS))
def test_rule_accepts_fp32_oracle(variant, dim):
    """Every check of a step (tolerance on w and each state block, the
    untouched-row invariants, the vacuity guard) passes on the unmodified
    float32 oracle, at the loosest margin and at margin 1."""
    case = ref.OptCase(variant, dim, 17)
    for t in range(case.STEPS):
        slots, grads, counts = case.step(t)
        w1, s1 = _fp32_step(case, t=t)
        for margin in (1.0, ref.MAX_MARGIN):
            assert ref.check_step(case, case.weights, case.state, w1, s1,
                                  slots, grads, counts, margin) == []


@pytest.mark.parametrize("dim", [9, 33])
@pytest.mark.parametrize("variant", ["adagrad", "adam", "ftrl_pow"])
def test_rule_rejects_mutated_optimizer(variant, dim):
    """adagrad epsilon replaced by initial_accumulator_value (the c1/c2
    mix-up), adam with beta_2^t not advanced, FTRL forced down the sqrt
    branch at power -0.4: each is rejected on the WEIGHTS alone."""
    case = ref.OptCase(variant, dim, 17)
    w1, s1 = _fp32_step(case, _mutant(variant))
    fails = _judge(case, w1, s1)
    assert any(f.startswith("w:") for f in fails), fails


@pytest.mark.parametrize("dim", [9, 33])
def test_rule_rejects_noop_adadelta(dim):
    case = ref.OptCase("adadelta", dim, 17)
    fails = _judge(case, case.weights.clone(), case.state.clone())
    assert any(f.startswith("w:") for f in fails), fails
    assert any(f.startswith("accum:") for f in fails), fails


def test_rule_rejects_stale_state_with_right_weights():
    """Right weights over an un-advanced beta power: only a state
    comparison sees it."""
    case = ref.OptCase("adam", 9, 17)
    w1, s1 = _fp32_step(case)
    s1[:, 2 * 9 + 1] = case.state[:, 2 * 9 + 1]
    fails = _judge(case, w1, s1)
    assert fails and all(f.startswith("beta_2_t:") for f in fails), fails


@pytest.mark.parametrize("variant", ["sgd_nesterov", "adam"])
def test_rule_rejects_update_of_canary_row(variant):
    case = ref.OptCase(variant, 9, 17)
    slots, grads, counts = case.step(0)
    w1, s1 = _fp32_step(case)
    canary = int(ref.untouched_rows(case.R, slots).nonzero()[0])
    extra = torch.tensor([canary])
    wx, sx = ref.step_reference(case.opt, case.weights, case.state, extra,
                                grads[:1], counts[:1], torch.float32)
    w1[canary], s1[canary] = wx[canary], sx[canary]
    fails = _judge(case, w1, s1)
    assert "weights of a row no live slot names changed" in fails
    assert "state of a row no live slot names changed" in fails


def test_rule_rejects_ignored_device_count():
    """A step applied to all n positions fails when only k are live."""
    case = ref.OptCase("sgd_nesterov", 16, 17)
    slots, grads, counts = case.step(0)
    w1, s1 = _fp32_step(case)
    fails = ref.check_step(case, case.weights, case.state, w1, s1, slots,
                           grads, counts, ref.MAX_MARGIN, live=9)
    assert "weights of a row no live slot names changed" in fails


def test_vacuity_guard_trips_at_default_learning_rates():
    """The engine parity test's blind spot: at adadelta's default
    hyper-parameters the reference step moves the weights too little to
    tell a working kernel from a no-op; the guard says so."""
    case = ref.OptCase("adadelta", 9, 17)
    slots, grads, counts = case.step(0)
    weak = make_optimizer("adadelta")
    w1, s1 = ref.step_reference(weak, case.weights, case.state, slots,
                                grads, counts, torch.float32)
    fails = ref.check_step(case, case.weights, case.state, w1, s1, slots,
                           grads, counts, ref.MAX_MARGIN, opt=weak)
    assert any(f.startswith("vacuous case") for f in fails), fails


def test_rule_fails_on_nan():
    r64 = torch.ones(4, dtype=torch.float64)
    r32 = torch.ones(4)
    got = torch.tensor([1.0, float("nan"), 1.0, 1.0])
    ok, _ = ref.within_reference_error(got, r32, r64, ref.MAX_MARGIN)
    assert not ok
    ok, _ = ref.within_reference_error(r32, r32, r64, 1.0)
    assert ok


def test_ulp32_at():
    assert ref.ulp32_at(1.0) == 2.0 ** -23
    assert ref.ulp32_at(1.5) == 2.0 ** -23
    assert ref.ulp32_at(2.0) == 2.0 ** -22
    assert ref.ulp32_at(0.75) == 2.0 ** -24


def test_cases_cover_every_pairing():
    """Every dim meets every variant by construction; every row count must
    meet both lane-group widths within each variant."""
    assert set(c for c, _ in ref.VARIANTS.values()) == set(OPTIMIZERS)
    for variant in ref.VARIANTS:
        for dims in ([d for d in ref.DIMS if d <= 32],
                     [d for d in ref.DIMS if d > 32]):
            assert ({ref.case_n(variant, d) for d in dims}
                    == set(ref.ROW_COUNTS))


@pytest.mark.parametrize("n", ref.ROW_COUNTS)
def test_case_shape(n):
    """Slots are distinct and in range, some are -1 once n allows, at least
    half the table is never named, and consecutive steps overlap."""
    case = ref.OptCase("adam", 17, n)
    named = set()
    per_step = []
    for t in range(case.STEPS):
        slots, grads, counts = case.step(t)
        live = slots[slots >= 0]
        assert live.numel() == torch.unique(live).numel()
        assert bool((live < case.R).all())
        assert grads.shape == (n, 17) and counts.shape == (n,)
        assert n < 5 or bool((slots == -1).any())
        named |= set(live.tolist())
        per_step.append(set(live.tolist()))
    assert case.R - len(named) >= len(named)
    if n > 1:
        assert per_step[0] & per_step[1] and per_step[0] != per_step[1]
    assert set(case.step(0)[2].tolist()) <= {1, 2, 7}


# ---------------------------------------------------------------- dedup

def _unique_triple(keys):
    uk, inv = torch.unique(keys, return_inverse=True)
    return uk, inv, uk.numel()


def test_dedup_checker_accepts_torch_unique():
    g = torch.Generator().manual_seed(0)
    for keys in (torch.randint(0, 50, (257,), generator=g),
                 ref.full_range_keys(65, g),
                 torch.full((9,), 4, dtype=torch.int64),
                 torch.arange(7, dtype=torch.int64)):
        assert not bool((keys == -1).any())
        assert ref.dedup_violations(keys, *_unique_triple(keys)) == []


def _with_reserved():
    """A valid result for keys holding three occurrences of -1."""
    keys = torch.tensor([5, -1, 9, 5, -1, 2, -1, 9], dtype=torch.int64)
    uk = torch.tensor([5, -1, 9, -1, 2, -1, 0, 0], dtype=torch.int64)
    inv = torch.tensor([0, 1, 2, 0, 3, 4, 5, 2], dtype=torch.int64)
    return keys, uk, inv, 6


def test_dedup_checker_accepts_own_uid_per_reserved_occurrence():
    assert ref.dedup_violations(*_with_reserved()) == []


def test_dedup_checker_rejects_swapped_inverse():
    keys, uk, inv, u = _with_reserved()
    inv[0], inv[2] = inv[2].clone(), inv[0].clone()
    assert "uk[inverse] != keys" in ref.dedup_violations(keys, uk, inv, u)


def test_dedup_checker_rejects_duplicated_uid():
    """Key 5 split over two uids: uk[inverse] == keys still holds."""
    keys, uk, inv, u = _with_reserved()
    uk[6] = 5
    inv[3] = 6
    bad = ref.dedup_violations(keys, uk, inv, 7)
    assert torch.equal(uk[inv], keys)
    assert "a key other than -1 owns more than one uid" in bad


def test_dedup_checker_rejects_merged_reserved_pair():
    keys, uk, inv, u = _with_reserved()
    inv[4] = 1   # second -1 joins the first one's uid
    bad = ref.dedup_violations(keys, uk, inv, u)
    assert torch.equal(uk[inv], keys)
    assert "two occurrences of -1 share a uid" in bad


def test_dedup_checker_rejects_wrong_count_and_range():
    keys, uk, inv, u = _with_reserved()
    assert ref.dedup_violations(keys, uk, inv, u + 1)
    assert ref.dedup_violations(keys, uk, inv, u - 1)


# ------------------------------------------------------- colliding keys

@pytest.mark.parametrize("mask,homes", [(1023, [5]), (15, [13, 14, 15]),
                                        (63, [61, 62, 63]),
                                        (255, [253, 254, 255])])
def test_colliding_keys_collide(mask, homes):
    count = 200 if mask == 1023 else 8
    ks = ref.colliding_keys(mask, homes, count)
    assert ks.numel() == count == torch.unique(ks).numel()
    assert bool((ks >= 0).all())
    h = rng.splitmix64(ks) & mask
    assert set(h.tolist()) <= set(homes)


# ------------------------------------------------- truncated normal init

NORMAL = dict(mean=0.5, stddev=0.2, truncated=0.5)
NORMAL_SEED = 11


def test_normal_fp64_chain_matches_fp32_oracle():
    """The float64 chain is the float32 initializer evaluated in double:
    away from the cut they agree to float32 rounding, resampling really
    happens at this cut, and under 1% of the elements lie within 1e-4 of
    it (the cap the GPU test asserts for the same seed and keys)."""
    g = torch.Generator().manual_seed(5)
    keys = ref.full_range_keys(67, g)
    r64, unsure = ref.normal_init_fp64(NORMAL_SEED, keys, 130, **NORMAL)
    r32 = rng.init_rows("normal", NORMAL, NORMAL_SEED, keys, 130)
    assert float(unsure.float().mean()) < 0.01
    first = rng._normal(NORMAL_SEED, keys.view(-1, 1).expand(67, 130),
                        torch.arange(130).view(1, -1).expand(67, 130), 0)
    assert float((first > NORMAL["truncated"]).float().mean()) > 0.25
    sure = ~unsure
    assert float((r32.double() - r64)[sure].abs().max()) < 2e-6
    z = (r64 - NORMAL["mean"]) / NORMAL["stddev"]
    assert float(z.max()) <= NORMAL["truncated"] + 1e-12
