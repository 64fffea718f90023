"""Reference side of tests/test_gpu_sparse_core.py: plain torch, no GPU.

Everything the GPU tests compare against lives here so that it can itself
be tested on a machine without a GPU (tests/test_sparse_core_checkers.py):

  - the optimizer cases (visible hyper-parameters, perturbed state, permuted
    slot vectors) and the single-step stepper built on
    ``SparseOptimizer.update`` (dtype-generic: float64 = the oracle, float32
    = the measure of the oracle's own rounding);
  - the reference-derived tolerance rule;
  - the property checker for a batch dedup result;
  - the CPU search for keys that collide under ``rng.splitmix64``;
  - a float64 evaluation of the truncated-normal initializer chain.
"""

from __future__ import annotations

import math

import torch

from openembedding_amd.core import rng
from openembedding_amd.core.optimizers import make_optimizer

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1

# --------------------------------------------------------- tolerance rule

# Upper limit of any margin used with the rule below. The margin covers the
# device's sqrtf / division / powf rounding differently from the CPU's; a
# kernel that needs more than this is wrong, not imprecise.
MAX_MARGIN = 8.0


def ulp32_at(x: float) -> float:
    """One float32 ulp at magnitude ``x``."""
    x = abs(float(x))
    if x == 0.0 or not math.isfinite(x):
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


def error_figures(got, ref32, ref64):
    """(ek, e32, ulp, ratio) for one output tensor.

    e32 = max|fp32-oracle - fp64-oracle| is the reference's own rounding
    and never involves the code under test; ek = max|got - fp64-oracle|;
    ulp = one float32 ulp at the tensor's largest magnitude. ``ratio`` is
    the smallest margin with ek <= margin * e32 + ulp (inf if none does).
    """
    if ref64.numel() == 0:
        return 0.0, 0.0, 0.0, 0.0
    r64 = ref64.double()
    e32 = float((ref32.double() - r64).abs().max())
    ek = float((got.double() - r64).abs().max())
    ulp = ulp32_at(float(r64.abs().max()))
    if not math.isfinite(ek):
        ratio = math.inf
    elif ek <= ulp:
        ratio = 0.0
    elif e32 == 0.0:
        ratio = math.inf
    else:
        ratio = (ek - ulp) / e32
    return ek, e32, ulp, ratio


def within_reference_error(got, ref32, ref64, margin):
    """The rule: ek <= margin * e32 + one fp32 ulp at the largest magnitude.
    Returns (ok, figures). A NaN anywhere in ``got`` fails."""
    assert margin <= MAX_MARGIN
    figs = error_figures(got, ref32, ref64)
    ek, e32, ulp, _ = figs
    return bool(ek <= margin * e32 + ulp), figs


# ------------------------------------------------------- optimizer cases

# Every hyper-parameter is far enough from its neutral value that dropping
# or swapping it moves the weights by much more than the tolerance.
_FTRL = dict(learning_rate=0.1, initial_accumulator_value=0.3,
             l1_regularization_strength=0.05,
             l2_regularization_strength=0.1,
             l2_shrinkage_regularization_strength=0.05, beta=0.2)
VARIANTS = {
    "default": ("default", dict(learning_rate=0.25)),
    "default_lr0": ("default", dict(learning_rate=0.0)),
    "adadelta": ("adadelta", dict(learning_rate=0.5, rho=0.8, epsilon=1e-2)),
    "adagrad": ("adagrad", dict(learning_rate=0.1,
                                initial_accumulator_value=0.3,
                                epsilon=1e-2)),
    "adam": ("adam", dict(learning_rate=0.05, beta_1=0.7, beta_2=0.9,
                          epsilon=1e-2)),
    "adamax": ("adamax", dict(learning_rate=0.05, beta_1=0.7, beta_2=0.9,
                              epsilon=1e-2)),
    "ftrl_pow": ("ftrl", dict(_FTRL, learning_rate_power=-0.4)),
    "ftrl_sqrt": ("ftrl", dict(_FTRL, learning_rate_power=-0.5)),
    "rmsprop_mom0": ("rmsprop", dict(learning_rate=0.05, rho=0.8,
                                     momentum=0.0, epsilon=1e-2)),
    "rmsprop_mom03": ("rmsprop", dict(learning_rate=0.05, rho=0.8,
                                      momentum=0.3, epsilon=1e-2)),
    "sgd_mom0": ("sgd", dict(learning_rate=0.1, momentum=0.0)),
    "sgd_mom09": ("sgd", dict(learning_rate=0.1, momentum=0.9)),
    "sgd_nesterov": ("sgd", dict(learning_rate=0.1, momentum=0.9,
                                 nesterov=True)),
    "test": ("test", dict(learning_rate=0.1, flip=2.5, init=1.0)),
}
# one variant per category, for the sweeps that run each category once
CATEGORY_VARIANT = {
    "default": "default", "adadelta": "adadelta", "adagrad": "adagrad",
    "adam": "adam", "adamax": "adamax", "ftrl": "ftrl_pow",
    "rmsprop": "rmsprop_mom03", "sgd": "sgd_nesterov", "test": "test",
}

DIMS = [1, 15, 16, 17, 32, 33, 63, 64, 65, 130]   # G=16 up to 32, 64 above
ROW_COUNTS = [1, 5, 16, 17, 67]   # cross 4 and 16 row groups per block


def case_n(variant: str, dim: int) -> int:
    """Row count of the (variant, dim) case. DIMS holds five dims per G, so
    for a fixed variant the rotation gives every n to both G values."""
    v = list(VARIANTS).index(variant)
    return ROW_COUNTS[(DIMS.index(dim) + v) % len(ROW_COUNTS)]


def state_blocks(category: str, dim: int):
    """[(name, start, stop, kind)] of the optimizer's state row."""
    d = dim
    return {
        "default": [],
        "adadelta": [("accum", 0, d, "pos"),
                     ("accum_update", d, 2 * d, "pos")],
        "adagrad": [("accum", 0, d, "pos")],
        "adam": [("m", 0, d, "signed"), ("v", d, 2 * d, "pos"),
                 ("beta_1_t", 2 * d, 2 * d + 1, "beta_1"),
                 ("beta_2_t", 2 * d + 1, 2 * d + 2, "beta_2")],
        "adamax": [("m", 0, d, "signed"), ("v", d, 2 * d, "pos"),
                   ("beta_1_t", 2 * d, 2 * d + 1, "beta_1")],
        "ftrl": [("accum", 0, d, "pos"), ("linear", d, 2 * d, "signed")],
        "rmsprop": [("accum", 0, d, "pos"), ("moment", d, 2 * d, "signed")],
        "sgd": [("moment", 0, d, "signed")],
        "test": [("flip_state", 0, 1, "flip"), ("pad", 1, 2, "pad")],
    }[category]


class OptCase:
    """One optimizer case: a small fp32 table with canary rows, and three
    steps that each touch a different overlapping subset of its rows
    through a permuted, non-contiguous slot vector with -1 entries."""

    STEPS = 3

    def __init__(self, variant: str, dim: int, n: int, seed: int = 0):
        self.variant, self.dim, self.n = variant, dim, n
        self.category, hyper = VARIANTS[variant]
        self.opt = make_optimizer(self.category, **hyper)
        self.sd = self.opt.state_dim(dim)
        g = torch.Generator().manual_seed(
            1000 * list(VARIANTS).index(variant) + 10 * dim + n + seed)
        self._h = n // 2                 # window shift between steps
        pool = n + 2 * self._h           # rows any step may name
        self.R = 2 * pool + 3            # at least as many canary rows
        self._pool = torch.randperm(self.R, generator=g)[:pool]
        self.weights = torch.randn(self.R, dim, generator=g) * 0.5
        self.state = torch.zeros(self.R, self.sd)
        if self.sd:
            self.opt.train_init(self.state, dim)
            self._perturb(g)
        self._g = g
        self._steps = [self._make_step(t) for t in range(self.STEPS)]

    def _perturb(self, g):
        cfg, R = self.opt.cfg, self.R
        row = torch.arange(R)
        for _, a, b, kind in state_blocks(self.category, self.dim):
            blk = self.state[:, a:b]
            if kind == "pos":
                blk += torch.rand(R, b - a, generator=g) * 0.5 + 0.05
            elif kind == "signed":
                blk += torch.randn(R, b - a, generator=g) * 0.3
            elif kind in ("beta_1", "beta_2"):
                # rows start at different powers of beta
                blk *= (cfg[kind] ** (row % 3).float()).unsqueeze(1)
            elif kind == "flip":
                flipped = (row % 2 == 1).unsqueeze(1)
                blk.copy_(torch.where(flipped, cfg["flip"] - blk, blk))

    def _make_step(self, t):
        n, g = self.n, self._g
        slots = self._pool[t * self._h: t * self._h + n].clone()
        slots[torch.arange(n) % 7 == 3] = -1
        grads = torch.randn(n, self.dim, generator=g)
        counts = torch.tensor([1, 2, 7], dtype=torch.int64).repeat(
            n // 3 + 1)[:n].clone()
        return slots, grads, counts

    def step(self, t):
        """(slots int64 [n], grads f32 [n, dim], counts int64 [n])."""
        return self._steps[t]

    def blocks(self):
        return state_blocks(self.category, self.dim)


def live_positions(slots, live=None):
    """Positions of ``slots`` the kernel must apply: below ``live`` (the
    device count, None = all) and with a slot >= 0."""
    n = slots.numel() if live is None else int(live)
    pos = torch.arange(slots.numel())
    return pos[(pos < n) & (slots >= 0)]


def step_reference(opt, w, s, slots, grads, counts, dtype, live=None):
    """One optimizer step from the snapshot (w, s) in ``dtype``; rows that
    no live position names come back as converted copies."""
    w = w.to(dtype).clone()
    s = s.to(dtype).clone()
    pos = live_positions(slots, live)
    if pos.numel():
        rows = slots[pos]
        wr, sr = w[rows], s[rows]
        opt.update(wr, sr, counts[pos], grads[pos].to(dtype))
        w[rows] = wr
        s[rows] = sr
    return w, s


def untouched_rows(R, slots, live=None):
    """Rows of an R-row table that no live position names."""
    keep = torch.ones(R, dtype=torch.bool)
    keep[slots[live_positions(slots, live)]] = False
    return keep


def bits_equal(a, b) -> bool:
    """Bitwise equality of two float32 tensors (NaN payloads included)."""
    if a.shape != b.shape:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(torch.int32),
                       b.contiguous().view(torch.int32))


def check_step(case, w0, s0, w1, s1, slots, grads, counts, margin,
               live=None, opt=None, report=None):
    """Judge one step (w0, s0) -> (w1, s1) of ``case``. Returns a list of
    failure strings (empty = pass); ``report`` collects the per-tensor
    figures as (name, ek, e32, ulp, ratio)."""
    opt = opt or case.opt
    fails = []
    w64, s64 = step_reference(opt, w0, s0, slots, grads, counts,
                              torch.float64, live)
    w32, s32 = step_reference(opt, w0, s0, slots, grads, counts,
                              torch.float32, live)
    keep = untouched_rows(case.R, slots, live)
    if not bits_equal(w1[keep], w0[keep]):
        fails.append("weights of a row no live slot names changed")
    if not bits_equal(s1[keep], s0[keep]):
        fails.append("state of a row no live slot names changed")
    touched = ~keep
    if case.opt.cfg.get("learning_rate") == 0:
        if not bits_equal(w1, w0):
            fails.append("lr == 0 changed the weights")
    elif bool(touched.any()):
        # vacuity guard: the reference step itself must be visible
        med = float((w64[touched] - w0[touched].double()).abs().median())
        if not med >= 1e-3:
            fails.append(f"vacuous case: median |dw| {med:.3g} < 1e-3")
    tensors = [("w", w1, w32, w64)]
    tensors += [(name, s1[:, a:b], s32[:, a:b], s64[:, a:b])
                for name, a, b, _ in case.blocks()]
    for name, got, r32, r64 in tensors:
        ok, (ek, e32, ulp, ratio) = within_reference_error(got, r32, r64,
                                                           margin)
        if report is not None:
            report.append((name, ek, e32, ulp, ratio))
        if not ok:
            fails.append(f"{name}: ek {ek:.3g} > {margin} * e32 {e32:.3g} "
                         f"+ ulp {ulp:.3g} (ratio {ratio:.3g})")
    return fails


# ------------------------------------------------------------ batch dedup

def dedup_violations(keys, uk, inverse, u):
    """Properties of a batch dedup result (uk [>=u], inverse [n], u) for
    ``keys`` [n]; returns the violated ones (empty = valid). The reserved
    key -1 is documented to give every OCCURRENCE its own uid."""
    bad = []
    n = keys.numel()
    u = int(u)
    if inverse.numel() != n:
        return ["inverse length != n"]
    if n == 0:
        return [] if u == 0 else ["u != 0 for an empty batch"]
    if not (0 <= u <= uk.numel()):
        return [f"u = {u} outside [0, {uk.numel()}]"]
    if bool((inverse < 0).any()) or bool((inverse >= u).any()):
        return ["inverse outside [0, u)"]
    if not torch.equal(uk[inverse], keys):
        bad.append("uk[inverse] != keys")
    res = keys == -1
    n_res = int(res.sum())
    n_distinct = int(torch.unique(keys[~res]).numel())
    if u != n_distinct + n_res:
        bad.append(f"u = {u} != distinct {n_distinct} + reserved {n_res}")
    uid_plain = torch.unique(inverse[~res])
    if uid_plain.numel() != n_distinct:
        bad.append("a key other than -1 owns more than one uid")
    uid_res = inverse[res]
    if torch.unique(uid_res).numel() != n_res:
        bad.append("two occurrences of -1 share a uid")
    if n_res and n_distinct and bool(torch.isin(uid_res, uid_plain).any()):
        bad.append("an occurrence of -1 shares a uid with another key")
    return bad


def colliding_keys(mask: int, homes, count: int, limit: int = 400_000):
    """The first ``count`` non-negative integers below ``limit`` whose
    ``splitmix64(k) & mask`` is one of ``homes`` (found by a CPU scan; the
    device hash is the same function)."""
    ks = torch.arange(limit, dtype=torch.int64)
    h = rng.splitmix64(ks) & mask
    sel = torch.isin(h, torch.as_tensor(list(homes), dtype=torch.int64))
    out = ks[sel][:count]
    assert out.numel() == count, (out.numel(), count)
    return out


def full_range_keys(n: int, g) -> torch.Tensor:
    """n keys uniform over the signed 64-bit range; the extremes and -2
    are planted when there is room (never the reserved -1)."""
    hi = torch.randint(-(1 << 31), 1 << 31, (n,), generator=g,
                       dtype=torch.int64)
    lo = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
    keys = hi * (1 << 32) + lo
    keys[keys == -1] = -2
    for i, v in enumerate((I64_MIN, I64_MAX, -2)):
        if n > 3 * i + 1:
            keys[3 * i + 1] = v
    return keys


# -------------------------------------------------- truncated normal init

def normal_init_fp64(seed, keys, dim, mean, stddev, truncated,
                     near=1e-4):
    """float64 evaluation of the initializer's Box-Muller chain from the
    same 24-bit uniforms. Returns (rows [n, dim] float64, unsure [n, dim]
    bool): ``unsure`` marks elements where the standardized sample of an
    attempt the chain visited lies within ``near`` of the cut, so that a
    float32 evaluation may legitimately take the other branch."""
    n = keys.numel()
    k = keys.view(-1, 1).expand(n, dim).to(torch.int64)
    c = torch.arange(dim, dtype=torch.int64).view(1, -1).expand(n, dim)

    def z_of(attempt):
        u1 = rng.uniform01(seed, k, c, attempt=2 * attempt).double()
        u2 = rng.uniform01(seed, k, c, attempt=2 * attempt + 1).double()
        return (torch.sqrt(-2.0 * torch.log(1.0 - u1))
                * torch.cos(2.0 * math.pi * u2))

    z = z_of(0)
    unsure = torch.zeros(n, dim, dtype=torch.bool)
    if truncated > 0.1:
        unsure |= (z - truncated).abs() < near
        for attempt in range(1, 16):
            bad = z > truncated
            if not bool(bad.any()):
                break
            z = torch.where(bad, z_of(attempt), z)
            if attempt < 15:   # the 16th sample is taken as it comes
                unsure |= bad & ((z - truncated).abs() < near)
    return mean + stddev * z, unsure
