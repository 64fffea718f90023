"""Independent emulation of the admission filter (count-min sketch and the
admit decision), written from the feature's specification and not from the
package: only ``core.rng.splitmix64`` is shared. Used by test_admission.py
(CPU) and test_gpu_admission.py.

Specification: the sketch is D rows of W int32 counters, W a power of two;
the cell of key k in row j is
``j*W + (splitmix64(splitmix64(k) ^ (seed + j)) & (W-1))`` in wrap-around
int64 arithmetic. One call sees unique keys; each key without a row adds 1
to its D cells, and after ALL adds of the call its estimate is the minimum of
its cells. ``estimate >= min_count`` gives it a row, in key order.
"""

import functools

import numpy as np
import torch

from openembedding_amd.core.rng import splitmix64


def cells(keys: torch.Tensor, W: int, D: int, seed: int) -> np.ndarray:
    """int64 [D, n] flat cell indices."""
    hk = splitmix64(keys.to(torch.int64))
    out = np.empty((D, keys.numel()), dtype=np.int64)
    for j in range(D):
        s = torch.tensor(seed, dtype=torch.int64) + j     # wraps like int64
        out[j] = j * W + (splitmix64(hk ^ s) & (W - 1)).numpy()
    return out


class RefAdmission:
    """Table (a dict key -> slot in admission order) + sketch + counters."""

    def __init__(self, W: int, D: int, seed: int, min_count: int,
                 row_cap: int = None):
        self.W, self.D, self.seed, self.min_count = W, D, seed, min_count
        self.sketch = np.zeros(D * W, dtype=np.int32)
        self.index = {}
        self.admitted = 0
        self.turned_away = 0
        self.row_cap = row_cap
        self.dropped = set()   # keys that overflowed the slab: miss forever

    def call(self, keys: torch.Tensor, live: int = None):
        """One training pull of unique ``keys`` (key -1 and the entries at
        and beyond ``live`` are defined misses that count nothing).
        Returns (slots int64 [n], new_mask uint8 [n])."""
        n = keys.numel()
        live = n if live is None else live
        kl = keys.tolist()
        slots = np.full(n, -1, dtype=np.int64)
        new = np.zeros(n, dtype=np.uint8)
        miss = []
        for i in range(live):
            k = kl[i]
            if k == -1 or k in self.dropped:
                continue
            s = self.index.get(k)
            if s is None:
                miss.append(i)
            else:
                slots[i] = s
        if miss:
            c = cells(keys[miss], self.W, self.D, self.seed)
            np.add.at(self.sketch, c.reshape(-1), 1)
            est = self.sketch[c].min(axis=0)
            for i, e in zip(miss, est.tolist()):
                if e >= self.min_count:
                    if self.row_cap is not None and \
                            len(self.index) + len(self.dropped) >= self.row_cap:
                        self.dropped.add(kl[i])
                        self.turned_away += 1
                        continue
                    slots[i] = len(self.index)
                    self.index[kl[i]] = slots[i]
                    new[i] = 1
                    self.admitted += 1
                else:
                    self.turned_away += 1
        return torch.from_numpy(slots), torch.from_numpy(new)

    def keys(self) -> torch.Tensor:
        return torch.tensor(sorted(self.index), dtype=torch.int64)

    def age(self, shift: int) -> None:
        self.sketch = (np.zeros_like(self.sketch) if shift >= 31
                       else self.sketch >> shift)


# ---------------------------------------------------------- reference stream

POOL = 3000
PULLS = 12
PER_PULL = 700
STREAM_D = 4
STREAM_SEED = 7
STREAM_MIN_COUNT = 3


@functools.lru_cache(maxsize=None)
def reference_stream():
    """12 pulls of 700 distinct keys out of a pool of 3000, drawn with
    probability ~ 1/(i+1). Returns a tuple of int64 tensors."""
    pool = (torch.arange(POOL, dtype=torch.int64) * 2654435761) % 2**40 + 1
    g = torch.Generator().manual_seed(1234)
    p = 1.0 / (torch.arange(POOL, dtype=torch.float64) + 1)
    return tuple(pool[torch.multinomial(p, PER_PULL, replacement=False,
                                        generator=g)]
                 for _ in range(PULLS))


@functools.lru_cache(maxsize=None)
def exact_counts():
    """key -> number of pulls of the reference stream that contain it."""
    cnt = {}
    for ks in reference_stream():
        for k in ks.tolist():
            cnt[k] = cnt.get(k, 0) + 1
    return cnt


@functools.lru_cache(maxsize=None)
def stream_result(W: int):
    """The emulation after the reference stream at width W (read-only)."""
    ref = RefAdmission(W, STREAM_D, STREAM_SEED, STREAM_MIN_COUNT)
    for ks in reference_stream():
        ref.call(ks)
    return ref
