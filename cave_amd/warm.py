"""Multiplier cache of the warm fused step (struct cave_warm_cache, include/cave_hip.h).

Cones are static per instance (src/dataset.py:72) and predictions drift slowly during training, so the multipliers
a solve of a cone ended with are a good starting point for the next solve of the same cone: TSP-20 needs ~2.6 Newton
iterations per step instead of ~5.2.  The cache lives on the device: a set-associative table (four ways per set) of
one 64-bit key and 32 float multipliers per entry, read and written by the solve half of the step kernel
(cave_hip_cone_step_warm).  Dense batches are keyed by the content of the cone, so they need no instance ids
and may be shuffled; a device-resident ConeStore keys by store slot.  Cached multipliers are only a starting point:
the results equal those of a cold start to the solver's tolerance whatever the cache holds.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib

__all__ = ["WarmCache", "DEFAULT_ENTRIES"]

DEFAULT_ENTRIES = 1 << 16  # 65 536 entries: 8.9 MB
THETA_PER_ENTRY = 32       # multipliers per entry (the one-wave solver takes up to 32 reduced rows)


def _pow2_at_least(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


class WarmCache:
    """Device memory of one multiplier cache: `key` [n] uint64 (as int64; 0 = empty) and `theta` [n, 32] float32.
    `entries` is rounded up to a power of two.  `reset()` empties it (the next solves start cold)."""

    def __init__(self, entries: int = DEFAULT_ENTRIES, device=None):
        if int(entries) <= 0:
            raise ValueError(f"WarmCache: entries must be positive, got {entries}")
        n = _pow2_at_least(int(entries))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.n = n
        self.key = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.theta = torch.zeros(n * THETA_PER_ENTRY, dtype=torch.float32, device=self.device)
        self.c = _lib.WarmCacheC(n_entries=n, key=self.key.data_ptr(), theta=self.theta.data_ptr())
        self.ref = C.byref(self.c)
        # a loss module's most recent call (device tensors; None before it): Newton iterations, status, and which
        # instances started from cached multipliers (None when a cold fallback served the batch)
        self.last_iters = self.last_status = self.last_hit = None

    @classmethod
    def for_capacity(cls, cones: int, device=None) -> "WarmCache":
        """A cache for `cones` distinct cones: twice as many entries, so that four-way sets rarely evict."""
        return cls(2 * int(cones), device)

    def reset(self) -> None:
        self.key.zero_()

    @property
    def nbytes(self) -> int:
        return self.key.numel() * self.key.element_size() + self.theta.numel() * self.theta.element_size()
