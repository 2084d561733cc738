"""Small +-1 cones of a given dense shape (m, d) for the row-scan tests (TEST INFRASTRUCTURE; numpy only, seeded):
tests/test_rowscan_emul.py and tests/test_gpu_rowscan.py draw the same instances."""

import numpy as np


def small_cone(rng, m, d, pad_middle=False):
    """[m, d] block of a cone the lite solver takes: [free rows, their negations, bound rows, unit rows], zero rows at
    the end (and, pad_middle, between the general and the unit rows).  Free rows carry every column of a random set,
    bound rows two entries, so no two general rows are equal or opposite."""
    blk = np.zeros((m, d), np.float32)
    r = 0
    nf = 0 if (d < 2 or m < 2) else int(min(rng.integers(1, 4), m // 2, max(1, d // 8)))
    free = []
    for i in range(nf):
        k = d if d < 8 else int(rng.integers(3, min(d, 70) + 1)) if i == 0 else 3 + i
        cols = rng.choice(d, size=k, replace=False)
        a = np.zeros(d, np.float32)
        a[cols] = rng.choice(np.array([-1.0, 1.0], np.float32), k)
        free.append(a)
    for a in free:
        blk[r] = a
        r += 1
    for a in free:
        blk[r] = -a
        r += 1
    nb = 0 if d < 3 else int(min(rng.integers(0, 3), m - r))
    for i in range(nb):
        cols = rng.choice(d, size=2, replace=False)
        if i == 1 and set(cols) == set(np.flatnonzero(blk[r - 1])):
            cols = (cols + 1) % d
        blk[r, cols] = rng.choice(np.array([-1.0, 1.0], np.float32), 2)
        r += 1
    if pad_middle and r + 3 <= m:
        r += 2
    room = m - r - (1 if m - r > 4 else 0)
    for k in rng.permutation(d)[:max(room, 0)]:
        blk[r, k] = 1.0 if rng.random() < 0.5 else -1.0
        r += 1
    return blk


def batch_of(seed, m, d, B=2):
    rng = np.random.default_rng([seed, m, d])
    return np.stack([small_cone(rng, m, d, pad_middle=(b == 1)) for b in range(B)])
