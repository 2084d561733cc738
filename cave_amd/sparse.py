"""Sparse wire format for cones: a batch in coordinate form, from the host to the pack kernels without a dense tensor.

The reference hands cones around as a zero-padded dense (B, m_max, d) float32 tensor (`collate_fn`,
src/dataset.py:133-144), although they come out of a sparse constraint matrix (src/dataset.py:167-169) and are almost
all zeros: a TSP-100 instance is 33 447 non-zeros in a 102 MB block.  `SparseCones` keeps, per batch,

    ent_off [B+1] int64    entry offsets of the instances
    key     [Z]   int32    (row << 16) | col as an unsigned 32-bit word, strictly increasing within an instance
    val     [Z]   float32  non-zero

which is `struct cave_sparse_cones` of include/cave_hip.h: 8 bytes per non-zero, read by the pack kernels in one
coalesced pass (cave_hip_pack_count_sparse / _fill_sparse / _large_sparse).  The constructors canonicalise on the host
with numpy: entries sorted by (row, col), explicit zeros dropped, a repeated (row, col) is an error (the dense format
cannot express it, and summing silently would hide a dataset bug).  Non-finite values stay in: the device rejects them
(CAVE_ST_BAD_INPUT -> ValueError), so that a caller of the C ABI and a caller of this layer get the same answer.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

__all__ = ["SparseCones", "collate_sparse"]

MAX_DIM = 65535  # rows and columns of an instance (16 bits each in the key)


def _canonical(rows, cols, vals, m, d: int, what: str):
    """One instance -> (key uint32 sorted, val float32, m)."""
    rows = np.asarray(rows).astype(np.int64, copy=False).ravel()
    cols = np.asarray(cols).astype(np.int64, copy=False).ravel()
    vals = np.asarray(vals).astype(np.float32, copy=False).ravel()
    if not (rows.shape == cols.shape == vals.shape):
        raise ValueError(f"{what}: rows, cols and vals must have the same length")
    keep = vals != 0  # (NaN != 0: non-finite values stay, for the device to reject)
    if not bool(keep.all()):
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    top = int(rows.max()) + 1 if rows.size else 0
    m = top if m is None else int(m)
    if rows.size and (int(rows.min()) < 0 or top > m or int(cols.min()) < 0 or int(cols.max()) >= d):
        raise ValueError(f"{what}: entry outside the ({m}, {d}) block")
    if m > MAX_DIM:
        raise ValueError(f"{what}: more than {MAX_DIM} rows per instance are not supported")
    key = (rows << 16) | cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    if key.size > 1 and bool((key[1:] == key[:-1]).any()):
        i = int(np.nonzero(key[1:] == key[:-1])[0][0])
        raise ValueError(f"{what}: entry (row {int(key[i] >> 16)}, col {int(key[i] & 0xffff)}) appears more than once")
    return key.astype(np.uint32), np.ascontiguousarray(vals), m


class SparseCones:
    """A batch of B cones in coordinate form (see the module docstring); tensors on any device."""

    def __init__(self, m_max: int, d: int, ent_off: torch.Tensor, key: torch.Tensor, val: torch.Tensor):
        self.m_max, self.d = int(m_max), int(d)
        if not 0 < self.d <= MAX_DIM or not 0 <= self.m_max <= MAX_DIM:
            raise ValueError(f"SparseCones: need 0 < d <= {MAX_DIM} and 0 <= m_max <= {MAX_DIM}")
        if ent_off.dtype != torch.int64 or key.dtype != torch.int32 or val.dtype != torch.float32:
            raise TypeError("SparseCones: ent_off int64, key int32 (the bits of the unsigned key), val float32")
        if ent_off.dim() != 1 or ent_off.numel() < 1 or key.shape != val.shape or key.dim() != 1:
            raise ValueError("SparseCones: ent_off [B+1], key [Z], val [Z]")
        self.ent_off, self.key, self.val = ent_off.contiguous(), key.contiguous(), val.contiguous()
        self.B = int(ent_off.numel()) - 1

    # ------------------------------------------------------------------ constructors
    @classmethod
    def _from_parts(cls, parts, d: int, m_max) -> "SparseCones":
        top = max((p[2] for p in parts), default=0)
        if m_max is None:
            m_max = top
        elif top > int(m_max):
            raise ValueError(f"SparseCones: an instance has {top} rows, m_max = {m_max}")
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        if parts:
            np.cumsum([p[0].size for p in parts], out=off[1:])
        key = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.uint32)
        val = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.float32)
        return cls(m_max, d, torch.from_numpy(off), torch.from_numpy(key.astype(np.uint32).view(np.int32)),
                   torch.from_numpy(val.astype(np.float32, copy=False)))

    @classmethod
    def from_coo(cls, items, d: int, m_max: int | None = None) -> "SparseCones":
        """`items`: one (rows, cols, vals[, m]) tuple per instance, entries in any order (what
        cave_amd.synth.coo_batch returns passes as is)."""
        parts = []
        for b, it in enumerate(items):
            m = it[3] if len(it) > 3 else None
            parts.append(_canonical(it[0], it[1], it[2], m, int(d), f"SparseCones.from_coo: instance {b}"))
        return cls._from_parts(parts, int(d), m_max)

    @classmethod
    def from_dense(cls, tensor) -> "SparseCones":
        """From the zero-padded (B, m_max, d) tensor of the reference's collate_fn (host copy; for tests, small data)."""
        a = tensor.detach().cpu().numpy() if isinstance(tensor, torch.Tensor) else np.asarray(tensor)
        if a.ndim != 3:
            raise ValueError("SparseCones.from_dense: need a (B, m_max, d) tensor")
        B, m, d = a.shape
        parts = []
        for b in range(B):
            r, c = np.nonzero(a[b])
            parts.append(_canonical(r, c, a[b][r, c], m, d, f"SparseCones.from_dense: instance {b}"))
        return cls._from_parts(parts, d, m)

    @classmethod
    def from_ragged(cls, ctrs, m_max: int | None = None) -> "SparseCones":
        """From `optDatasetConstrs.ctrs`: a list of (m_i, d) tensors / arrays or scipy.sparse matrices."""
        parts, d = [], None
        for b, a in enumerate(ctrs):
            what = f"SparseCones.from_ragged: instance {b}"
            if hasattr(a, "tocoo") and not isinstance(a, (np.ndarray, torch.Tensor)):  # scipy.sparse
                coo = a.tocoo()
                coo.sum_duplicates()
                mi, di = coo.shape
                r, c, v = coo.row, coo.col, coo.data
            else:
                x = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
                if x.ndim != 2:
                    raise ValueError(f"{what}: need an (m_i, d) matrix")
                mi, di = x.shape
                r, c = np.nonzero(x)
                v = x[r, c]
            if d is None:
                d = int(di)
            elif int(di) != d:
                raise ValueError(f"{what}: {di} columns, the instances before it have {d}")
            parts.append(_canonical(r, c, v, mi, d, what))
        if d is None:
            raise ValueError("SparseCones.from_ragged: no instances")
        return cls._from_parts(parts, d, m_max)

    @classmethod
    def from_uniform(cls, m_max: int, d: int, nnz: int, key: torch.Tensor, val: torch.Tensor) -> "SparseCones":
        """A batch whose instances all hold `nnz` entries, from canonical flat key / val tensors (what a device kernel
        writes: cave_amd.tight.sp_cones_hip); ent_off is made on their device, nothing is copied or checked."""
        nnz = int(nnz)
        if nnz <= 0 or key.numel() % nnz:
            raise ValueError("SparseCones.from_uniform: key must hold a whole number of instances")
        off = torch.arange(key.numel() // nnz + 1, dtype=torch.int64, device=key.device) * nnz
        return cls(m_max, d, off, key, val)

    @classmethod
    def cat(cls, pieces, m_max: int | None = None) -> "SparseCones":
        """Concatenate batches (offset arithmetic only)."""
        pieces = list(pieces)
        if not pieces:
            raise ValueError("SparseCones.cat: nothing to concatenate")
        d = pieces[0].d
        if any(p.d != d for p in pieces):
            raise ValueError("SparseCones.cat: pieces differ in d")
        top = max(p.m_max for p in pieces)
        m_max = top if m_max is None else int(m_max)
        if m_max < top:
            raise ValueError(f"SparseCones.cat: a piece has m_max = {top}, asked for {m_max}")
        offs, base = [pieces[0].ent_off[:1]], 0
        for p in pieces:
            offs.append(p.ent_off[1:] + base)
            base += int(p.ent_off[-1])
        return cls(m_max, d, torch.cat(offs), torch.cat([p.key for p in pieces]), torch.cat([p.val for p in pieces]))

    # ------------------------------------------------------------------ container
    def __len__(self) -> int:
        return self.B

    @property
    def device(self):
        return self.key.device

    @property
    def is_cuda(self) -> bool:
        return self.key.is_cuda

    @property
    def nnz(self) -> int:
        return int(self.key.numel())

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.ent_off, self.key, self.val))

    @property
    def nnz_per_instance(self) -> torch.Tensor:
        return self.ent_off[1:] - self.ent_off[:-1]

    def to(self, device, non_blocking: bool = False) -> "SparseCones":
        device = torch.device(device)
        if device == self.key.device:
            return self
        return SparseCones(self.m_max, self.d, self.ent_off.to(device, non_blocking=non_blocking),
                           self.key.to(device, non_blocking=non_blocking), self.val.to(device, non_blocking=non_blocking))

    def cuda(self, device=None) -> "SparseCones":
        return self.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)

    def __getitem__(self, idx) -> "SparseCones":
        """An int (a batch of one), a slice, or a list / tensor of instance indices."""
        if isinstance(idx, slice):
            start, stop, step = idx.indices(self.B)
            if step == 1:
                stop = max(stop, start)
                off = self.ent_off[start:stop + 1]
                lo, hi = int(off[0]), int(off[-1])
                return SparseCones(self.m_max, self.d, off - lo, self.key[lo:hi], self.val[lo:hi])
            idx = list(range(start, stop, step))
        elif isinstance(idx, (int, np.integer)):
            idx = [int(idx)]
        ids = torch.as_tensor(idx, dtype=torch.int64).reshape(-1).cpu()
        if ids.numel() and (int(ids.min()) < -self.B or int(ids.max()) >= self.B):
            raise IndexError("SparseCones: instance index out of range")
        ids = torch.where(ids < 0, ids + self.B, ids)
        off = self.ent_off.cpu()
        cnt = off[ids + 1] - off[ids]
        new_off = torch.zeros(ids.numel() + 1, dtype=torch.int64)
        torch.cumsum(cnt, 0, out=new_off[1:])
        # entry e of output instance j comes from off[ids[j]] + (e - new_off[j])
        src = torch.repeat_interleave(off[ids] - new_off[:-1], cnt) + torch.arange(int(new_off[-1]), dtype=torch.int64)
        src = src.to(self.key.device)
        return SparseCones(self.m_max, self.d, new_off.to(self.key.device), self.key[src], self.val[src])

    def densify(self, device=None) -> torch.Tensor:
        """The zero-padded (B, m_max, d) float32 tensor of the dense wire format (tests, fallbacks)."""
        device = self.key.device if device is None else torch.device(device)
        out = torch.zeros(self.B, self.m_max, self.d, dtype=torch.float32, device=device)
        if self.nnz:
            key = self.key.to(device).to(torch.int64) & 0xffffffff
            inst = torch.repeat_interleave(torch.arange(self.B, device=device), self.nnz_per_instance.to(device))
            out.view(-1)[(inst * self.m_max + (key >> 16)) * self.d + (key & 0xffff)] = self.val.to(device)
        return out

    def c_struct(self) -> "_lib.SparseConesC":
        """struct cave_sparse_cones over this batch's device tensors (the batch must outlive the launch)."""
        if not self.is_cuda:
            raise ValueError("SparseCones: the kernels need the batch on the device (.to(device))")
        return _lib.SparseConesC(B=self.B, m_max=self.m_max, d=self.d, ent_off=self.ent_off.data_ptr(),
                                 key=self.key.data_ptr(), val=self.val.data_ptr())

    def c_ref(self):
        self._c = self.c_struct()
        return C.byref(self._c)


def collate_sparse(batch):
    """Drop-in for the reference `collate_fn` (src/dataset.py:133-144) when the dataset yields
    (x, c, w, z, cone) with `cone` a one-instance SparseCones: stacks the dense fields and concatenates the cones on the
    host into one SparseCones (offset arithmetic only, no padding)."""
    *fields, cones = zip(*batch)
    return (*(torch.stack(f, 0) for f in fields), SparseCones.cat(cones))
