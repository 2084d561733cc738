"""Cone-aligned vector estimation (CaVE) losses with the MI355X `solver='hip'` backend.

Host-side mirror of /root/reference src/cave.py: same class names, constructor
arguments, call convention ``module(pred_cost, tight_ctrs) -> loss`` and error
behaviour, for ONE backend.  The whole forward of the reference —
sign flip, projection under no_grad, target construction, cosine loss
(src/cave.py:55-73,121-129,197-219) — and its autograd backward are one fused
HIP kernel launch (cave_amd/csrc/cave_hip.hip) behind a
``torch.autograd.Function``; ``reduction`` stays in torch.

Constructor signatures are the reference's (src/cave.py:93-100,152-163), including the
default ``solver='clarabel'``; ``'hip'`` is the one name added to the accepted set (src/cave.py:111).
The reference's own backends ('clarabel', 'nnls', 'apgd') are not shipped in this package and
there is no CPU fallback: asking for one raises ImportError, the way the reference refuses
``solver='clarabel'`` without cvxpy (src/cave.py:113-117).
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .abcmodule import EPO, optModule, sense_sign
from .dataset import PackedBatch
from .qpsolver import (PreparedCones, _step_qualifies, cone_op_dense, cone_op_prepared, cone_op_sparse, prepare_cones,
                       prepare_dense, prepare_sparse)
from .sparse import SparseCones
from .warm import DEFAULT_ENTRIES, WarmCache

__all__ = ["exactConeAlignedCosine", "innerConeAlignedCosine", "abstractConeAlignedCosine", "EPO", "flush_checks"]

_REFERENCE_SOLVERS = ("apgd", "clarabel", "nnls")


def _dense_shape_settled(tight_ctrs) -> bool:
    from . import qpsolver

    return (int(tight_ctrs.shape[1]), int(tight_ctrs.shape[2])) in qpsolver._settled


def _packed_kwargs(kwargs: dict) -> dict:
    """Launch limits (nnz_cap, lds_bytes) only apply to the dense scan; the store knows its own."""
    return {k: v for k, v in kwargs.items() if k in ("max_iter", "check")}


_APGD_KEYS = ("max_iters", "tol_grad", "check_frequency", "power_iter")  # the reference's names (src/qpsolver.py:11-18)


def _op_kwargs(kwargs: dict) -> dict:
    """solver_kwargs minus the keys the loss modules consume themselves ('inner': the kind of interior point,
    'warm_start': the multiplier cache; on the APGD arm of innerConeAlignedCosine -- '_apgd', set by its
    _solver_kwargs_for_call -- also the projector's own keys, which no other entry takes)."""
    drop = ("inner", "warm_start", "_apgd") + (_APGD_KEYS if kwargs.get("_apgd") else ())
    return {k: v for k, v in kwargs.items() if k not in drop}


def _apgd_op(tight_ctrs, pred_cost, mode, sign, kwargs: dict, check: bool, outputs):
    """The inner='apgd' arm: the reference's chunked APGD loop on the device (qpsolver._apgd_chunks) for a dense tensor or
    a SparseCones; a PreparedCones is unwrapped to the batch it keeps.  A store cannot serve: it holds reduced cones."""
    from .qpsolver import _apgd_chunks

    if isinstance(tight_ctrs, PackedBatch):
        raise ValueError("solver_kwargs['inner'] = 'apgd' iterates on the rows of the wire format as they are; a PackedBatch's "
                         "store holds reduced cones (pairs merged, unit rows eliminated). Pass the dense tensor or a SparseCones.")
    if isinstance(tight_ctrs, PreparedCones):
        tight_ctrs = tight_ctrs.ctrs
    out, _, _ = _apgd_chunks(tight_ctrs, pred_cost, mode, sign, kwargs.get("max_iters", 200), kwargs.get("tol_grad"),
                             kwargs.get("check_frequency", 200), kwargs.get("power_iter", 8), check, outputs)
    return out


_WARM_MODES = (_lib.MODE_PROJECT, _lib.MODE_EXACT, _lib.MODE_INNER)  # (HEURISTIC / AVG solve nothing; IPM runs cold)


def _warm_dense_ok(t, kwargs: dict) -> bool:
    """A plain dense batch the warm route may take: a shape of the fused step, launch limits not pinned by the caller
    (cone_op_dense honours pinned waves / nnz_cap / lds_bytes; the split form of the step has none)."""
    return not any(kwargs.get(k) for k in ("waves", "nnz_cap", "lds_bytes")) and _step_qualifies(t)


def _warm_entries(opt) -> int:
    """Table size for solver_kwargs['warm_start']: True = the default, an int = a capacity in distinct cones (the table
    holds twice as many entries).  Anything else is refused."""
    if opt is True:
        return DEFAULT_ENTRIES
    if isinstance(opt, int) and not isinstance(opt, bool) and opt > 0:
        return 2 * opt
    raise ValueError(f"Invalid solver_kwargs['warm_start'] {opt!r}. It should be True or a positive number of cones.")


# ---- deferred status checks (solver_kwargs={"check": "lazy"})
# Reading the per-instance status back right after the launch costs a host sync per step, which exposes the launch
# latency of everything else in an eager training step.  In lazy mode the status is copied to pinned memory
# asynchronously and examined by a LATER loss call, once its copy has arrived (or by flush_checks()), so a failing
# instance still raises -- a call or two later.  A later call never WAITS for a verdict (round 3 did, at the next call:
# the host could then not run ahead of the GPU by more than one step, 0.45 ms per step against 0.31 unchecked); only when
# more than LAZY_MAX_PENDING verdicts are outstanding does it wait for the oldest.
_pending_checks: list = []
LAZY_MAX_PENDING = 4


def _examine(host, what, shape, prepared=False) -> None:
    from . import _lib as L
    from . import qpsolver
    from .qpsolver import HipSolverError, _raise_for_status, forget_shape

    _pinned_free.setdefault(host.numel(), []).append(host)  # pinned allocations are slow: keep them
    if not bool(host.any()):  # every status CAVE_ST_OK (= 0): the common case costs one reduction on the host
        return
    too_large = bool((host == L.ST_TOO_LARGE).any())
    if shape is not None and too_large:
        forget_shape(*shape)
        if prepared:
            # the verdict of a step-kernel launch (a PreparedCones: prepare_dense / prefetch): the batch held a cone the
            # one-wave solver does not take.  forget_shape alone would leave the shape qualifying, and every later
            # batch with such a cone would fail the same way: prepare_dense now returns the tensor for this shape and
            # the next call, status-checked, settles a tier of the general path
            qpsolver._step_ok[(int(shape[0]), int(shape[1]))] = False
            bad = int((host == L.ST_TOO_LARGE).sum())
            first = int((host == L.ST_TOO_LARGE).nonzero()[0])
            raise HipSolverError(
                f"{what}: {bad} cone(s) (first index {first}) are not ones the one-wave solver of the fused step takes "
                "(more than 32 reduced rows, 8 bound rows, 8 entries per column or 1536 non-zeros, entries other than "
                "+-1, or no room for the active-set scratch); those instances contributed zero loss and zero gradient. "
                "Later batches of this shape take the general path.")
    _raise_for_status(host, what, sparse="sparse cones" in what)


def flush_checks() -> None:
    """Examine the status of every lazily checked launch so far (waits for them); raises like the strict check would.

    A launch whose cached shape (waves / LDS tier per (m_max, d)) turned out too small for a later batch
    forgets that shape first, so the next call for it runs status-checked and re-tiers (two waves, full
    arena, large-cone path) instead of failing again.  The failed instances of the lazy launch itself
    contributed zero loss and zero gradient (masked on the device), so no NaN reached the optimizer."""
    while _pending_checks:
        host, event, what, shape, prepared = _pending_checks.pop(0)
        event.synchronize()
        _examine(host, what, shape, prepared)


def _poll_checks() -> None:
    """The verdicts that have arrived, without waiting (beyond LAZY_MAX_PENDING outstanding: the oldest is awaited)."""
    while _pending_checks and (_pending_checks[0][1].query() or len(_pending_checks) > LAZY_MAX_PENDING):
        host, event, what, shape, prepared = _pending_checks.pop(0)
        event.synchronize()
        _examine(host, what, shape, prepared)


_pinned_free: dict = {}


def _defer_check(status: torch.Tensor, what: str, shape=None, prepared: bool = False) -> None:
    free = _pinned_free.get(status.numel())
    host = free.pop() if free else torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
    host.copy_(status, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    _pending_checks.append((host, event, what, shape, prepared))


class _ConeLossFunction(torch.autograd.Function):
    """loss_b = 1 - cos(sign*pred_b, target_b), target constant (src/cave.py:68-72) — fused fwd+bwd."""

    @staticmethod
    def forward(ctx, pred_cost, tight_ctrs, mode, sign, inner_ratio, kwargs):
        if kwargs.get("_apgd") and mode == _lib.MODE_EXACT:
            return _ConeLossFunction._forward_apgd(ctx, pred_cost, tight_ctrs, mode, sign, kwargs)
        warm = kwargs.get("warm_start")  # (a WarmCache: solver_kwargs={"warm_start": ...}, see _solver_kwargs_for_call)
        warm = warm if isinstance(warm, WarmCache) else None
        kwargs = _op_kwargs(kwargs)
        lazy = kwargs.get("check") == "lazy"
        if lazy:
            _poll_checks()  # the verdicts of earlier calls that have arrived
            kwargs = dict(kwargs, check=False)
        if isinstance(tight_ctrs, PreparedCones):
            from . import qpsolver

            if qpsolver._step_ok.get(tight_ctrs.shape[1:]) is False:
                # prepared before a verdict said that this shape holds cones the step kernel does not take (_examine):
                # the batch it keeps (tensor or SparseCones) goes down the general path, status-checked until a tier has settled
                tight_ctrs = tight_ctrs.ctrs
        if warm is not None and mode not in _WARM_MODES:
            warm = None
        if warm is not None and isinstance(tight_ctrs, SparseCones):
            # warm start on a plain sparse batch: the split form of the fused step (pack-only launch, then the warm solve);
            # a shape the step does not take runs cold on today's route
            if _step_qualifies(tight_ctrs) and tight_ctrs.device == warm.device:
                tight_ctrs = prepare_sparse(tight_ctrs)
            else:
                warm = None
        if warm is not None and not isinstance(tight_ctrs, (PackedBatch, PreparedCones)) and _warm_dense_ok(tight_ctrs, kwargs) \
                and tight_ctrs.device == warm.device:
            # warm start on a plain dense batch: the split form of the fused step (pack-only launch, then solve)
            if lazy and not _dense_shape_settled(tight_ctrs):
                kwargs = dict(kwargs, check=True)  # first call for this shape: strict, as below
                lazy = False
            tight_ctrs = prepare_dense(tight_ctrs)
        if isinstance(tight_ctrs, PackedBatch):  # device-resident cones, ids only (cave_amd/dataset.py)
            o = tight_ctrs.store.cone_op(tight_ctrs.ids, pred_cost, mode, sign, inner_ratio, zero_failed=lazy,
                                         outputs=("loss", "grad"), **_packed_kwargs(kwargs))
        elif isinstance(tight_ctrs, PreparedCones):  # dense batch whose pack stage ran ahead (qpsolver.prepare_dense)
            w = warm if warm is not None and tight_ctrs.device == warm.device else None
            o = cone_op_prepared(tight_ctrs, pred_cost, mode, sign, inner_ratio, zero_failed=lazy, outputs=("loss", "grad"),
                                 warm=w, **_packed_kwargs(kwargs))
            if w is not None and kwargs.get("check", True) is True:
                from . import qpsolver

                qpsolver._settled.add(tight_ctrs.shape[1:])  # a clean strict call: later lazy calls may run unchecked
        elif isinstance(tight_ctrs, SparseCones):  # sparse wire format (cave_amd/sparse.py): no dense tensor anywhere
            o = cone_op_sparse(tight_ctrs, pred_cost, mode, sign, inner_ratio, outputs=("loss", "grad"), **_packed_kwargs(kwargs))
        else:
            if lazy and not _dense_shape_settled(tight_ctrs):
                kwargs = dict(kwargs, check=True)  # first call for this shape: strict, so the launch tier can settle
                lazy = False
            o = cone_op_dense(tight_ctrs, pred_cost, mode, sign, inner_ratio, outputs=("loss", "grad"), **kwargs)
        if warm is not None:  # diagnostics of the most recent call (device tensors): what served it, in how many iterations
            warm.last_iters, warm.last_status, warm.last_hit = o["iters"], o["status"], o.get("warm_hit")
        loss, grad = o["loss"], o["grad"]
        if lazy:
            if isinstance(tight_ctrs, SparseCones):
                _defer_check(o["status"], "solver='hip' (lazy check, sparse cones)", (tight_ctrs.m_max, tight_ctrs.d))
            elif isinstance(tight_ctrs, PreparedCones) and tight_ctrs.sparse:
                _defer_check(o["status"], "solver='hip' (lazy check, sparse cones)", tight_ctrs.shape[1:], prepared=True)
            else:
                shape = None if isinstance(tight_ctrs, PackedBatch) else (int(tight_ctrs.shape[1]), int(tight_ctrs.shape[2]))
                _defer_check(o["status"], "solver='hip' (lazy check)", shape, prepared=isinstance(tight_ctrs, PreparedCones))
            # the verdict arrives a call or two late: until then a failed instance (NaN-filled outputs) must not reach
            # the optimizer.  The step kernel zeroes its loss and gradient itself (CAVE_STEP_ZERO_FAILED); after the
            # other kernels it is masked here, on the device (no host sync either way)
            if not o.get("zero_failed"):
                ok = o["status"] == 0
                loss = torch.where(ok, loss, torch.zeros_like(loss))
                grad = torch.where(ok.unsqueeze(1), grad, torch.zeros_like(grad))
        ctx.save_for_backward(grad)
        ctx.pred_meta = (pred_cost.device, pred_cost.dtype)
        return loss.to(device=pred_cost.device, dtype=pred_cost.dtype)

    @staticmethod
    def _forward_apgd(ctx, pred_cost, tight_ctrs, mode, sign, kwargs):
        """inner='apgd': the target is the normalised truncated APGD iterate (src/cave.py:213-214 with solver='apgd');
        always cold.  `check`: True / False / 'lazy' as on the other routes (a dense shape whose entry capacity has not
        settled yet runs its first lazy call strict)."""
        from . import qpsolver

        check = kwargs.get("check", True)
        lazy = check == "lazy"
        if lazy:
            _poll_checks()
            cones = tight_ctrs.ctrs if isinstance(tight_ctrs, PreparedCones) else tight_ctrs
            if isinstance(cones, torch.Tensor) and (int(cones.shape[1]), int(cones.shape[2])) not in qpsolver._apgd_cap:
                lazy = False
        o = _apgd_op(tight_ctrs, pred_cost, mode, sign, kwargs, bool(check) and not lazy, ("loss", "grad"))
        loss, grad = o["loss"], o["grad"]
        if lazy:
            sparse = isinstance(tight_ctrs, SparseCones) or (isinstance(tight_ctrs, PreparedCones) and tight_ctrs.sparse)
            _defer_check(o["status"], "solver='hip' (lazy check, apgd" + (", sparse cones)" if sparse else ")"))
            ok = o["status"] == 0
            loss = torch.where(ok, loss, torch.zeros_like(loss))
            grad = torch.where(ok.unsqueeze(1), grad, torch.zeros_like(grad))
        ctx.save_for_backward(grad)
        ctx.pred_meta = (pred_cost.device, pred_cost.dtype)
        return loss.to(device=pred_cost.device, dtype=pred_cost.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        device, dtype = ctx.pred_meta
        g = grad * grad_out.to(device=grad.device, dtype=grad.dtype).unsqueeze(1)
        return g.to(device=device, dtype=dtype), None, None, None, None, None


class abstractConeAlignedCosine(optModule):
    """CaVE family base: loss = 1 - cos(sense-flipped prediction, cone projection target)."""

    def __init__(self, optmodel, processes: int = 1, reduction: str = "mean") -> None:
        super().__init__(optmodel, processes, solve_ratio=1.0, reduction=reduction)

    def _mode(self) -> int:
        raise NotImplementedError

    def forward(self, pred_cost: torch.Tensor, tight_ctrs: torch.Tensor) -> torch.Tensor:
        """`tight_ctrs`: the reference's dense (B, m_max, d) tensor, a PackedBatch (store + ids), a PreparedCones, or a
        cave_amd.sparse.SparseCones (the sparse wire format: same loss and gradient as the dense tensor it stands for;
        ``check`` as for a PackedBatch; under ``solver_kwargs["warm_start"]`` a batch of a shape the fused step takes is
        packed by a launch of its own and solved warm, like a plain dense batch)."""
        sign = sense_sign(self.optmodel.modelSense)  # ValueError on a bad sense, src/cave.py:62-67
        kwargs = self._solver_kwargs_for_call()
        mode = self._mode()
        if kwargs.get("warm_start") and not kwargs.get("_apgd"):  # (the APGD arm runs cold: no cache is made for it)
            kwargs = dict(kwargs, warm_start=self._warm_cache(tight_ctrs, mode, kwargs))
        loss = _ConeLossFunction.apply(pred_cost, tight_ctrs, mode, sign, self._inner_ratio(), kwargs)
        return self._reduce(loss)

    def _warm_cache(self, tight_ctrs, mode: int, kwargs: dict) -> "WarmCache | None":
        """The module's multiplier cache (solver_kwargs={"warm_start": ...}) when this call can use it -- a projection
        mode on a prepared batch or a plain dense batch the fused step takes; None otherwise (a PackedBatch warm-starts
        through its store).  Created on the device of the first call that can use it."""
        if mode not in _WARM_MODES or isinstance(tight_ctrs, PackedBatch):
            return None
        if isinstance(tight_ctrs, SparseCones):
            if not _step_qualifies(tight_ctrs):
                return None
        elif not isinstance(tight_ctrs, PreparedCones) and not (isinstance(tight_ctrs, torch.Tensor) and
                                                                _warm_dense_ok(tight_ctrs, _op_kwargs(kwargs))):
            return None
        cache = getattr(self, "_warm", None)
        if cache is None:
            cache = self._warm = WarmCache(_warm_entries(self.solver_kwargs["warm_start"]), tight_ctrs.device)
        return cache if cache.device == tight_ctrs.device else None

    def reset_warm_start(self) -> None:
        """Forget every cached multiplier (the next solves start cold)."""
        cache = getattr(self, "_warm", None)
        if cache is not None:
            cache.reset()

    def _inner_ratio(self) -> float:
        return 0.0

    @staticmethod
    def prepare(tight_ctrs, following=None):
        """Run the prediction-independent half of the forward pass (streaming the dense cones and building the
        reduced cones) for a batch now; pass the result in place of `tight_ctrs`: `loss_fn(cp, prep)`.  Both arguments
        may be dense tensors or SparseCones (on the device), in any combination.  With
        `following` (the cones of the batch after it -- the DataLoader has collated them already) that batch's
        half rides in the launch of this batch's loss call, beside its solve, and `prep.next` is what to pass for it:

            prep = loss_fn.prepare(bctr_0, bctr_1)
            loss = loss_fn(cp_0, prep); nxt = prep.next.then(bctr_2); loss = loss_fn(cp_1, nxt); ...

        (`cave_amd.dataset.prefetch(loader)` does this wiring around a DataLoader.)  Returns the tensor itself when
        the shape does not qualify."""
        prep = prepare_cones(tight_ctrs)
        if following is not None and isinstance(prep, PreparedCones):
            prep.then(following)
        return prep

    def _solver_kwargs_for_call(self) -> dict:
        return self.solver_kwargs

    def _get_projection(self, signed_cost: torch.Tensor, tight_ctrs: torch.Tensor) -> torch.Tensor:
        """The constant target for an already sense-flipped cost (src/cave.py:121-129,197-219)."""
        if isinstance(tight_ctrs, PreparedCones):
            tight_ctrs = tight_ctrs.ctrs  # the batch it was prepared from (the target needs no fused step)
        kw = self._solver_kwargs_for_call()
        mode = self._mode()
        if kw.get("_apgd") and mode == _lib.MODE_EXACT:
            with torch.no_grad():
                o = _apgd_op(tight_ctrs, signed_cost, mode, 1.0, kw, kw.get("check", True) is True, ("target",))
            return o["target"].to(device=signed_cost.device, dtype=signed_cost.dtype)
        with torch.no_grad():
            if isinstance(tight_ctrs, PackedBatch):
                o = tight_ctrs.store.cone_op(tight_ctrs.ids, signed_cost, mode, 1.0, self._inner_ratio(),
                                             outputs=("target",), **_packed_kwargs(kw))
            elif isinstance(tight_ctrs, SparseCones):
                o = cone_op_sparse(tight_ctrs, signed_cost, mode, 1.0, self._inner_ratio(),
                                   outputs=("target",), **_packed_kwargs(kw))
            else:
                o = cone_op_dense(tight_ctrs, signed_cost, mode, 1.0, self._inner_ratio(),
                                  outputs=("target",), **_op_kwargs(kw))
        return o["target"].to(device=signed_cost.device, dtype=signed_cost.dtype)


class exactConeAlignedCosine(abstractConeAlignedCosine):
    """CaVE Exact: full projection onto the cone of binding-constraint normals (src/cave.py:84-129)."""

    def __init__(self, optmodel, solver: str = "clarabel", solver_kwargs: dict | None = None, processes: int = 1,
                 reduction: str = "mean") -> None:
        super().__init__(optmodel, processes, reduction)
        if solver not in ("hip",) + _REFERENCE_SOLVERS:
            raise ValueError(f"Invalid solver: {solver}. Must be 'apgd', 'clarabel', 'nnls' or 'hip'.")  # src/cave.py:111-112
        if solver != "hip":
            raise ImportError(f"solver='{solver}' is the reference's own backend and is not shipped with cave_amd "
                              "(no cvxpy/clarabel/SciPy path, no CPU fallback): pass solver='hip'.")  # cf. :113-117
        _lib.load()  # ImportError if the HIP extension or a device is missing (cf. src/cave.py:113-117)
        self.solver = solver
        self.solver_kwargs = dict(solver_kwargs or {})
        # warm start of the fused step (cave_amd/warm.py): True, or a capacity in distinct cones; False / absent: off
        if self.solver_kwargs.get("warm_start", False) is not False:
            _warm_entries(self.solver_kwargs["warm_start"])
        self._warm = None

    def _mode(self) -> int:
        return _lib.MODE_EXACT


class innerConeAlignedCosine(exactConeAlignedCosine):
    """CaVE+ / CaVE Hybrid (src/cave.py:132-219).

    Default (``solver_kwargs`` without ``'inner'``, or ``{'inner': 'push'}``): `solver='hip'` is an exact
    projector like 'nnls', so the interior point comes from the convex combination with the average normal
    (src/cave.py:216-219); ``max_iter`` is then ignored exactly as the nnls arm ignores it (src/cave.py:302).

    ``solver_kwargs={'inner': 'ipm'}``: the interior point is a truncated interior-point iterate, the way the
    reference's CaVE+ uses Clarabel with ``max_iter`` iterations (src/cave.py:213-214, 267-295): ``max_iter``
    path-following steps on the barrier problem (CAVE_MODE_INNER_IPM, include/cave_hip.h), every multiplier of
    the iterate strictly positive, the normalised iterate is the target and no average normal is mixed in.
    A restatement of the mechanism, not of Clarabel's iterates (no Clarabel in the image: parity unpinned).

    ``solver_kwargs={'inner': 'apgd'}``: the interior point is the truncated iterate of the reference's APGD projector
    (`project_apgd`, src/qpsolver.py:11-110, what the reference's CaVE+ runs under ``solver='apgd'``), restated on the
    device (cave_hip_cone_apgd, include/cave_hip.h) and pinned against the unmodified reference by fixtures.  The keys
    ``max_iters`` (default 200), ``tol_grad`` (default None), ``check_frequency`` and ``power_iter`` keep the reference's
    names; the constructor's ``max_iter`` is ignored on this arm, as in the reference.  Takes dense tensors and
    SparseCones (a PreparedCones is unwrapped); a PackedBatch raises ValueError (its store holds reduced cones);
    ``warm_start`` runs cold and makes no cache.  ``check=True`` (default) reads the status of the first chunk back, which
    is every chunk's; with ``tol_grad=None`` nothing else is read on the host, and ``check=False`` / ``'lazy'`` read nothing.
    The arm belongs to this class: exactConeAlignedCosine ignores ``'inner'``, as it always has.
    """

    _INNER_DEFAULTS: dict[str, dict] = {"hip": {}}

    def __init__(self, optmodel, solver: str = "clarabel", solver_kwargs: dict | None = None, max_iter: int = 3,
                 solve_ratio: float = 1.0, inner_ratio: float = 0.2, processes: int = 1, reduction: str = "mean",
                 seed: int | None = None) -> None:
        if solver_kwargs is None:
            solver_kwargs = dict(self._INNER_DEFAULTS.get(solver, {}))
        super().__init__(optmodel, solver, solver_kwargs, processes, reduction)
        if not 0 <= solve_ratio <= 1:
            raise ValueError(f"Invalid solve_ratio {solve_ratio}. It should be between 0 and 1.")
        if not 0 <= inner_ratio <= 1:
            raise ValueError(f"Invalid inner_ratio {inner_ratio}. It should be between 0 and 1.")
        self.inner = str(self.solver_kwargs.get("inner", "push"))
        if self.inner not in ("push", "ipm", "apgd"):
            raise ValueError(f"Invalid solver_kwargs['inner'] {self.inner!r}. It should be 'push', 'ipm' or 'apgd'.")
        self.max_iter = int(max_iter)
        self.solve_ratio = float(solve_ratio)
        self.inner_ratio = float(inner_ratio)
        if seed is not None:
            self._branch_rng = np.random.RandomState(seed)

    def _mode(self) -> int:
        # one draw per forward call decides QP vs heuristic for the whole batch (src/cave.py:201);
        # under data parallelism every rank must construct the module with the same seed
        if self._branch_rng.uniform() > self.solve_ratio:
            return _lib.MODE_HEURISTIC
        if self.inner == "apgd":  # the normalised APGD iterate is the target: the epilogue of MODE_EXACT (src/cave.py:213-214)
            return _lib.MODE_EXACT
        return _lib.MODE_INNER_IPM if self.inner == "ipm" else _lib.MODE_INNER

    def _solver_kwargs_for_call(self) -> dict:
        if self.inner == "ipm":  # max_iter is honoured: it is the number of interior-point steps
            return dict(self.solver_kwargs, max_iter=max(1, self.max_iter))
        if self.inner == "apgd":  # the class, not the key, chooses the arm: exactConeAlignedCosine ignores 'inner' as before
            return dict(self.solver_kwargs, _apgd=True)
        return self.solver_kwargs

    def _inner_ratio(self) -> float:
        return self.inner_ratio
