"""CPU tier: warm start of the fused step -- solver_kwargs={"warm_start": ...} validation, the multiplier-cache export
of the C ABI and its argument checks (rejected before any launch: no GPU needed)."""

import ctypes as C
import os
import re
from unittest.mock import Mock

import pytest

from cave_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from cave_amd.cave import EPO

    m = Mock()
    m.modelSense = EPO.MINIMIZE
    return m


def test_warm_start_option_validation(monkeypatch):
    from cave_amd.cave import _op_kwargs, exactConeAlignedCosine, innerConeAlignedCosine

    monkeypatch.setattr(_lib, "load", lambda: None)
    for bad in ("yes", 0, -3, 2.5, [1], None):
        with pytest.raises(ValueError):
            innerConeAlignedCosine(_model(), solver="hip", solver_kwargs={"warm_start": bad})
        with pytest.raises(ValueError):
            exactConeAlignedCosine(_model(), solver="hip", solver_kwargs={"warm_start": bad})
    for ok in (True, False, 1, 4096):
        m = innerConeAlignedCosine(_model(), solver="hip", solver_kwargs={"warm_start": ok})
        assert m.solver_kwargs["warm_start"] is ok and m._warm is None  # the cache is created by the first call
        m.reset_warm_start()  # (nothing to reset yet)
    # the key never reaches the operators
    assert _op_kwargs({"warm_start": True, "inner": "push", "max_iter": 7}) == {"max_iter": 7}


def test_warm_cache_sizes():
    from cave_amd.cave import _warm_entries
    from cave_amd.warm import DEFAULT_ENTRIES, _pow2_at_least

    assert DEFAULT_ENTRIES == 65536 and _warm_entries(True) == DEFAULT_ENTRIES and _warm_entries(1000) == 2000
    assert [_pow2_at_least(n) for n in (1, 2, 3, 4, 5, 2000, 65536)] == [1, 2, 4, 4, 8, 2048, 65536]
    assert DEFAULT_ENTRIES * (8 + 32 * 4) == 8912896  # ~8.9 MB


def test_warm_step_export_and_argument_checks():
    _lib.build()
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "cave_hip.h")).read()
    assert "cave_hip_cone_step_warm" in _lib.ABI_SYMBOLS and len(lib.cave_hip_cone_step_warm.argtypes) == 27
    assert int(re.search(r"#define CAVE_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 10 == lib.cave_hip_version()
    none7 = [None] * 7

    def call(warm):
        return lib.cave_hip_cone_step_warm(None, None, None, 4, 2, 1.0, 0.2, 0, 0, *none7, None, 0, 0, 190, None, None,
                                           warm, None, None, None, None)

    buf = (C.c_float * 64)()
    keys = (C.c_uint64 * 4)()
    th = C.addressof(buf)
    th = (th + 15) & ~15  # 16-byte aligned
    for n, key, theta, what in ((3, keys, th, b"power of two"), (0, keys, th, b"power of two"), (4, None, th, b"null"),
                                (4, keys, None, b"null"), (4, keys, th + 4, b"aligned")):
        w = _lib.WarmCacheC(n_entries=n, key=C.cast(key, C.c_void_p).value if key is not None else None, theta=theta)
        assert call(C.byref(w)) == -1, what
        assert what in lib.cave_hip_last_error(), (what, lib.cave_hip_last_error())
    # a good cache gets as far as the checks of cave_hip_cone_step (here: no cu_tickets); warm = NULL likewise
    w = _lib.WarmCacheC(n_entries=4, key=C.cast(keys, C.c_void_p).value, theta=th)
    assert call(C.byref(w)) == -1 and b"cu_tickets" in lib.cave_hip_last_error()
    assert call(None) == -1 and b"cu_tickets" in lib.cave_hip_last_error()
    assert lib.cave_hip_cone_step_warm(None, None, None, 0, 0, 1.0, 0.0, 0, 0, *none7, None, 0, 0, 190, None, None,
                                       None, None, None, None, None) == 0  # nothing to do
