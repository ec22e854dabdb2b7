"""CPU: the CMUX and blind-rotation entry points are declared, exported, typed and bound, and the argument checks that need no module
return the documented error with nothing launched.  (Overlaps that are not equalities need the ring degree, hence a module, hence a
device: tests/test_gpu_cmux.py.)"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pz_glwe_cmux_batched", "pz_glwe_cmux_workspace_bytes", "pz_glwe_blind_rotation_batched", "pz_glwe_blind_rotation_tmp_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from poulpy_amd.hal import load_library
    return load_library()


def _params(**kw):
    from poulpy_amd.hal import GlweOpParams
    d = dict(rank=1, dnum=3, dsize=1, key_size=3, key_base2k=12, a_size=3, a_base2k=12, res_size=3, res_base2k=12, rank_out=1)
    d.update(kw)
    return GlweOpParams(**d)


def test_header_declares_and_library_exports_the_entry_points(lib):
    from poulpy_amd import abi
    from poulpy_amd.hal import GlweOpParams
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poulpy_hip.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in abi.PROTOTYPES, s
    f = lib.pz_glwe_cmux_batched
    assert f.restype is C.c_int and len(f.argtypes) == 10
    assert f.argtypes[3] is C.c_size_t and f.argtypes[4] is C.c_int64 and f.argtypes[6] is C.c_size_t and f.argtypes[8] is C.POINTER(GlweOpParams)
    r = lib.pz_glwe_blind_rotation_batched
    assert r.restype is C.c_int and len(r.argtypes) == 11 and r.argtypes[5] is C.c_int and r.argtypes[6] is C.c_size_t and r.argtypes[7] is C.POINTER(GlweOpParams)
    for q, nargs in ((lib.pz_glwe_cmux_workspace_bytes, 3), (lib.pz_glwe_blind_rotation_tmp_bytes, 3)):
        assert q.restype is C.c_size_t and len(q.argtypes) == nargs
        assert q(None, C.byref(_params()), 4) == 0          # no module: nothing to size


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    """No module is passed: a call that got past its argument checks would fail with "null module" (PZ_ERR_INVALID) - the checks below must
    fire before that, with their own message; the alias check with its own code."""
    from poulpy_amd import abi
    f = lib.pz_glwe_cmux_batched
    res, t, fp, key = 0x10000, 0x20000, 0x30000, 0x40000      # never dereferenced

    def err():
        return lib.pz_last_error().decode()

    # t, f, res and the GGSW share one base2k (external_product/glwe.rs:213)
    for bad in (dict(a_base2k=13), dict(res_base2k=11), dict(key_base2k=14)):
        assert f(None, res, t, 3, 0, fp, 3, key, C.byref(_params(**bad)), 2) == abi.PZ_ERR_INVALID
        assert "one base2k" in err(), err()
    # the rotated source: res == f is an overlap, t_size must be f_size
    assert f(None, fp, None, 3, 5, fp, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_ALIAS
    assert "must not overlap f" in err(), err()
    assert f(None, res, None, 2, 5, fp, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID
    assert "t_size == f_size" in err(), err()
    # the assign forms need one layout for res and the operand it is
    assert f(None, t, t, 2, 0, fp, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "different layouts" in err()
    assert f(None, fp, t, 3, 0, fp, 2, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "different layouts" in err()
    # null arguments, empty shapes
    assert f(None, res, t, 3, 0, None, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null argument" in err()
    assert f(None, res, t, 3, 0, fp, 3, key, None, 2) == abi.PZ_ERR_INVALID and "null params" in err()
    assert f(None, res, t, 3, 0, fp, 0, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "empty shape" in err()
    # well-formed arguments get as far as the module
    assert f(None, res, t, 3, 0, fp, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null module" in err()

    r = lib.pz_glwe_blind_rotation_batched
    bits = (C.c_void_p * 2)(key, 0)
    assert r(None, res, t, 2, bits, 1, 0, C.byref(_params()), 0x50000, 1 << 20, 2) == abi.PZ_ERR_INVALID and "GGSW 1 is null" in err()
    bits = (C.c_void_p * 2)(key, key)
    assert r(None, res, t, 2, bits, 1, 0, C.byref(_params(res_base2k=13)), 0x50000, 1 << 20, 2) == abi.PZ_ERR_INVALID and "one base2k" in err()
    assert r(None, res, res, 2, bits, 1, 0, C.byref(_params(a_size=2)), 0x50000, 1 << 20, 2) == abi.PZ_ERR_INVALID and "different layouts" in err()
    assert r(None, res, t, 2, bits, 1, 0, C.byref(_params()), 0x50000, 1 << 20, 2) == abi.PZ_ERR_INVALID and "null module" in err()


def test_bindings_exist_in_every_language():
    from poulpy_amd import bdd
    from poulpy_amd.hal import Module
    for m in ("glwe_cmux_batched", "glwe_cmux_workspace_bytes", "glwe_blind_rotation_batched", "glwe_blind_rotation_tmp_bytes"):
        assert callable(getattr(Module, m)), m
    assert callable(bdd.glwe_blind_selection)
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")).read()
    for s in ("pz_glwe_cmux_batched", "pz_glwe_blind_rotation_batched"):
        assert s + "(m_," in mirror, s
        assert "ffi::" + s + "(" in rust, s


class _Recorder:
    """stands in for a Module: records the CMUX calls the blind-selection helper issues"""
    def __init__(self, n):
        self._n, self.calls = n, []

    def n(self):
        return self._n

    def glwe_cmux_batched(self, res, t, f, key, params, batch, *, t_size, f_size, t_rot=0):
        self.calls.append((res.value, t.value, f.value, key, t_size, f_size, batch))


def test_blind_selection_issues_one_call_per_level_over_the_last_slots():
    from poulpy_amd import bdd
    n, batch, size = 1024, 2, 3
    slot = batch * n * 2 * size * 8
    rec = _Recorder(n)
    out = bdd.glwe_blind_selection(rec, 0x1000000, ["B0", "B1", "B2"], _params(), batch)
    base = 0x1000000
    assert rec.calls == [
        (base + 4 * slot, base + 4 * slot, base, "B2", size, size, 4 * batch),               # t = 4: slots 4..7 against 0..3, the MSB first
        (base + 6 * slot, base + 6 * slot, base + 4 * slot, "B1", size, size, 2 * batch),    # t = 2: slots 6..7 against 4..5
        (base + 7 * slot, base + 7 * slot, base + 6 * slot, "B0", size, size, batch),        # t = 1: slot 7 against 6
    ]
    assert out.value == base + 7 * slot
