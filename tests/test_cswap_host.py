"""CPU: the conditional-swap and blind-retrieval entry points are declared, exported, typed and bound, and the argument checks that need no
module return the documented error with nothing launched.  (Overlaps that need the ring degree, host pointers and everything that
launches need a module, hence a device: tests/test_gpu_cswap.py.)"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pz_glwe_cswap_batched", "pz_glwe_cswap_workspace_bytes", "pz_glwe_blind_retrieval_batched", "pz_glwe_blind_retrieval_workspace_bytes")


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
    f = lib.pz_glwe_cswap_batched
    assert f.restype is C.c_int and len(f.argtypes) == 8
    assert f.argtypes[2] is C.c_size_t and f.argtypes[4] is C.c_size_t and f.argtypes[6] is C.POINTER(GlweOpParams) and f.argtypes[7] is C.c_size_t
    r = lib.pz_glwe_blind_retrieval_batched
    assert r.restype is C.c_int and len(r.argtypes) == 8
    assert r.argtypes[2] is C.c_size_t and r.argtypes[3] is C.c_size_t and r.argtypes[5] is C.c_int and r.argtypes[6] is C.POINTER(GlweOpParams)
    q = lib.pz_glwe_cswap_workspace_bytes
    assert q.restype is C.c_size_t and len(q.argtypes) == 3
    assert q(None, C.byref(_params()), 4) == 0                 # no module: nothing to size
    q = lib.pz_glwe_blind_retrieval_workspace_bytes
    assert q.restype is C.c_size_t and len(q.argtypes) == 5
    assert q(None, C.byref(_params()), 5, 3, 4) == 0


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    """No module is passed: a call that got past its argument checks would fail with "null module" (PZ_ERR_INVALID) - the checks below must
    fire before that, with their own message; the alias check with its own code."""
    from poulpy_amd import abi
    f = lib.pz_glwe_cswap_batched
    a, b, key = 0x10000000, 0x20000000, 0x40000      # never dereferenced

    def err():
        return lib.pz_last_error().decode()

    # a, b and the GGSW share one base2k (eval.rs:427, external_product/glwe.rs:213)
    for bad in (dict(a_base2k=13), dict(res_base2k=11), dict(key_base2k=14)):
        assert f(None, a, 3, b, 3, key, C.byref(_params(**bad)), 2) == abi.PZ_ERR_INVALID
        assert "one base2k" in err(), err()
    # any overlap of a and b: the same buffer, and a partial overlap that the pointers alone show (two ciphertexts of 2 x 3 limbs are
    # at least 2 * 2 * 3 * 2 * 8 = 192 bytes at the smallest ring degree)
    assert f(None, a, 3, a, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_ALIAS and "overlap" in err()
    assert f(None, a, 3, a + 64, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_ALIAS and "overlap" in err()
    assert f(None, a + 64, 3, a, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_ALIAS and "overlap" in err()
    # the difference lives on max(a_size, b_size) limbs; a' keeps the layout of a
    assert f(None, a, 3, b, 4, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "max(a_size, b_size)" in err(), err()
    assert f(None, a, 2, b, 2, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "max(a_size, b_size)" in err(), err()
    assert f(None, a, 3, b, 4, key, C.byref(_params(a_size=4, res_size=4)), 2) == abi.PZ_ERR_INVALID and "p->res_size is a_size" in err(), err()
    assert f(None, a, 2, b, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "p->res_size is a_size" in err(), err()
    # null arguments, empty shapes
    assert f(None, None, 3, b, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null argument" in err()
    assert f(None, a, 3, None, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null argument" in err()
    assert f(None, a, 3, b, 3, None, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null argument" in err()
    assert f(None, a, 3, b, 3, key, None, 2) == abi.PZ_ERR_INVALID and "null params" in err()
    assert f(None, a, 3, b, 0, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "empty shape" in err()
    assert f(None, a, 3, b, 3, key, C.byref(_params(dsize=0)), 2) == abi.PZ_ERR_INVALID and "empty shape" in err()
    # well-formed arguments get as far as the module - with any dsize >= 1, and with unequal sizes
    assert f(None, a, 3, b, 3, key, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null module" in err()
    assert f(None, a, 3, b, 3, key, C.byref(_params(dsize=2)), 2) == abi.PZ_ERR_INVALID and "null module" in err()
    assert f(None, a, 3, b, 4, key, C.byref(_params(a_size=4)), 2) == abi.PZ_ERR_INVALID and "null module" in err()
    assert f(None, a, 4, b, 3, key, C.byref(_params(a_size=4, res_size=4)), 2) == abi.PZ_ERR_INVALID and "null module" in err()

    r = lib.pz_glwe_blind_retrieval_batched
    bits = (C.c_void_p * 3)(key, 0, key)
    assert r(None, a, 5, 3, bits, 0, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "GGSW 1 is null" in err(), err()
    bits = (C.c_void_p * 3)(key, key, key)
    assert r(None, a, 5, 3, bits, 0, C.byref(_params(res_base2k=13)), 2) == abi.PZ_ERR_INVALID and "one base2k" in err()
    assert r(None, a, 5, 3, bits, 1, C.byref(_params(a_size=2)), 2) == abi.PZ_ERR_INVALID and "one layout" in err()
    assert r(None, None, 5, 3, bits, 0, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null argument" in err()
    assert r(None, a, 5, 3, bits, 0, None, 2) == abi.PZ_ERR_INVALID and "null params" in err()
    assert r(None, a, 5, 3, bits, 0, C.byref(_params()), 2) == abi.PZ_ERR_INVALID and "null module" in err()
    # nothing to do: PZ_OK without a module
    assert r(None, a, 0, 3, bits, 0, C.byref(_params()), 2) == abi.PZ_OK
    assert r(None, a, 5, 0, None, 1, C.byref(_params()), 2) == abi.PZ_OK


def test_bindings_exist_in_every_language():
    from poulpy_amd import bdd
    from poulpy_amd.hal import Module
    for m in ("glwe_cswap_batched", "glwe_cswap_workspace_bytes", "glwe_blind_retrieval_batched", "glwe_blind_retrieval_workspace_bytes"):
        assert callable(getattr(Module, m)), m
    assert callable(bdd.glwe_blind_retrieval)
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")).read()
    ffi = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "ffi.rs")).read()
    for s in ("pz_glwe_cswap_batched", "pz_glwe_blind_retrieval_batched"):
        assert s + "(m_," in mirror, s
        assert "ffi::" + s + "(" in rust, s
    for s in NEW_SYMBOLS:
        assert "pub fn " + s + "(" in ffi, s


class _Recorder:
    """stands in for a Module: records the composite call the blind-retrieval helper issues"""
    def __init__(self):
        self.calls = []

    def glwe_blind_retrieval_batched(self, slots, nslots, bit_ptrs, reverse, params, batch):
        self.calls.append((slots, nslots, list(bit_ptrs), reverse, batch))


def test_blind_retrieval_helper_is_one_composite_call():
    from poulpy_amd import bdd
    rec = _Recorder()
    out = bdd.glwe_blind_retrieval(rec, 0x1000000, 5, ["B0", "B1", "B2"], _params(), 2)
    bdd.glwe_blind_retrieval(rec, 0x1000000, 5, ["B0", "B1", "B2"], _params(), 2, reverse=True)
    assert rec.calls == [(0x1000000, 5, ["B0", "B1", "B2"], False, 2), (0x1000000, 5, ["B0", "B1", "B2"], True, 2)]
    assert out.value == 0x1000000
