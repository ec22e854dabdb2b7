"""CPU: the many-rotations entry point is declared, exported and bound, and poulpy_amd.ckks plans a rotation with the metadata of
poulpy-ckks src/leveled/default/rotate.rs:44-55.  (The workspace query reads the module's plan, and a module needs a device: its
monotonicity is checked in tests/test_gpu_rotations.py.)"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pz_glwe_automorphism_many_batched", "pz_glwe_automorphism_many_workspace_bytes", "pz_module_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from poulpy_amd.hal import load_library
    return load_library()


def test_header_declares_and_library_exports_the_entry_points(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poulpy_hip.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
    from poulpy_amd.hal import GlweOpParams
    f = lib.pz_glwe_automorphism_many_batched
    assert f.restype is C.c_int and len(f.argtypes) == 8 and f.argtypes[6] is C.POINTER(GlweOpParams)
    q = lib.pz_glwe_automorphism_many_workspace_bytes
    assert q.restype is C.c_size_t and len(q.argtypes) == 4
    # no module: nothing to size, and no call
    p = GlweOpParams(rank=1, dnum=3, dsize=1, key_size=3, key_base2k=12, a_size=3, a_base2k=12, res_size=3, res_base2k=12, rank_out=1)
    assert q(None, C.byref(p), 4, 4) == 0 and lib.pz_module_workspace_bytes(None) == 0
    g, k = (C.c_int64 * 1)(5), (C.c_void_p * 1)(0)
    assert f(None, None, None, 1, g, k, C.byref(p), 1) < 0 and lib.pz_last_error()


def test_module_binds_both_methods():
    from poulpy_amd.hal import Module
    for m in ("glwe_automorphism_many_batched", "glwe_automorphism_many_workspace_bytes", "workspace_bytes"):
        assert callable(getattr(Module, m)), m
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    assert "pz_glwe_automorphism_many_batched(m_," in mirror and "pz_glwe_automorphism_many_workspace_bytes(m_," in mirror


def test_plan_rotate_metadata_follows_the_reference():
    from poulpy_amd import ckks
    # rotate.rs:44-55: offset = offset_unary(dst, src); dst.meta = src.meta; log_budget -= offset
    src = ckks.Ct(base2k=12, size=4, log_delta=30, log_budget=18)            # effective_k 48 = max_k: nothing to drop
    dst = ckks.Ct(base2k=12, size=4, log_delta=0, log_budget=0)
    p = ckks.plan_rotate_into(dst, src)
    assert (p.offset, p.log_delta, p.log_budget) == (0, 30, 18)
    p.apply_meta(dst)
    assert (dst.log_delta, dst.log_budget) == (30, 18)
    # a smaller destination: the reference shifts the source left by the offset first and the budget pays for it
    small = [ckks.Ct(base2k=12, size=3, log_delta=0, log_budget=0) for _ in range(3)]
    p = ckks.plan_rotate_many(small, src)
    assert p.offset == ckks.offset_unary(small[0], src) == 12
    assert (p.log_delta, p.log_budget) == (30, 6) and p.name == "rotate_many"
    # a budget too small for the offset: CKKSCompositionError before anything is launched
    poor = ckks.Ct(base2k=12, size=4, log_delta=40, log_budget=8)
    with pytest.raises(ckks.CKKSError):
        ckks.plan_rotate_into(ckks.Ct(base2k=12, size=3, log_delta=0, log_budget=0), poor)
    # destinations of one call share a layout and the source's base
    with pytest.raises(ckks.CKKSError):
        ckks.plan_rotate_many([small[0], dst], src)
    with pytest.raises(ckks.CKKSError):
        ckks.plan_rotate_into(ckks.Ct(base2k=13, size=4, log_delta=0, log_budget=0), src)
    with pytest.raises(ckks.CKKSError):
        ckks.plan_rotate_many([], src)


class _Recorder:
    """stands in for a Module: records the device calls a plan issues"""
    def __init__(self):
        self.calls = []

    def glwe_combine_batched(self, res, cols, size, base2k, terms, normalize, batch):
        self.calls.append(("combine", res, cols, size, base2k, [(t["a"], t["a_size"], t["kind"], t["k"]) for t in terms], normalize, batch))

    def glwe_automorphism_many_batched(self, res, a, gals, keys, params, batch):
        self.calls.append(("rotate", res, a, list(gals), list(keys), batch))


def test_plan_launch_issues_one_call_and_shifts_first_when_the_reference_does():
    from poulpy_amd import ckks
    n = 8192
    src = ckks.Ct(base2k=12, size=4, log_delta=30, log_budget=18, data="SRC")
    same = [ckks.Ct(base2k=12, size=4, log_delta=0, log_budget=0, data="DST") for _ in range(2)]
    rec = _Recorder()
    ckks.plan_rotate_many(same, src).launch(rec, same, src, [5, 2 * n - 1], ["K0", "KCONJ"], "P", 7)
    assert rec.calls == [("rotate", "DST", "SRC", [5, 2 * n - 1], ["K0", "KCONJ"], 7)]
    assert all((d.log_delta, d.log_budget) == (30, 18) for d in same)
    small = [ckks.Ct(base2k=12, size=3, log_delta=0, log_budget=0, data="DST3")]
    rec = _Recorder()
    plan = ckks.plan_rotate_into(small[0], src)
    with pytest.raises(ckks.CKKSError):
        plan.launch(rec, small, src, [5], ["K0"], "P", 7)                       # an offset needs the temporary
    plan.launch(rec, small, src, [5], ["K0"], "P", 7, tmp="TMP")
    assert rec.calls == [("combine", "TMP", 2, 3, 12, [("SRC", 4, ckks.LSH, 12)], False, 7), ("rotate", "DST3", "TMP", [5], ["K0"], 7)]
    assert (small[0].log_delta, small[0].log_budget) == (30, 6)
