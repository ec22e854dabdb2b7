"""CPU: the plans of the products and weighted sums by constants (poulpy_amd/ckks.py) against the restatement of the reference's composites
(tests/ckks_lincomb_oracle.py) and against cases derived by hand from poulpy-ckks leveled/default/mul.rs:498-513, error.rs:177-194 and
leveled/delegates/composite.rs; the new entry point in the header, the library and every binding; and the kernel's per-coefficient walk
(poulpy_amd/csrc/device_lincomb.hpp, lc_walk) run on the host by a stand-alone program built with the host sanitizers, on the oracle's
digits.  (The device: tests/test_gpu_ckks_lincomb.py.)"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import Cst, Ct
from tests import ckks_lincomb_cases as cases
from tests import ckks_lincomb_oracle as lo
from tests.helpers import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, COLS = 16, 2


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


def _plan(sc, dst, ops):
    if sc["kind"] == "dot":
        return ckks.plan_dot_product_pt_const(dst, ops, sc["csts"])
    return ckks.plan_mul_add_pt_const(dst, ops[0], sc["csts"][0], sub=sc["kind"] == "sub")


def _oracle(ref, sc, dst, ops):
    if sc["kind"] == "dot":
        lo.ckks_dot_product_pt_const(ref, dst, ops, sc["csts"])
    else:
        lo.ckks_mul_add_pt_const(ref, dst, ops[0], sc["csts"][0], sub=sc["kind"] == "sub")


@pytest.mark.parametrize("B", [12, 19])
def test_plans_reproduce_the_oracle_metadata_and_digits(ref, B):
    """every scenario: the composite restated on the oracle's primitives, and the plan's own term list run on the same primitives - same
    digits, same metadata"""
    joins = set()
    for i, sc in enumerate(cases.scenarios(B)):
        host = cases.host_inputs(seeded(B * 100 + i), sc, N, COLS, 1)
        want, ops = cases.on_host(sc, host, 0, N, COLS)
        _oracle(ref, sc, want, ops)
        got, ops = cases.on_host(sc, host, 0, N, COLS)
        plan = _plan(sc, got, ops)
        lo.run_plan(ref, plan, got, ops, sc["csts"])
        assert (got.log_delta, got.log_budget) == (want.log_delta, want.log_budget), sc["label"]
        assert np.array_equal(got.data.data, want.data.data), sc["label"]
        joins |= {(t.join, t.k < B) for t in plan.terms[0 if plan.init_res else 1:]}
        assert all(t.k > 0 for t in plan.terms if t.join != ckks.PLAIN) and all(t.k == 0 for t in plan.terms if t.join == ckks.PLAIN)
    # every branch, each with a shift below base2k and one that spans more than a limb
    assert joins >= {(ckks.PLAIN, True), (ckks.LSH_TERM, True), (ckks.LSH_TERM, False), (ckks.LSH_ACC, True), (ckks.LSH_ACC, False)}


def test_scenarios_cover_what_they_claim():
    for B in (12, 19):
        S = cases.scenarios(B)
        offs = [t.cnv_offset for sc in S for t in _plan(sc, Ct(B, sc["dst"].size, sc["dst"].log_delta, sc["dst"].log_budget), sc["ops"]).terms]
        assert any(0 < o < B for o in offs) and any(o >= 2 * B for o in offs) and any(o == 0 for o in offs)
        assert {len(sc["ops"]) for sc in S if sc["kind"] == "dot"} == {1, 2, 5}
        forms = {(c.re is not None, c.im is not None) for sc in S for c in sc["csts"]}
        assert forms == {(True, False), (False, True), (True, True), (False, False)}
        assert any(int(d) < 0 for sc in S for c in sc["csts"] for arr in (c.re, c.im) if arr is not None for d in arr)
        assert any(sc["shared"] for sc in S) and {sc["wide"] for sc in S} == {False, True}
        assert any(sc["kind"] == "dot" and len(sc["ops"]) > 1 and all(c.im is None for c in sc["csts"]) for sc in S)   # the unpaired mapping


def test_get_mul_const_params_by_hand():
    """mul.rs:498-513: budget = a.log_budget - prec.log_delta; offset = (budget + a.log_delta) -| res.max_k; cnv = min_k(prec) + offset"""
    a = Ct(12, 5, 20, 34)
    assert ckks.min_k(3, 21, 12) == 24 and ckks.min_k(0, 0, 12) == 0 and ckks.min_k(3, 10, 12) == 24 and ckks.min_k(3, 9, 12) == 12
    assert ckks.get_mul_const_params(Ct(12, 5, 0, 0), a, Cst(3, 21)) == (31, 20, 24)          # 31 + 20 <= 60: no offset
    assert ckks.get_mul_const_params(Ct(12, 3, 0, 0), a, Cst(3, 21)) == (16, 20, 24 + 15)     # 51 - 36 = 15 squeezed out
    assert ckks.get_mul_const_params(Ct(12, 3, 0, 0), a, Cst(0, 0)) == (16, 20, 18)           # min_k = 0: the offset alone, 54 - 36
    with pytest.raises(ckks.CKKSError, match="precision underflow"):
        ckks.get_mul_const_params(Ct(12, 5, 0, 0), a, Cst(35, 0))                             # prec.log_delta > a.log_budget
    into = ckks.plan_mul_pt_const_into(Ct(12, 3, 0, 0), a, Cst(3, 21, re=[1, 2]))
    assert (into.log_budget, into.log_delta, into.cnv_offset) == (16, 20, 39)
    d = Ct(12, 5, 20, 34)
    asg = ckks.plan_mul_pt_const_assign(d, Cst(3, 21, im=[1]))
    assert (asg.log_budget, asg.log_delta, asg.cnv_offset, asg.name) == (31, 20, 24, "mul_pt_const_assign")


def test_composites_by_hand():
    B = 12
    a = Ct(B, 3, 12, 15)
    c = Cst(3, 9, re=[5, -7])
    # product budget 12; dst at 19 / 12 / 5
    hi = ckks.plan_mul_add_pt_const(Ct(B, 4, 11, 19), a, c)
    assert [(t.join, t.k, t.sign, t.cnv_offset) for t in hi.terms] == [(ckks.LSH_ACC, 7, 1, 12)] and hi.init_res and hi.normalize
    assert (hi.log_delta, hi.log_budget) == (11, 12)
    eq = ckks.plan_mul_sub_pt_const(Ct(B, 4, 13, 12), a, c)
    assert [(t.join, t.k, t.sign) for t in eq.terms] == [(ckks.PLAIN, 0, -1)] and (eq.log_delta, eq.log_budget) == (12, 12)
    lw = ckks.plan_mul_add_pt_const(Ct(B, 4, 12, 5), a, c, sub=True)
    assert [(t.join, t.k, t.sign) for t in lw.terms] == [(ckks.LSH_TERM, 7, -1)] and (lw.log_delta, lw.log_budget) == (12, 5)
    # an empty constant: no term, metadata untouched (composite.rs:301-303), also where the product itself would be refused
    none = ckks.plan_mul_add_pt_const(Ct(B, 4, 11, 19), Ct(B, 3, 12, 1), Cst(3, 9))
    assert none.terms == [] and (none.log_delta, none.log_budget) == (11, 19)

    class Recorder:
        calls = 0

        def glwe_lincomb_const_batched(self, *a, **k):
            self.calls += 1
    rec, d = Recorder(), Ct(B, 4, 11, 19)
    none.launch(rec, d, 3, [a], [Cst(3, 9)])
    assert rec.calls == 0 and (d.log_delta, d.log_budget) == (11, 19)
    # the dot product: n = 1 is the plain product (no normalize); an all-empty constant still aligns the budgets
    one = ckks.plan_dot_product_pt_const(Ct(B, 4, 0, 0), [a], [c])
    assert not one.normalize and not one.init_res and len(one.terms) == 1 and (one.log_delta, one.log_budget) == (12, 12)
    dp = ckks.plan_dot_product_pt_const(Ct(B, 4, 0, 0), [a, Ct(B, 3, 10, 8), Ct(B, 3, 12, 22)], [c, Cst(3, 9), c])
    assert [(t.index, t.join, t.k) for t in dp.terms] == [(0, ckks.PLAIN, 0), (1, ckks.LSH_ACC, 7), (2, ckks.LSH_TERM, 14)]
    assert dp.normalize and (dp.log_delta, dp.log_budget) == (10, 5)
    for ops, cs, msg in (([], [], "at least one pair"), ([a], [c, c], "length mismatch"), ([a, Ct(B, 3, 12, 2)], [c, c], "precision underflow"),
                         ([a, Ct(13, 3, 12, 15)], [c, c], "base2k")):
        with pytest.raises(ckks.CKKSError, match=msg):
            ckks.plan_dot_product_pt_const(Ct(B, 4, 0, 0), ops, cs)
    with pytest.raises(ckks.CKKSError, match="i64 overflow"):                                   # ensure_accumulation_fits: 2^(63 - 61) = 4 < 5
        ckks.plan_dot_product_pt_const(Ct(61, 4, 0, 0), [Ct(61, 3, 12, 15)] * 5, [c] * 5)


def test_entry_point_in_header_library_and_bindings():
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from poulpy_amd import abi, hal
    lib = hal.load_library()
    name = "pz_glwe_lincomb_const_batched"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poulpy_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % name, hdr) and hasattr(lib, name) and name in abi.PROTOTYPES
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == 19
    assert [fn.argtypes[i] for i in (2, 3, 4, 15, 18)] == [C.c_size_t] * 5 and fn.argtypes[16] is C.c_int and fn.argtypes[17] is C.c_int
    assert (abi.PZ_LINCOMB_INIT_NONE, abi.PZ_LINCOMB_INIT_RES) == (0, 1)
    assert (abi.PZ_JOIN_PLAIN, abi.PZ_JOIN_LSH_TERM, abi.PZ_JOIN_LSH_ACC) == (ckks.PLAIN, ckks.LSH_TERM, ckks.LSH_ACC) == (0, 1, 2)
    assert hal.Module.JOIN_KINDS == {"plain": 0, "lsh_term": 1, "lsh_acc": 2} and callable(hal.Module.glwe_lincomb_const_batched)
    assert fn(None, *([None] * 1), 1, 4, 12, *([None] * 10), 1, 0, 0, 1) == abi.PZ_ERR_INVALID and b"null module" in lib.pz_last_error()
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "ffi.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")).read()
    assert name + "(m_," in mirror and "fn %s(" % name in ffi and "ffi::%s(" % name in rust


# ---- the kernel's walk on the host, under the sanitizers ------------------------------------------------------------------------------
def _write_case(f, ref, sc, n, cols, seed):
    host = cases.host_inputs(seeded(seed), sc, n, cols, 1)
    want, ops = cases.on_host(sc, host, 0, n, cols)
    _oracle(ref, sc, want, ops)
    dst, ops = cases.on_host(sc, host, 0, n, cols)
    plan = _plan(sc, dst, ops)
    if not plan.terms:
        return 0
    f.write("%d %d %d %d %d %d %d\n" % (n, cols, dst.size, dst.base2k, len(plan.terms), int(plan.init_res), int(plan.normalize)))
    f.write(" ".join(str(int(v)) for v in host["dst"][0].reshape(-1)) + "\n")
    for t in plan.terms:
        o, c = ops[t.index], sc["csts"][t.index]
        b_size = len(c.re) if c.re is not None else (len(c.im) if c.im is not None else 0)
        f.write("%d %d %d %d %d %d %d %d\n" % (o.size, t.cnv_offset, c.re is not None, c.im is not None, b_size, t.join, t.k, t.sign < 0))
        for arr in (c.re, c.im):
            if arr is not None:
                f.write(" ".join(str(int(v)) for v in arr) + "\n")
        f.write(" ".join(str(int(v)) for v in o.data.data.reshape(-1)) + "\n")
    f.write(" ".join(str(int(v)) for v in want.data.data.reshape(-1)) + "\n")
    return 1


def test_walk_stand_alone_under_the_host_sanitizers(ref, tmp_path):
    """tests/cpp/test_lincomb_walk.cpp includes device_lincomb.hpp and calls lc_plan_term / lc_walk - the functions the kernel and its
    launcher call - on the host, with its own main.  Built by the HIP compiler with -fsanitize=address,undefined on the host side only
    (plain where the compiler has no sanitizer runtimes); run as a child process on every scenario at both bases, at N = 16 with 2 columns."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert shutil.which(hipcc) is not None, "the HIP compiler that builds the library"
    path = tmp_path / "cases.txt"
    count = 0
    with open(tmp_path / "body.txt", "w") as f:
        for B in (12, 19):
            for i, sc in enumerate(cases.scenarios(B)):
                count += _write_case(f, ref, sc, N, COLS, 7 * B + i)
    path.write_text("%d\n" % count + (tmp_path / "body.txt").read_text())
    exe = str(tmp_path / "test_lincomb_walk")
    base = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "poulpy_amd", "csrc"), "-I",
            os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_lincomb_walk.cpp"), "-o", exe]
    san = subprocess.run(base + ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[lincomb] HIP compiler without host sanitizer runtimes: built plain")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "all lincomb walk checks passed: %d cases" % count in r.stdout and count >= 50, r.stdout[-2000:]
