"""CPU: pz_glwe_sum_batched and the CKKS plans built on it (poulpy_amd/ckks.py: add_many, the products and composites by plaintext vectors)
against the literal restatement of the reference (tests/ckks_sum_oracle.py); the entry point in the header, the library and every
binding; the kernel's planner and per-thread walk (poulpy_amd/csrc/device_sum.hpp: sum_plan, sum_walk) run on the host by a stand-alone
program built with the host sanitizers, on the oracle chain's digits; and the decoded value of a dot product.  (The device:
tests/test_gpu_ckks_sum.py.)"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH_ACC, LSH_TERM, PLAIN, Ct, Pt
from poulpy_amd.layouts import VecZnx
from tests import ckks_sum_cases as cases
from tests import ckks_sum_oracle as so_sum
from tests.helpers import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, COLS = 16, 2


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


# ---- the kernel's planner and walk on the host, under the sanitizers ----------------------------------------------------------------------
def _chains(ref):
    """(base2k, res, terms, want): random chains over every base, size and term count of the device test, normalized and not, with term 0 =
    res (with and without a later shift of the running sum, and joined by a shift of its own)"""
    out = []
    for B in (5, 12, 17, 50):
        rng = seeded(9000 + B)
        for i in range(70):
            res_size = int(rng.choice([1, 2, 3, 5]))
            nterms = int(rng.choice([1, 2, 3, 5, 6])) if i % 10 else min(64, 1 << (63 - B))
            normalized = i % 4 < 2
            res = VecZnx(N, COLS, res_size)
            inplace = i % 3 == 2
            if inplace:
                cases.fill(rng, res, B, normalized)
            terms = cases.random_chain(rng, N, COLS, B, res_size, nterms, normalized, res if inplace else None,
                                       acc_shift=(i % 6 == 2) if inplace else None,
                                       res_k=int(rng.integers(B, 3 * B + 1)) if inplace and i % 12 == 5 else None)
            start = res.copy()
            so_sum.sum_chain(ref, B, res, terms)
            want = res
            terms = [(start if a is res else a, j, k, s) for a, j, k, s in terms]
            out.append((B, start, terms, want))
    return out


def test_walk_stand_alone_under_the_host_sanitizers(ref, tmp_path):
    """tests/cpp/test_sum_walk.cpp includes device_sum.hpp and calls sum_plan / sum_walk - the functions the kernel and its entry point call
    - on the host, with its own main.  Built by the HIP compiler with -fsanitize=address,undefined on the host side only (plain where the
    compiler has no sanitizer runtimes); run as a child process on 280 random chains the oracle ran, at N = 16 with 2 columns."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert shutil.which(hipcc) is not None, "the HIP compiler that builds the library"
    chains = _chains(ref)
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        f.write("%d\n" % len(chains))
        for B, res, terms, want in chains:
            cases.write_chain(f, B, res, terms, want)
    joins = {(j, k % B == 0, k >= B) for B, _, terms, _ in chains for _, j, k, _ in terms}
    # term 0 = res moved by its own shift of a limb or more, in containers that keep some of it
    assert sum(terms[0][0] is res and terms[0][1] == LSH_TERM and terms[0][2] // B < res.size for B, res, terms, _ in chains) >= 4
    assert joins >= {(PLAIN, True, False), (LSH_TERM, False, False), (LSH_TERM, False, True), (LSH_TERM, True, True), (LSH_ACC, False, False),
                     (LSH_ACC, False, True), (LSH_ACC, True, True)}
    exe = str(tmp_path / "test_sum_walk")
    base = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "poulpy_amd", "csrc"), "-I",
            os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_sum_walk.cpp"), "-o", exe]
    san = subprocess.run(base + ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[sum] HIP compiler without host sanitizer runtimes: built plain")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"all sum walk checks passed: (\d+) cases, (\d+) staged, (\d+) with dropped terms", r.stdout)
    assert m and int(m.group(1)) == len(chains) >= 250 and int(m.group(2)) >= 5 and int(m.group(3)) >= 5, r.stdout[-2000:]


def test_entry_point_in_header_library_and_bindings():
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from poulpy_amd import abi, hal
    lib = hal.load_library()
    name = "pz_glwe_sum_batched"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poulpy_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % name, hdr) and hasattr(lib, name) and name in abi.PROTOTYPES
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    assert [fn.argtypes[i] for i in (2, 3, 4, 11, 12)] == [C.c_size_t] * 5
    assert callable(hal.Module.glwe_sum_batched)
    assert fn(None, None, 2, 4, 12, *([None] * 6), 1, 1) == abi.PZ_ERR_INVALID and b"null module" in lib.pz_last_error()
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "ffi.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")).read()
    assert name + "(m_," in mirror and "fn %s(" % name in ffi and "ffi::%s(" % name in rust
    # the header states what becomes of an in-place term 0 that a later join shifts
    doc = open(os.path.join(ROOT, "include", "poulpy_hip.h")).read()
    block = doc[doc.index("Normalized signed sum of up to 64"):doc.index("int pz_glwe_sum_batched")]
    assert "staged" in block and "32 limbs" in block and "PZ_ERR_ALIAS" in block


# ---- the plans against the literal restatement ------------------------------------------------------------------------------------------------
def _meta(ct):
    return ct.log_delta, ct.log_budget


@pytest.mark.parametrize("B", [12, 17])
def test_add_many_plans_reproduce_the_oracle(ref, B):
    """every scenario: ckks_add_many restated on the oracle's primitives, and the plan's own term list as pz_glwe_sum_batched is asked to
    compute it - same digits, same metadata; the chain route's calls, run on the same primitives, give the same digits again"""
    joins = []
    for i, (label, dst, inputs) in enumerate(cases.add_many_scenarios(B)):
        rng = seeded(B * 131 + i)
        ins = [cases.materialize(rng, N, x) for x in inputs]
        want = cases.materialize(rng, N, dst)
        so_sum.ckks_add_many(ref, want, ins)
        got = cases.materialize(rng, N, dst)
        plan = ckks.plan_add_many(got, ins)
        so_sum.run_sum_plan(ref, plan, got, ins)
        assert _meta(got) == _meta(want), label
        assert np.array_equal(got.data.data, want.data.data), label
        if plan.normalize:
            via = cases.materialize(rng, N, dst)
            _run_chain_calls(ref, ckks.chain_calls(plan.terms), via, lambda t: ins[t.index].data)
            assert np.array_equal(via.data.data, want.data.data), label
        joins += [(u, t.join) for u, t in enumerate(plan.terms)]
    assert {j for _, j in joins} == {PLAIN, LSH_TERM, LSH_ACC} and any(j == LSH_ACC and u >= 2 for u, j in joins)


def _run_chain_calls(ref, calls, dst, operand, started=False):
    """pz_glwe_combine_batched's contract on the oracle: the terms applied in order to a zero container, the last call normalized"""
    from tests import shift_oracle as so
    B = dst.base2k
    for n, call in enumerate(calls):
        assert 1 <= len(call) <= 4 and sum(isinstance(src, str) for src, *_ in call) <= 1
        old = dst.data.copy()
        new = VecZnx(N, dst.cols, dst.size)
        for src, kind, k, sign in call:
            a = old if isinstance(src, str) else operand(src)
            if kind == ckks.RAW:
                (so.glwe_sub_assign if sign < 0 else so.glwe_add_assign)(ref, new, a)
            else:
                (so.glwe_lsh_sub if sign < 0 else so.glwe_lsh_add)(B, k, new, a)
        if n == len(calls) - 1:
            so.glwe_normalize_assign(ref, B, new)
        dst.data.data[...] = new.data


def test_chain_calls_by_hand():
    T = ckks.SumTerm
    t = [T(0), T(1), T(2), T(3), T(4, LSH_TERM, 5), T(5, LSH_ACC, 7), T(6, LSH_ACC, 3), T(7)]
    calls = ckks.chain_calls(t)
    shape = [[(s if isinstance(s, str) else s.index, kind, k) for s, kind, k, _ in c] for c in calls]
    assert shape == [[(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], [("dst", 0, 0), (4, 1, 5)], [("dst", 1, 7), (5, 0, 0)],
                     [("dst", 1, 3), (6, 0, 0), (7, 0, 0)]]
    cont = ckks.chain_calls([T(0, LSH_ACC, 9), T(1)], started=True)
    assert [[(s if isinstance(s, str) else s.index, kind, k) for s, kind, k, _ in c] for c in cont] == [[("dst", 1, 9), (0, 0, 0), (1, 0, 0)]]


def test_get_mul_pt_params_by_hand():
    """mul.rs:480-496: budget = a.log_budget - pt.log_delta; offset = (budget + a.log_delta) -| res.max_k; cnv = pt.max_k + offset"""
    a = Ct(12, 5, 27, 33)
    pt = Pt(12, 2, 15, log_budget=9)
    assert ckks.get_mul_pt_params(Ct(12, 5, 0, 0), a, pt) == (18, 27, 24)           # 18 + 27 <= 60: no offset
    assert ckks.get_mul_pt_params(Ct(12, 3, 0, 0), a, pt) == (9, 27, 24 + 9)        # 45 - 36 = 9 squeezed out
    with pytest.raises(ckks.CKKSError, match="precision underflow"):
        ckks.get_mul_pt_params(Ct(12, 5, 0, 0), a, Pt(12, 3, 34, log_budget=2))
    into = ckks.plan_mul_pt_vec_znx_into(Ct(12, 3, 0, 0), a, pt)
    assert (into.log_budget, into.log_delta, into.cnv_offset, into.name) == (9, 27, 33, "mul_pt_vec_znx_into")
    asg = ckks.plan_mul_pt_vec_znx_assign(Ct(12, 5, 27, 33), pt)
    assert (asg.log_budget, asg.log_delta, asg.cnv_offset, asg.name) == (18, 27, 24, "mul_pt_vec_znx_assign")


@pytest.mark.parametrize("B", [12, 17])
def test_pt_vec_plans_reproduce_the_oracle(ref, B):
    """mul_pt_vec_znx into / assign, mul_add and mul_sub: the literal restatement against the plans' own amounts on the same primitives"""
    from tests import plain_oracle as po
    from tests import shift_oracle as so
    for i, (label, dst, a, pt) in enumerate(cases.pt_scenarios(B)):
        rng = seeded(B * 977 + i)
        ha, hp = cases.materialize(rng, N, a), cases.materialize_pt(rng, N, pt)
        # into
        want = cases.materialize(rng, N, dst)
        so_sum.ckks_mul_pt_vec_znx_into(ref, want, ha, hp)
        got = cases.clone(want)
        got.data.data[...] = 0
        plan = ckks.plan_mul_pt_vec_znx_into(got, ha, hp)
        po.glwe_mul_plain(ref, plan.cnv_offset, got.data, B, ha.data, ha.effective_k, hp.data, hp.max_k, B)
        plan.apply_meta(got)
        assert _meta(got) == _meta(want) and np.array_equal(got.data.data, want.data.data), label
        # assign: the operand is the destination
        want = cases.clone(ha)
        so_sum.ckks_mul_pt_vec_znx_into(ref, want, want, hp)
        got = cases.clone(ha)
        plan = ckks.plan_mul_pt_vec_znx_assign(got, hp)
        po.glwe_mul_plain_assign(ref, plan.cnv_offset, got.data, got.effective_k, hp.data, hp.max_k, B)
        plan.apply_meta(got)
        assert _meta(got) == _meta(want) and np.array_equal(got.data.data, want.data.data), label
        # mul_add / mul_sub at three budgets of dst: below, at and above the product's
        for sub in (False, True):
            prod_budget = ckks.get_mul_pt_params(dst, ha, hp)[0]
            for budget in (max(prod_budget - 5, 0), prod_budget, prod_budget + B + 1):
                want = cases.materialize(rng, N, Ct(B, dst.size, dst.log_delta, budget, dst.cols))
                got = cases.clone(want)
                so_sum.ckks_mul_add_pt_vec_znx(ref, want, ha, hp, sub=sub)
                plan = (ckks.plan_mul_sub_pt_vec_znx if sub else ckks.plan_mul_add_pt_vec_znx)(got, ha, hp)
                tmp = Ct(B, dst.size, 0, 0, dst.cols, VecZnx(N, dst.cols, dst.size))
                po.glwe_mul_plain(ref, plan.mul.cnv_offset, tmp.data, B, ha.data, ha.effective_k, hp.data, hp.max_k, B)
                plan.mul.apply_meta(tmp)
                so.run(ref, plan.add, got, tmp)
                plan.apply_meta(got)
                assert plan.add.normalize and _meta(got) == _meta(want) and np.array_equal(got.data.data, want.data.data), (label, sub, budget)


@pytest.mark.parametrize("B", [12, 17])
def test_dot_product_plans_reproduce_the_oracle(ref, B):
    """the literal dot product against the plan's products and joins, joined whole and in chunks of 1 and 2 scratch slots"""
    joins = []
    for i, (label, dst, ops, pts) in enumerate(cases.dot_scenarios(B)):
        rng = seeded(B * 389 + i)
        hops, hpts = [cases.materialize(rng, N, a) for a in ops], [cases.materialize_pt(rng, N, p) for p in pts]
        want = cases.materialize(rng, N, dst)
        so_sum.ckks_dot_product_pt_vec_znx(ref, want, hops, hpts)
        for slots in (None, 1, 2):
            got = cases.materialize(rng, N, dst)
            plan = ckks.plan_dot_product_pt_vec_znx(got, hops, hpts)
            so_sum.run_dot_plan(ref, plan, got, hops, hpts, slots)
            assert _meta(got) == _meta(want) and np.array_equal(got.data.data, want.data.data), (label, slots)
        joins += [(u, t.join) for u, t in enumerate(plan.terms)]
    assert {j for _, j in joins} == {PLAIN, LSH_TERM, LSH_ACC} and any(j == LSH_ACC and u >= 2 for u, j in joins)


def test_plan_refusals():
    B = 12
    a = Ct(B, 5, 27, 33)
    pt = Pt(B, 2, 15, log_budget=9)
    with pytest.raises(ckks.CKKSError, match="at least one ciphertext"):
        ckks.plan_add_many(Ct(B, 5, 0, 0), [])
    with pytest.raises(ckks.CKKSError, match="i64 overflow"):                       # ensure_accumulation_fits: 2^(63 - 61) = 4 < 5
        ckks.plan_add_many(Ct(61, 4, 0, 0), [Ct(61, 3, 12, 15)] * 5)
    with pytest.raises(ckks.CKKSError, match="base2k"):
        ckks.plan_add_many(Ct(B, 5, 0, 0), [a, Ct(13, 5, 27, 33)])
    with pytest.raises(ckks.CKKSError, match="insufficient homomorphic capacity"):  # offset_unary 60 - 24 = 36 > 33
        ckks.plan_add_many(Ct(B, 2, 0, 0), [a])
    for ops, ps, msg in (([], [], "at least one pair"), ([a], [pt, pt], "length mismatch"), ([a, Ct(B, 3, 27, 9)], [pt, pt], "precision underflow"),
                         ([a, Ct(13, 5, 27, 38)], [pt, pt], "base2k"), ([a], [Pt(13, 2, 15)], "base2k"),
                         ([Ct(B, 5, 27, 20)], [pt], "ciphertext size"), ([a], [_short_pt()], "plaintext size")):
        with pytest.raises(ckks.CKKSError, match=msg):
            ckks.plan_dot_product_pt_vec_znx(Ct(B, 5, 0, 0), ops, ps)
    with pytest.raises(ckks.CKKSError, match="i64 overflow"):
        ckks.plan_dot_product_pt_vec_znx(Ct(61, 4, 0, 0), [Ct(61, 3, 100, 83)] * 5, [Pt(61, 1, 3)] * 5)
    with pytest.raises(ckks.CKKSError, match="ciphertext size"):
        ckks.plan_mul_pt_vec_znx_into(Ct(B, 5, 0, 0), Ct(B, 5, 27, 20), pt)
    with pytest.raises(ckks.CKKSError, match="ciphertext size"):
        ckks.plan_mul_pt_vec_znx_assign(Ct(B, 5, 27, 20), pt)
    with pytest.raises(ckks.CKKSError, match="precision underflow"):
        ckks.plan_mul_add_pt_vec_znx(Ct(B, 5, 27, 33), Ct(B, 3, 27, 9), pt)
    plan = ckks.plan_dot_product_pt_vec_znx(Ct(B, 5, 0, 0), [a, a], [pt, pt])
    for kw in (dict(tmp=None, slots=1), dict(tmp=1 << 20, slots=0), dict(tmp=1 << 20, slots=3), dict(tmp=1 << 20, slots=1, route="fused")):
        with pytest.raises(ckks.CKKSError):
            plan.launch(None, Ct(B, 5, 0, 0), 1, [a, a], [pt, pt], **kw)
    with pytest.raises(ckks.CKKSError, match="route"):
        ckks.plan_add_many(Ct(B, 5, 0, 0), [a, a]).launch(None, Ct(B, 5, 0, 0), 1, [a, a], route="fused")
    assert ckks.sum_route(2) == (2 in ckks.SUM_WINS) and not ckks.sum_route(65)


def test_plans_raise_before_the_first_launch_what_the_calls_would_refuse():
    """more than 64 terms in one pz_glwe_sum_batched, and a running sum of more than 32 limbs shifted in place by a limb or more (neither
    route serves it): CKKSError, and not one call reaches the module"""
    B = 12

    class Recorder:
        calls = 0

        def n(self):
            return 16

        def __getattr__(self, name):
            def call(*a, **k):
                self.calls += 1
            return call
    a = Ct(B, 5, 27, 33)
    pt = Pt(B, 2, 15, log_budget=9)
    rec = Recorder()
    many = ckks.plan_add_many(Ct(B, 5, 0, 0), [a] * 65)
    with pytest.raises(ckks.CKKSError, match="65 terms in one pz_glwe_sum_batched"):
        many.launch(rec, Ct(B, 5, 0, 0), 1, [a] * 65, route="sum")
    dot = ckks.plan_dot_product_pt_vec_znx(Ct(B, 5, 0, 0), [a] * 130, [pt] * 130)
    with pytest.raises(ckks.CKKSError, match="65 terms in one pz_glwe_sum_batched"):
        dot.launch(rec, Ct(B, 5, 0, 0), 1, [a] * 130, [pt] * 130, tmp=1 << 20, slots=64, route="sum")
    assert rec.calls == 0
    many.launch(rec, Ct(B, 5, 0, 0), 1, [a] * 65)                                   # unrouted: the chain
    dot.launch(rec, Ct(B, 5, 0, 0), 1, [a] * 130, [pt] * 130, tmp=1 << 20, slots=63, route="sum")
    assert rec.calls == 22 + (130 + 3)                                              # 4 + 3 x 20 + 1 inputs; 130 products, 3 joins
    # 33 limbs: the third input lies a limb and a bit below the running sum
    wide = [Ct(B, 33, 40, 33 * B - 40), Ct(B, 33, 40, 33 * B - 40), Ct(B, 33, 40, 32 * B - 41)]
    rec = Recorder()
    plan = ckks.plan_add_many(Ct(B, 33, 0, 0), wide)
    assert [t.join for t in plan.terms] == [PLAIN, PLAIN, LSH_ACC] and plan.terms[2].k == B + 1
    with pytest.raises(ckks.CKKSError, match="shifted in place"):
        plan.launch(rec, Ct(B, 33, 0, 0), 1, wide, route="chain")
    plan.launch(rec, Ct(B, 33, 0, 0), 1, wide, route="sum")                         # one pass from a zero container: nothing in place
    assert rec.calls == 1
    wpt = Pt(B, 2, 15, log_budget=9)
    wops = [Ct(B, 33, 40, 33 * B - 40), Ct(B, 33, 40, 33 * B - 40), Ct(B, 33, 40, 33 * B - 40 - B - 1)]
    wops[2].size = 32                                                               # effective_k = 32 base2k - 1
    dotw = ckks.plan_dot_product_pt_vec_znx(Ct(B, 33, 0, 0), wops, [wpt] * 3)
    assert dotw.terms[2].join == LSH_ACC and dotw.terms[2].k == B + 1
    rec = Recorder()
    for route in ("sum", "chain", None):
        with pytest.raises(ckks.CKKSError, match="shifted in place"):
            dotw.launch(rec, Ct(B, 33, 0, 0), 1, wops, [wpt] * 3, tmp=1 << 20, slots=2, route=route)
    assert rec.calls == 0
    dotw.launch(rec, Ct(B, 33, 0, 0), 1, wops, [wpt] * 3, tmp=1 << 20, slots=3, route="sum")
    assert rec.calls == 4


def _short_pt():
    class Odd(Pt):                       # a plaintext whose size disagrees with its max_k (glwe.rs:209 would assert)
        @property
        def max_k(self):
            return 30
    return Odd(12, 2, 15, log_budget=9)


# ---- the decoded value, with one-amount-wrong controls ----------------------------------------------------------------------------------------
def _negacyclic(a, b):
    """(cols, n) x (n,) -> (cols, n) over Python ints, X^n = -1"""
    n = a.shape[-1]
    out = np.zeros_like(a)
    for i in range(n):
        for j in range(n):
            if b[j] != 0:
                if i + j < n:
                    out[:, i + j] += a[:, i] * b[j]
                else:
                    out[:, i + j - n] -= a[:, i] * b[j]
    return out


def test_dot_product_value_with_controls(ref):
    """The decoded result of a dot product is sum_i value(pt_i) value(ct_i) on exact integers.  Allowance, in units of the last limb of
    dst: every product is rounded once into dst's layout at its own budget (vec_znx_big_normalize: half a unit, times 1 / (1 - 2^-base2k)
    for the rounding of the digits below), and a join that shifts a product up by d bits scales that by 2^d; the joins and the closing
    normalize are exact.  A cnv_offset or a join shift wrong by one bit moves the result by far more than that."""
    from tests import ckks_meaning as cm
    B = 12
    a5 = Ct(B, 5, 2 * B + 3, 3 * B - 3)                       # full precision: effective_k = max_k, nothing masked away
    dst, ops = Ct(B, 5, 0, 0), [a5] * 4
    pts = [Pt(B, 2, B + d, log_budget=B - d) for d in (3, 5, 3, 1)]   # product budgets 18, 16, 18, 20: plain, lsh_acc, lsh_term, lsh_term
    rng = seeded(4242)
    hops, hpts = [cases.materialize(rng, N, a) for a in ops], [cases.materialize_pt(rng, N, p) for p in pts]

    def run(mutate=None):
        got = cases.materialize(seeded(1), N, dst)
        plan = ckks.plan_dot_product_pt_vec_znx(got, hops, hpts)
        if mutate:
            mutate(plan)
        so_sum.run_dot_plan(ref, plan, got, hops, hpts)
        return plan, got

    plan, got = run()
    lb = plan.log_budget
    v, allow = None, 0.0
    for a, p, t in zip(hops, hpts, plan.terms):
        va, vp = cm.value_ct(a), cm.value_pt(p)
        term = cm.Val(_negacyclic(va.num, vp.num[0]), va.e + vp.e)
        v = term if v is None else cm.vsum(v, term)
        allow += cm.carried(cm.HALF(B), t.log_budget, lb)
    want = cm.place(v, lb)
    dev = cm.deviation_ulps(got.data, want, got.size, B)
    print("[sum] dot product value: deviation %.3f units of the last limb, allowance %.3f" % (dev, allow))
    assert dev <= allow
    shifted = [u for u, t in enumerate(plan.terms) if t.join != PLAIN]
    assert shifted

    def wrong_offset(p):
        p.terms[1].cnv_offset += 1

    def wrong_shift(p):
        p.terms[shifted[0]].k += 1
    for mutate in (wrong_offset, wrong_shift):
        _, bad = run(mutate)
        assert cm.deviation_ulps(bad.data, want, bad.size, B) > 8 * allow, mutate.__name__
