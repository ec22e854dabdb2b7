"""CPU: the plan of ckks_dot_product_ct (poulpy_amd/ckks.py plan_dot_product_ct) against the literal restatement of the reference
(tests/ckks_dot_oracle.py) on every scenario of tests/ckks_dot_cases.py; its refusals in the reference's order; the form of the accumulated
tensor (poulpy_amd/csrc/dot_form.hpp) pinned at its boundaries; the entry point pz_glwe_tensor_dot_relinearize_batched in the header, the
library and every binding; the order and arguments of the launches on a recording module.  (The device: tests/test_gpu_ckks_dot.py.)"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH, Ct
from poulpy_amd.layouts import VecZnx
from tests import ckks_dot_cases as dcases
from tests import ckks_dot_oracle as do
from tests import ckks_mul_cases as cases
from tests import ckks_mul_oracle as mo
from tests import ckks_sum_oracle as so_sum
from tests import shift_oracle as so
from tests.helpers import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
B = 12


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


def _meta(ct):
    return ct.log_delta, ct.log_budget


def _key(ref, rng, rank, limbs):
    mat = cases.random_tensor_key(rng, N, B, rank, limbs, limbs + 1)
    pm = ref.vmp_pmat_alloc(limbs, rank * (rank + 1) // 2, rank + 1, limbs + 1)
    ref.vmp_prepare(pm, mat)
    return mo.Tsk(pm, 1, B)


def _empty(size, cols):
    return Ct(B, size, 0, 0, cols, VecZnx(N, cols, size))


# ---- the plan against the literal restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [1, 2])
def test_plan_reproduces_the_literal_restatement_on_every_scenario(ref, rank):
    """digits and metadata at N = 64; the branch the plan takes is the scenario's; on the fast branch the tensor has
    max(a_target_eff_k, b_target_eff_k).div_ceil(base2k) limbs, and only an unaligned side is rescaled - all of its inputs"""
    limbs, cols = 5, rank + 1
    rng = seeded(70 + rank)
    tsk = _key(ref, rng, rank, limbs)
    for label, branch, dsize, a_list, b_list in dcases.dot_scenarios(B, cols, limbs):
        ha = [cases.fill_ct(rng, N, x) for x in a_list]
        hb = [cases.fill_ct(rng, N, x) for x in b_list]
        d1, d2 = _empty(dsize, cols), _empty(dsize, cols)
        plan = ckks.plan_dot_product_ct(d1, ha, hb)
        assert plan.branch == branch and plan.n == dcases.NPAIRS, label
        do.run_dot_plan(ref, plan, d1, ha, hb, tsk)
        do.ckks_dot_product_ct(ref, d2, ha, hb, tsk)
        assert np.array_equal(d1.data.data, d2.data.data), label
        assert _meta(d1) == _meta(d2) == (plan.log_delta, plan.log_budget), label
        assert np.any(d1.data.data), label
        if branch == "fast":
            a_eff = min(x.log_budget for x in a_list) + a_list[0].log_delta
            b_eff = min(x.log_budget for x in b_list) + b_list[0].log_delta
            assert (plan.a_effective_k, plan.b_effective_k) == (a_eff, b_eff), label
            assert plan.tensor_size == -(-max(a_eff, b_eff) // B) and (plan.a_size, plan.b_size) == (-(-a_eff // B), -(-b_eff // B)), label
            want = {s for s, xs in (("a", a_list), ("b", b_list)) if len({x.log_budget for x in xs}) > 1}
            assert set(plan.rescales) == want and all(len(v) == dcases.NPAIRS for v in plan.rescales.values()), label
            assert (plan.scratch_bytes(3, N) == 0) == (not want), label
        else:
            assert [p.join is None for p in plan.muls] == [True, False, False] and plan.scratch_bytes(3, N) == 0, label
    # the aligned case in numbers: 5 limbs of 12 bits, log_delta 20, three pairs
    full = [cases.fresh(B, 60) for _ in range(3)]
    p = ckks.plan_dot_product_ct(Ct(B, 5, 0, 0), full, full)
    assert (p.log_delta, p.log_budget, p.cnv_offset, p.tensor_size, p.a_strides, p.b_strides) == (20, 20, 60, 5, [5] * 3, [5] * 3)
    p = ckks.plan_dot_product_ct(Ct(B, 4, 0, 0), full, full)                                   # smaller output: res_offset 40 - 48 < 0
    assert (p.log_delta, p.log_budget, p.cnv_offset) == (20, 20, 60)
    p = ckks.plan_dot_product_ct(Ct(B, 3, 0, 0), full, full)                                   # res_offset 4
    assert (p.log_delta, p.log_budget, p.cnv_offset) == (20, 16, 64)
    # one a-side input at k = 49: every a input is rescaled to effective_k 49 (shifts 11, 0, 11), the tensor follows the b side
    short = [cases.fresh(B, 49 if i == 1 else 60) for i in range(3)]
    p = ckks.plan_dot_product_ct(Ct(B, 5, 0, 0), short, full)
    assert [r.shift for r in p.rescales["a"]] == [11, 0, 11] and (p.a_effective_k, p.b_effective_k, p.a_size, p.tensor_size) == (49, 60, 5, 5)
    assert (p.log_delta, p.log_budget, p.cnv_offset) == (20, 9, 60)


def test_one_pair_is_plan_mul_into(ref):
    rng = seeded(75)
    tsk = _key(ref, rng, 1, 5)
    for label, dsize, a, b in cases.mul_scenarios(B):
        ha, hb = cases.fill_ct(rng, N, a), cases.fill_ct(rng, N, b)
        d1, d2, d3 = _empty(dsize, 2), _empty(dsize, 2), _empty(dsize, 2)
        plan = ckks.plan_dot_product_ct(d1, [ha], [hb])
        assert plan.branch == "single" and plan.muls == [ckks.plan_mul_into(d1, ha, hb)], label
        do.run_dot_plan(ref, plan, d1, [ha], [hb], tsk)
        mo.run_mul_plan(ref, ckks.plan_mul_into(d2, ha, hb), d2, ha, hb, tsk)
        do.ckks_dot_product_ct(ref, d3, [ha], [hb], tsk)
        assert np.array_equal(d1.data.data, d2.data.data) and np.array_equal(d1.data.data, d3.data.data) and _meta(d1) == _meta(d2) == _meta(d3), label


def test_fallback_last_join_with_normalize_is_add_unsafe_then_normalize(ref):
    """what the last call of the fallback branch is asked for (accumulate = 1, normalize = 1: tests/ckks_mul_oracle.join) is the reference's
    ckks_add_assign_unsafe followed by the closing glwe_normalize_assign, on an un-normalized running sum, for every join kind"""
    rng = seeded(76)
    for d_budget in (12, 20, 33):                                                             # product budget 20: lsh_acc / plain / lsh_term
        acc = cases.fill_ct(rng, N, Ct(B, 5, cases.D, d_budget), normalized=False)
        prod = cases.fill_ct(rng, N, Ct(B, 5, cases.D, 20))
        join, k = ckks._join(acc.log_budget, prod.log_budget)
        v = acc.data.copy()
        mo.join(ref, B, v, prod.data, join, k, 1, True)
        so_sum.ckks_add_assign_unsafe(ref, acc, prod)
        so.glwe_normalize_assign(ref, B, acc.data)
        assert np.array_equal(v.data, acc.data.data), d_budget


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_in_the_references_order_with_its_messages(ref):
    full = lambda n=3: [cases.fresh(B, 60) for _ in range(n)]                                 # noqa: E731
    dst = Ct(B, 5, 0, 0)
    low = [cases.fresh(B, 60), Ct(B, 5, 20, 10), cases.fresh(B, 60)]                          # min budget 10 < log_delta 20
    small = [cases.fresh(B, 60), Ct(B, 4, 20, 40), cases.fresh(B, 60)]                        # effective_k 60 in 4 limbs
    with pytest.raises(ckks.CKKSError, match=r"ckks_dot_product_ct: inputs must contain at least one pair"):
        ckks.plan_dot_product_ct(dst, [], [])
    with pytest.raises(ckks.CKKSError, match=r"ckks_dot_product_ct: length mismatch between ct vector \(3\) and weight vector \(2\)"):
        ckks.plan_dot_product_ct(dst, full(), full(2))
    wide = [cases.fresh(62, 124) for _ in range(3)]
    with pytest.raises(ckks.CKKSError, match=r"ckks_dot_product_ct: 3 terms risks i64 overflow at base2k=62"):
        ckks.plan_dot_product_ct(Ct(62, 2, 0, 0), wide, wide)
    with pytest.raises(ckks.CKKSError, match=r"length mismatch"):                             # ... before the accumulation bound
        ckks.plan_dot_product_ct(Ct(62, 2, 0, 0), wide, wide[:2])
    with pytest.raises(ckks.CKKSError, match=r"dot_product_ct: multiplication precision underflow \(lhs log_budget 40, log_delta 20; rhs log_budget 10, log_delta 20\)"):
        ckks.plan_dot_product_ct(dst, full(), low)
    with pytest.raises(ckks.CKKSError, match=r"dot_product_ct: insufficient homomorphic capacity \(log_budget 20 < 28\)"):
        ckks.plan_dot_product_ct(Ct(B, 1, 0, 0), full(), full())
    with pytest.raises(ckks.CKKSError, match=r"dot_product_ct: the container \(4 limbs\) is smaller than effective_k 60"):
        ckks.plan_dot_product_ct(dst, small, full())
    with pytest.raises(ckks.CKKSError, match=r"dot_product_ct: 65 pairs in one pz_glwe_tensor_dot_relinearize_batched \(at most 64\)"):
        ckks.plan_dot_product_ct(dst, full(65), full(65))
    assert ckks.plan_dot_product_ct(dst, full(64), full(64)).n == 64 == ckks.DOT_MAX_PAIRS
    # the order: each refusal wins over every later one
    small_low = [Ct(B, 4, 20, 40), Ct(B, 5, 20, 10), cases.fresh(B, 60)]
    with pytest.raises(ckks.CKKSError, match="precision underflow"):
        ckks.plan_dot_product_ct(Ct(B, 1, 0, 0), small_low, full())
    with pytest.raises(ckks.CKKSError, match="insufficient homomorphic capacity"):
        ckks.plan_dot_product_ct(Ct(B, 1, 0, 0), small, full())
    with pytest.raises(ckks.CKKSError, match="smaller than effective_k"):
        ckks.plan_dot_product_ct(dst, [Ct(B, 4, 20, 40)] * 65, full(65))
    # the fallback branch refuses what its products refuse, pair by pair
    mixed = [Ct(B, 5, 12, 48), cases.fresh(B, 60), cases.fresh(B, 60)]
    assert ckks.plan_dot_product_ct(dst, full(), mixed).branch == "fallback"
    with pytest.raises(ckks.CKKSError, match="mul: insufficient homomorphic capacity"):
        ckks.plan_dot_product_ct(Ct(B, 1, 0, 0), full(), mixed)
    with pytest.raises(ckks.CKKSError, match="base2k"):
        ckks.plan_dot_product_ct(dst, full(), [cases.fresh(17, 68)] * 3)
    # the literal restatement refuses the same cases
    for d, xs, ys in ((dst, [], []), (dst, full(), full(2)), (dst, full(), low), (Ct(B, 1, 0, 0), full(), full())):
        with pytest.raises(ckks.CKKSError):
            hx = [Ct(x.base2k, x.size, x.log_delta, x.log_budget, 2, VecZnx(N, 2, x.size)) for x in xs]
            hy = [Ct(y.base2k, y.size, y.log_delta, y.log_budget, 2, VecZnx(N, 2, y.size)) for y in ys]
            do.ckks_dot_product_ct(ref, Ct(B, d.size, 0, 0, 2, VecZnx(N, 2, d.size)), hx, hy, None)


# ---- the form of the accumulated tensor -------------------------------------------------------------------------------------------------------
def test_tensor_form_is_pinned_at_its_boundaries(tmp_path):
    """tests/cpp/test_dot_form.cpp includes poulpy_amd/csrc/dot_form.hpp - the function the entry point calls - with the host compiler: the
    16-bit form exactly where npairs 3 2^(base2k-1) <= 2^15 - 1 on compact shapes (5 pairs at base2k 12, 2 at 13, 1 at 14, never above 14),
    and not at the 15 pairs the diagonal columns alone would admit.  Built with the host sanitizers linked in where the compiler has them."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "test_dot_form")
    base = [cxx, "-std=c++17", "-O1", "-g", os.path.join(ROOT, "tests", "cpp", "test_dot_form.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all dot-form checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------------
def test_entry_point_in_header_library_and_bindings():
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from poulpy_amd import abi, hal
    lib = hal.load_library()
    name, ws = "pz_glwe_tensor_dot_relinearize_batched", "pz_glwe_tensor_dot_relinearize_workspace_bytes"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poulpy_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % name, hdr) and re.search(r"\bsize_t %s\s*\(" % ws, hdr)
    assert hasattr(lib, name) and hasattr(lib, ws) and name in abi.PROTOTYPES and ws in abi.PROTOTYPES
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == 11 and getattr(lib, ws).restype is C.c_size_t and len(getattr(lib, ws).argtypes) == 5
    assert fn.argtypes[8] is C.POINTER(hal.GlweTensorParams) and fn.argtypes[9] is C.POINTER(hal.GlweOpParams)
    assert [fn.argtypes[i] for i in (4, 10)] == [C.c_size_t] * 2 and [fn.argtypes[i] for i in (2, 3, 5, 6)] == [C.c_void_p] * 4
    assert callable(hal.Module.glwe_tensor_dot_relinearize_batched) and callable(hal.Module.glwe_tensor_dot_relinearize_workspace_bytes)
    assert fn(None, None, None, None, 1, None, None, None, None, None, 1) == abi.PZ_ERR_INVALID and b"null module" in lib.pz_last_error()
    assert getattr(lib, ws)(None, None, None, 1, 1) == 0
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "ffi.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")).read()
    assert name + "(m_," in mirror and ws + "(m_," in mirror and "fn %s(" % name in ffi and "fn %s(" % ws in ffi and "ffi::%s(" % name in rust
    # no new parameter struct; the header states the semantics, the alias rule, the two forms and the refusals
    doc = open(os.path.join(ROOT, "include", "poulpy_hip.h")).read()
    block = doc[doc.index("The sum of npairs products in ONE GLWETensor"):doc.index("size_t " + ws)]
    for word in ("glwe_tensor_apply_add_assign", "HOST arrays", "PZ_ERR_ALIAS", "never\n * reaches caller memory", "npairs 3 2^(base2k-1) <= 2^15 - 1",
                 "above 64", "Nothing is launched on a refusal", "HIP graph"):
        assert word in block, word
    with pytest.raises(ValueError, match="one b pointer and one stride per a pointer"):
        hal.Module._dot_lists([1, 2], [1], None, None)
    n, pa, pb, sa, sb = hal.Module._dot_lists([16, 32], [48, 16], [6, 6], None)
    assert (n, list(pa), list(pb), list(sa), sb) == (2, [16, 32], [48, 16], [6, 6], None)


# ---- the launches --------------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for a Module: records the calls DotCtPlan.launch issues"""

    def __init__(self, n):
        self._n, self.calls = n, []

    def n(self):
        return self._n

    def glwe_combine_batched(self, res, res_cols, res_size, base2k, terms, normalize, batch):
        self.calls.append(("combine", res, res_cols, res_size, base2k, [(t["a"], t["a_size"], t["kind"], t["k"]) for t in terms], normalize, batch))

    def glwe_tensor_dot_relinearize_batched(self, res, a_ptrs, b_ptrs, tsk_pmat, tp, rp, batch, a_strides=None, b_strides=None):
        self.calls.append(("dot", res, list(a_ptrs), list(b_ptrs), tsk_pmat, tp, rp, batch, list(a_strides), list(b_strides)))

    def glwe_tensor_mul_relinearize_acc_batched(self, res, a, b, tsk_pmat, tp, rp, mode, batch, **kw):
        self.calls.append(("mul", res, a, b, tsk_pmat, mode, batch, kw))


def test_launch_order_and_arguments_on_a_recording_module():
    """an unaligned a side: three rescales (one pz_glwe_combine_batched per input, the one with shift 0 included) into 256-byte aligned scratch
    copies, then ONE dot call that reads the copies on the a side and the inputs in place on the b side; without the scratch, or with a
    wrong pair count, CKKSError before any launch.  The fallback: one _acc call per pair, un-normalized but for the last."""
    n, batch, cols = 8192, 3, 2
    a = [Ct(B, 5, 20, 29 if i == 1 else 40, cols, 0x1000 * (i + 1)) for i in range(3)]
    b = [Ct(B, 6, 20, 40, cols, 0x10000 * (i + 1)) for i in range(3)]                          # aligned, in larger containers
    dst = Ct(B, 5, 0, 0, cols, 0x900000)
    plan = ckks.plan_dot_product_ct(dst, a, b)
    assert plan.branch == "fast" and set(plan.rescales) == {"a"}
    offs, total = plan.scratch_offsets(batch, n)
    each = batch * cols * 5 * n * 8
    assert total == plan.scratch_bytes(batch, n) == 3 * each and [offs[("a", i)] for i in range(3)] == [0, each, 2 * each] and each % 256 == 0
    rec = _Recorder(n)
    with pytest.raises(ckks.CKKSError, match="bytes of scratch"):
        plan.launch(rec, dst, batch, a, b, tsk_ptr=0x77, tsk=(5, 1, 6, B))
    with pytest.raises(ckks.CKKSError, match="planned for 3 pairs"):
        plan.launch(rec, dst, batch, a[:2], b[:2], tsk_ptr=0x77, tsk=(5, 1, 6, B), tmp=0x4000000)
    assert rec.calls == [] and (dst.log_delta, dst.log_budget) == (0, 0)
    tmp = 0x4000000
    plan.launch(rec, dst, batch, a, b, tsk_ptr=0x77, tsk=(5, 1, 6, B), tmp=tmp)
    assert [c[0] for c in rec.calls] == ["combine"] * 3 + ["dot"]
    for i, c in enumerate(rec.calls[:3]):
        assert c[1:] == (tmp + i * each, cols, 5, B, [(a[i].data, 5, LSH, [11, 0, 11][i])], False, batch), i
    _, res, pa, pb, key, tp, rp, bt, sa, sb = rec.calls[3]
    assert (res, pa, pb, key, bt, sa, sb) == (dst.data, [tmp, tmp + each, tmp + 2 * each], [x.data for x in b], 0x77, batch, [5] * 3, [6] * 3)
    assert (tp.a_size, tp.b_size, tp.a_effective_k, tp.b_effective_k, tp.res_size, tp.cnv_offset, tp.ab_base2k) == (5, 5, 49, 60, 5, 60, B)
    assert (rp.a_size, rp.res_size, rp.dnum, rp.key_size, rp.rank, rp.rank_out) == (5, 5, 5, 6, 1, 1)
    assert (dst.log_delta, dst.log_budget) == (plan.log_delta, plan.log_budget) == (20, 9)
    # the fallback
    low = Ct(B, 5, 12, 40, cols, 0x50000)
    fb = ckks.plan_dot_product_ct(dst, a[:1] + [a[0], a[2]], [low, b[1], b[2]])
    assert fb.branch == "fallback"
    rec = _Recorder(n)
    d2 = Ct(B, 5, 0, 0, cols, 0x900000)
    fb.launch(rec, d2, batch, a[:1] + [a[0], a[2]], [low, b[1], b[2]], tsk_ptr=0x77, tsk=(5, 1, 6, B))
    assert [c[0] for c in rec.calls] == ["mul"] * 3
    assert [(c[7]["accumulate"], c[7]["normalize"]) for c in rec.calls] == [(False, False), (True, False), (True, True)]
    assert [(c[2], c[3]) for c in rec.calls] == [(a[0].data, low.data), (a[0].data, b[1].data), (a[2].data, b[2].data)]
    assert (d2.log_delta, d2.log_budget) == (fb.log_delta, fb.log_budget)
