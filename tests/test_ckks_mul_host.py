"""CPU: the plans of the ciphertext products (poulpy_amd/ckks.py: mul_into / mul_assign / square_into / square_assign, mul_add_ct /
mul_sub_ct, mul_many, compact_limbs_copy) against the literal restatement of the reference (tests/ckks_mul_oracle.py); the entry point
pz_glwe_tensor_mul_relinearize_acc_batched in the header, the library and every binding; and one decrypted case under a real key with its
negative control.  (The device: tests/test_gpu_ckks_mul.py.)"""
import os
import re

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH_ACC, LSH_TERM, PLAIN, Ct
from poulpy_amd.layouts import VecZnx
from tests import ckks_mul_cases as cases
from tests import ckks_mul_oracle as mo
from tests import fhe_sk as fs
from tests.core_cases import prepare
from tests.helpers import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


def _meta(ct):
    return ct.log_delta, ct.log_budget


def test_entry_point_in_header_library_and_bindings():
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from poulpy_amd import abi, hal
    lib = hal.load_library()
    name, ws = "pz_glwe_tensor_mul_relinearize_acc_batched", "pz_glwe_tensor_mul_relinearize_acc_workspace_bytes"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poulpy_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % name, hdr) and re.search(r"\bsize_t %s\s*\(" % ws, hdr)
    assert hasattr(lib, name) and hasattr(lib, ws) and name in abi.PROTOTYPES and ws in abi.PROTOTYPES
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == 16 and getattr(lib, ws).restype is C.c_size_t
    assert fn.argtypes[5] is C.POINTER(hal.GlweTensorParams) and fn.argtypes[6] is C.POINTER(hal.GlweOpParams)
    assert [fn.argtypes[i] for i in (7, 8, 11, 15)] == [C.c_size_t] * 4 and [fn.argtypes[i] for i in (9, 10, 12, 13, 14)] == [C.c_int] * 5
    assert callable(hal.Module.glwe_tensor_mul_relinearize_acc_batched) and callable(hal.Module.glwe_tensor_mul_relinearize_acc_workspace_bytes)
    assert fn(None, None, None, None, None, None, None, 0, 0, 0, 0, 0, 1, 1, 0, 1) == abi.PZ_ERR_INVALID and b"null module" in lib.pz_last_error()
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "ffi.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")).read()
    assert name + "(m_," in mirror and ws + "(m_," in mirror and "fn %s(" % name in ffi and "fn %s(" % ws in ffi and "ffi::%s(" % name in rust
    # the header states the alias rule, the staging decision and where the product of a wave lives
    doc = open(os.path.join(ROOT, "include", "poulpy_hip.h")).read()
    block = doc[doc.index("The same product on operands that sit in larger containers"):doc.index("size_t " + ws)]
    for word in ("a_stride", "PZ_ERR_ALIAS", "nothing is staged", "workspace", "never to caller memory", "Nothing is launched on a refusal"):
        assert word in block, word


# ---- metadata and refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [12, 17])
def test_metadata_of_every_operation_on_the_reference_cases(B):
    """log_delta, log_budget and cnv_offset of every form on mul.rs / mul_add.rs / mul_sub.rs / composition.rs's cases, against
    get_mul_ct_params restated in tests/ckks_mul_oracle.py; sizes and strides from the containers"""
    for label, dsize, a, b in cases.mul_scenarios(B):
        dst = Ct(B, dsize, 0, 0)
        for name, plan, x, y, res in (("mul_into", ckks.plan_mul_into(dst, a, b), a, b, dst),
                                      ("mul_assign", ckks.plan_mul_assign(a, b), a, b, a),
                                      ("square_into", ckks.plan_square_into(dst, a), a, a, dst),
                                      ("square_assign", ckks.plan_square_assign(a), a, a, a)):
            budget, delta, cnv = mo.get_mul_ct_params(res, x, y)
            assert (plan.log_budget, plan.log_delta, plan.cnv_offset) == (budget, delta, cnv), (label, name)
            assert cnv == max(x.effective_k, y.effective_k) + max(min(x.log_budget, y.log_budget) - max(x.log_delta, y.log_delta)
                                                                   + min(x.log_delta, y.log_delta) - res.max_k, 0), (label, name)
            assert (plan.a_size, plan.b_size) == (-(-x.effective_k // B), -(-y.effective_k // B)) and (plan.a_stride, plan.b_stride) == (x.size, y.size)
            assert plan.tensor_size == max(x.size, y.size) and plan.square == name.startswith("square") and plan.join is None
        for sub in (False, True):
            for d_budget in (0, 11, 40):
                d = Ct(B, dsize, cases.D, d_budget)
                plan = ckks.plan_mul_add_ct(d, a, b, sub=sub)
                tmp = Ct(B, dsize, 0, 0)
                budget, delta, cnv = mo.get_mul_ct_params(tmp, a, b)
                assert (plan.prod_log_budget, plan.prod_log_delta, plan.cnv_offset) == (budget, delta, cnv), (label, sub)
                want_join = (LSH_TERM, budget - d_budget) if d_budget < budget else (LSH_ACC, d_budget - budget) if d_budget > budget else (PLAIN, 0)
                assert (plan.join, plan.k, plan.sign) == (*want_join, -1 if sub else 1), (label, sub, d_budget)
                assert (plan.log_delta, plan.log_budget) == (min(cases.D, delta), min(d_budget, budget))
    # the aligned case in numbers: 5 limbs of 12 bits, log_delta 20
    p = ckks.plan_mul_into(Ct(12, 5, 0, 0), cases.fresh(12, 60), cases.fresh(12, 60))
    assert (p.log_delta, p.log_budget, p.cnv_offset) == (20, 20, 60)
    p = ckks.plan_mul_into(Ct(12, 3, 0, 0), cases.fresh(12, 60), cases.fresh(12, 60))       # smaller output: res_offset 4
    assert (p.log_delta, p.log_budget, p.cnv_offset) == (20, 16, 64)


def test_refusals_carry_the_variant():
    B = 12
    full = cases.fresh(B, 60)
    with pytest.raises(ckks.CKKSError, match="multiplication precision underflow"):         # min budget 10 < max log_delta 20
        ckks.plan_mul_into(Ct(B, 5, 0, 0), full, Ct(B, 5, 20, 10))
    with pytest.raises(ckks.CKKSError, match="multiplication precision underflow"):
        ckks.plan_square_assign(Ct(B, 5, 20, 19))
    with pytest.raises(ckks.CKKSError, match="insufficient homomorphic capacity"):           # res_offset 28 > res_log_budget 20
        ckks.plan_mul_into(Ct(B, 1, 0, 0), full, full)
    with pytest.raises(ckks.CKKSError, match="insufficient homomorphic capacity"):
        ckks.plan_mul_add_ct(Ct(B, 1, 20, 5), full, full)
    with pytest.raises(ckks.CKKSError, match="insufficient homomorphic capacity"):
        ckks.plan_mul_many(Ct(B, 1, 0, 0), [full])
    with pytest.raises(ckks.CKKSError, match="smaller than effective_k"):
        ckks.plan_mul_into(Ct(B, 5, 0, 0), Ct(B, 4, 20, 40), full)
    with pytest.raises(ckks.CKKSError, match="same log_delta"):
        ckks.plan_mul_many(Ct(B, 5, 0, 0), [full, Ct(B, 5, 19, 41), full])
    with pytest.raises(ckks.CKKSError, match="at least one ciphertext"):
        ckks.plan_mul_many(Ct(B, 5, 0, 0), [])
    with pytest.raises(ckks.CKKSError, match="base2k"):
        ckks.plan_mul_into(Ct(B, 5, 0, 0), full, cases.fresh(17, 68))
    with pytest.raises(ckks.CKKSError, match="multiplication precision underflow"):         # three levels of 20 bits out of a budget of 40
        ckks.plan_mul_many(Ct(B, 5, 0, 0), [full] * 5)
    with pytest.raises(ckks.CKKSError, match="rounds up to 4"):
        ckks.plan_compact_limbs_copy(Ct(B, 5, 0, 0), Ct(B, 6, 20, 25))
    assert ckks.plan_compact_limbs_copy(Ct(B, 4, 0, 0), Ct(B, 6, 20, 25)).size == 4


# ---- the plans against the literal restatement ------------------------------------------------------------------------------------------------
def _key(ref, rng, B, rank, limbs):
    mat = cases.random_tensor_key(rng, N, B, rank, limbs, limbs + 1)
    pm = ref.vmp_pmat_alloc(limbs, rank * (rank + 1) // 2, rank + 1, limbs + 1)
    ref.vmp_prepare(pm, mat)
    return mo.Tsk(pm, 1, B)


def _copy(ct: Ct) -> Ct:
    return Ct(ct.base2k, ct.size, ct.log_delta, ct.log_budget, ct.cols, ct.data.copy())


@pytest.mark.parametrize("rank", [1, 2])
def test_product_plans_reproduce_the_literal_restatement(ref, rank):
    """every form on every scenario at N = 64: the plan's own numbers on the oracle == ckks_mul_into / _assign / square / mul_add / mul_sub
    written out, limbs and metadata"""
    B, limbs, cols = 12, 5, rank + 1
    rng = seeded(40 + rank)
    tsk = _key(ref, rng, B, rank, limbs)
    for label, dsize, a, b in cases.mul_scenarios(B, cols, limbs):
        ha, hb = cases.fill_ct(rng, N, a), cases.fill_ct(rng, N, b)
        for name in ("mul_into", "mul_assign", "square_into", "square_assign", "mul_add_ct", "mul_sub_ct"):
            if name.endswith("assign"):
                d1 = _copy(ha)
            elif name.startswith("mul_a") or name.startswith("mul_s"):
                d1 = cases.fill_ct(rng, N, Ct(B, dsize, cases.D, 11, cols), normalized=False)
            else:
                d1 = Ct(B, dsize, 0, 0, cols, VecZnx(N, cols, dsize))
            d2 = _copy(d1)
            if name == "mul_into":
                plan = ckks.plan_mul_into(d1, ha, hb)
                mo.run_mul_plan(ref, plan, d1, ha, hb, tsk)
                mo.ckks_mul_into(ref, d2, ha, hb, tsk)
            elif name == "mul_assign":
                plan = ckks.plan_mul_assign(d1, hb)
                mo.run_mul_plan(ref, plan, d1, hb, None, tsk)
                mo.ckks_mul_into(ref, d2, d2, hb, tsk)
            elif name == "square_into":
                plan = ckks.plan_square_into(d1, ha)
                mo.run_mul_plan(ref, plan, d1, ha, None, tsk)
                mo.ckks_mul_into(ref, d2, ha, None, tsk)
            elif name == "square_assign":
                plan = ckks.plan_square_assign(d1)
                mo.run_mul_plan(ref, plan, d1, None, None, tsk)
                mo.ckks_mul_into(ref, d2, d2, None, tsk)
            else:
                sub = name == "mul_sub_ct"
                plan = ckks.plan_mul_add_ct(d1, ha, hb, sub=sub)
                mo.run_mul_plan(ref, plan, d1, ha, hb, tsk)
                mo.ckks_mul_add_ct_into(ref, d2, ha, hb, tsk, sub=sub)
            assert np.array_equal(d1.data.data, d2.data.data), (label, name)
            assert _meta(d1) == _meta(d2), (label, name)
            assert np.any(d1.data.data), (label, name)


@pytest.mark.parametrize("rank", [1, 2])
def test_mul_many_nodes_equal_the_literal_recursion(ref, rank):
    """the reference's five cases and n = 1 .. 9 with one input at a lower budget: the plan's nodes, in order, carry the layouts and metadata
    the recursion produces in its evaluation order; run on the oracle (each slot checked never to be live twice) they leave the recursion's
    limbs"""
    B, cols = 12, rank + 1
    rng = seeded(50 + rank)
    tsk = _key(ref, rng, B, rank, 10)
    for label, dsize, inputs in cases.mul_many_scenarios(B, cols):
        hin = [cases.fill_ct(rng, N, x) for x in inputs]
        plan = ckks.plan_mul_many(Ct(B, dsize, 0, 0, cols), hin)
        d1 = Ct(B, dsize, 0, 0, cols, VecZnx(N, cols, dsize))
        d2 = _copy(d1)
        trace = []
        mo.ckks_mul_many(ref, d2, hin, tsk, trace)
        assert [(nd.op == "lsh", (nd.ct.size, nd.ct.log_delta, nd.ct.log_budget)) for nd in plan.nodes] == [(cnt == 1, m) for cnt, m in trace], label
        assert plan.nodes[-1].out == "dst" and all(nd.out != "dst" for nd in plan.nodes[:-1]), label
        mo.run_mul_many_plan(ref, plan, d1, hin, tsk)
        assert np.array_equal(d1.data.data, d2.data.data) and _meta(d1) == _meta(d2) == (plan.log_delta, plan.log_budget), label
        # the scratch: every slot 256-byte aligned, none overlapping, the total what the offsets say
        offs, total = plan.slot_offsets(3, N)
        assert plan.scratch_bytes(3, N) == total and all(o % 256 == 0 for o in offs)
        ends = [o + 3 * cols * limbs * N * 8 for o, limbs in zip(offs, plan.slot_limbs)]
        assert all(e <= o2 for e, o2 in zip(ends, offs[1:] + [total])), label
        if len(inputs) <= 2:
            assert total == 0
    # where an operand holds fewer effective limbs than its container (an input rescaled by more than a limb), the node passes stride and
    # size apart
    plan = ckks.plan_mul_many(Ct(B, 10, 0, 0, cols), [Ct(B, 10, cases.D, 120 - cases.D - (15 if i == 1 else 0), cols) for i in range(4)])
    assert any(nd.mul and (nd.mul.a_size < nd.mul.a_stride or nd.mul.b_size < nd.mul.b_stride) for nd in plan.nodes)


# ---- one decrypted case ----------------------------------------------------------------------------------------------------------------------------
def test_mul_add_and_mul_many_decrypt_to_the_exact_products_with_a_control(ref):
    """dst + a b and a b c d at N = 64 under a real tensor key: the exact integer products within reference_bound at the product's cnv_offset
    and within an eighth of the unit they are counted in (tests/ckks_mul_cases.py); with the join's k off by one the same case misses."""
    c = cases.decrypt_case(N, 1, 60, s=19)
    tsk = mo.Tsk(prepare(ref, c.key), 1, c.B)
    E, s, size, cols, Bk = c.E, c.s, c.size, c.cols, c.B
    a, b = cases.ct_of(c, 0), cases.ct_of(c, 1)
    # a b stands at 2^-(E - 2 s); dst holds md in that unit at 5 bits of budget above the product's
    bits = E - 2 * s
    prod_budget = E - 2 * cases.D
    md = cases._ternary(N, c.rng)
    want = fs.mul_msg(c.ms[0], c.ms[1]) + md

    def fresh_dst():
        d = Ct(Bk, size, cases.D, prod_budget + 5, cols)
        ed = d.effective_k
        d.data = VecZnx(N, cols, size, np.ascontiguousarray(fs.glwe_encrypt(c.sk, fs.encode(md << (ed - bits - 5), Bk, ed, size), Bk, E, seeded(61))))
        return d
    dst = fresh_dst()
    plan = ckks.plan_mul_add_ct(dst, a, b)
    assert (plan.join, plan.k) == (LSH_ACC, 5)
    mo.run_mul_plan(ref, plan, dst, a, b, tsk)
    lit = fresh_dst()
    mo.ckks_mul_add_ct_into(ref, lit, a, b, tsk)
    assert np.array_equal(dst.data.data, lit.data.data) and _meta(dst) == _meta(lit) == (cases.D, prod_budget)
    cases.check_decrypt("dst + a b", c, dst.data.data, want, bits, plan.cnv_offset)
    # negative control: the same case with the join's k off by one
    for k_off in (-1, 1):
        bad = fresh_dst()
        plan.k += k_off
        mo.run_mul_plan(ref, plan, bad, a, b, tsk)
        plan.k -= k_off
        cases.check_decrypt(f"dst + a b, join k {k_off:+d}", c, bad.data.data, want, bits, plan.cnv_offset, fail=True)
    # a b c d: two levels; the product of the halves stands at 2^-(E - D - 4 s) ... in the halves' unit 2^-(E - 2 s) twice, times 2^(E - D)
    ins = [cases.ct_of(c, i) for i in range(4)]
    d4 = Ct(Bk, size, 0, 0, cols, VecZnx(N, cols, size))
    p4 = ckks.plan_mul_many(d4, ins)
    mo.run_mul_many_plan(ref, p4, d4, ins, tsk)
    l4 = Ct(Bk, size, 0, 0, cols, VecZnx(N, cols, size))
    mo.ckks_mul_many(ref, l4, ins, tsk)
    assert np.array_equal(d4.data.data, l4.data.data) and _meta(d4) == _meta(l4)
    want4 = fs.mul_msg(fs.mul_msg(c.ms[0], c.ms[1]), fs.mul_msg(c.ms[2], c.ms[3]))
    top = p4.nodes[-1].mul
    bits4 = 2 * bits - top.cnv_offset
    assert bits4 > 0
    cases.check_decrypt("a b c d", c, d4.data.data, want4, bits4, top.cnv_offset)
