"""The weighted sums of ciphertexts by constants restated from the CPU oracle's per-op calls, in the reference's own order:
poulpy-ckks src/leveled/delegates/composite.rs:290-308 (ckks_mul_add_pt_const_znx_into), :423-441 (ckks_mul_sub_pt_const_znx_into) and
:760-784 (ckks_dot_product_pt_const_znx, with accumulate_unnormalized :478-506).  Every step is the reference's: the product into a scratch
ciphertext of dst's layout (tests/plain_oracle.ckks_mul_pt_const_into), the three branches of ckks_add_assign_unsafe / ckks_sub_assign_unsafe
(leveled/default/add.rs:122-146, sub.rs:122-146) on tests/shift_oracle's GLWE primitives, and the closing glwe_normalize_assign.

`dst`, `a`, `ops[i]`: ckks.Ct with a VecZnx in .data; `cst`, `csts[i]`: ckks.Cst.  Results and metadata are written into `dst`.
pz_glwe_lincomb_const_batched must reproduce these digits; run_plan() runs a poulpy_amd.ckks.LincombPlan's own term list the same way."""
from __future__ import annotations

from poulpy_amd import ckks
from poulpy_amd.layouts import VecZnx
from tests import plain_oracle as po
from tests import shift_oracle as so


def _scratch(dst: ckks.Ct) -> ckks.Ct:
    """take_mul_tmp (composite.rs:31-41): a ciphertext of dst's layout with default metadata"""
    return ckks.Ct(dst.base2k, dst.size, 0, 0, dst.cols, VecZnx(dst.data.n, dst.cols, dst.size))


def ckks_mul_pt_const_into(ref, dst: ckks.Ct, a: ckks.Ct, cst: ckks.Cst):
    """leveled/default/mul.rs:342-374."""
    log_budget, log_delta, cnv_offset = ckks.get_mul_const_params(dst, a, cst)
    po.ckks_mul_pt_const_into(ref, cnv_offset, dst.data, dst.base2k, a.data, a.base2k, cst.re, cst.im)
    dst.log_budget, dst.log_delta = log_budget, log_delta


def ckks_add_assign_unsafe(ref, dst: ckks.Ct, a: ckks.Ct, sub=False):
    """add.rs:122-146 / sub.rs:122-146."""
    B = dst.base2k
    if dst.log_budget < a.log_budget:
        (so.glwe_lsh_sub if sub else so.glwe_lsh_add)(B, a.log_budget - dst.log_budget, dst.data, a.data)
    elif dst.log_budget > a.log_budget:
        so.glwe_lsh_assign(ref, B, dst.log_budget - a.log_budget, dst.data)
        (so.glwe_sub_assign if sub else so.glwe_add_assign)(ref, dst.data, a.data)
    else:
        (so.glwe_sub_assign if sub else so.glwe_add_assign)(ref, dst.data, a.data)
    dst.log_budget = min(dst.log_budget, a.log_budget)
    dst.log_delta = min(dst.log_delta, a.log_delta)


def ckks_mul_add_pt_const(ref, dst: ckks.Ct, a: ckks.Ct, cst: ckks.Cst, sub=False):
    """composite.rs:290-308 / :423-441: ckks_add_assign / ckks_sub_assign are the unsafe forms followed by glwe_normalize_assign."""
    if cst.empty:                                                   # :301-303
        return
    tmp = _scratch(dst)
    ckks_mul_pt_const_into(ref, tmp, a, cst)
    ckks_add_assign_unsafe(ref, dst, tmp, sub)
    so.glwe_normalize_assign(ref, dst.base2k, dst.data)


def ckks_dot_product_pt_const(ref, dst: ckks.Ct, ops, csts):
    """composite.rs:760-784."""
    n = len(ops)
    assert n >= 1 and n == len(csts) and n <= (1 << (63 - dst.base2k))
    ckks_mul_pt_const_into(ref, dst, ops[0], csts[0])
    if n <= 1:                                                      # accumulate_unnormalized, :492-494
        return
    tmp = _scratch(dst)
    for i in range(1, n):
        ckks_mul_pt_const_into(ref, tmp, ops[i], csts[i])
        ckks_add_assign_unsafe(ref, dst, tmp)
    so.glwe_normalize_assign(ref, dst.base2k, dst.data)


def run_plan(ref, plan: ckks.LincombPlan, dst: ckks.Ct, ops, csts):
    """The plan's own term list on the oracle's primitives: what pz_glwe_lincomb_const_batched is asked to compute."""
    B = dst.base2k
    have = plan.init_res
    for t in plan.terms:
        a, c = ops[t.index], csts[t.index]
        tmp = VecZnx(dst.data.n, dst.cols, dst.size)
        po.ckks_mul_pt_const_into(ref, t.cnv_offset, tmp, B, a.data, a.base2k, c.re, c.im)
        if not have:
            dst.data.data[...] = tmp.data
            have = True
            continue
        if t.join == ckks.LSH_TERM:
            (so.glwe_lsh_sub if t.sign < 0 else so.glwe_lsh_add)(B, t.k, dst.data, tmp)
            continue
        if t.join == ckks.LSH_ACC:
            so.glwe_lsh_assign(ref, B, t.k, dst.data)
        (so.glwe_sub_assign if t.sign < 0 else so.glwe_add_assign)(ref, dst.data, tmp)
    if plan.terms and plan.normalize:
        so.glwe_normalize_assign(ref, B, dst.data)
    plan.apply_meta(dst)
