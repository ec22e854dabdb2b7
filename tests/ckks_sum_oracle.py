"""The normalized sums of ciphertexts and the plaintext-vector composites of poulpy-ckks restated from the CPU oracle's per-op calls, in the
reference's own order:

* sum_chain: what pz_glwe_sum_batched is asked to compute (include/poulpy_hip.h) - the joins of ckks_add_assign_unsafe /
  ckks_sub_assign_unsafe (leveled/default/add.rs:122-146, sub.rs:122-146) applied term after term to a zero container on tests/shift_oracle's
  GLWE primitives, then glwe_normalize_assign.
* ckks_add_many (leveled/delegates/composite.rs:63-93), ckks_mul_pt_vec_znx_into / _assign (leveled/default/mul.rs:243-293, on
  tests/plain_oracle.glwe_mul_plain), ckks_mul_add_pt_vec_znx / ckks_mul_sub_pt_vec_znx (composite.rs:256-270, :389-403) and
  ckks_dot_product_pt_vec_znx (:705-729 with accumulate_unnormalized :478-506).
* run_sum_plan / run_dot_plan: a poulpy_amd.ckks.SumPlan's / DotPlan's own term list on the same primitives.

`dst`, `a`, `inputs[i]`: ckks.Ct with a VecZnx in .data; `pt`: ckks.Pt with a VecZnx(1 column) in .data.  Results and metadata are written
into `dst`."""
from __future__ import annotations

from poulpy_amd import ckks
from poulpy_amd.layouts import VecZnx
from tests import plain_oracle as po
from tests import shift_oracle as so


def join_term(ref, base2k, acc: VecZnx, a: VecZnx, join: int, k: int, sign: int):
    """one join of the chain into the running, un-normalized sum `acc`"""
    sub = sign < 0
    if join == ckks.LSH_TERM:
        (so.glwe_lsh_sub if sub else so.glwe_lsh_add)(base2k, k, acc, a)
        return
    if join == ckks.LSH_ACC:
        so.glwe_lsh_assign(ref, base2k, k, acc)
    else:
        assert k == 0
    (so.glwe_sub_assign if sub else so.glwe_add_assign)(ref, acc, a)


def sum_chain(ref, base2k, res: VecZnx, terms):
    """terms: (a: VecZnx, join, k, sign) in order; `a` may be `res` itself for term 0 (its content is read first).  Writes res."""
    acc = VecZnx(res.n, res.cols, res.size)
    for i, (a, join, k, sign) in enumerate(terms):
        if a is res:
            assert i == 0
            a = res.copy()
        join_term(ref, base2k, acc, a, join, k, sign)
    so.glwe_normalize_assign(ref, base2k, acc)
    res.data[...] = acc.data


def _scratch(dst: ckks.Ct) -> ckks.Ct:
    """take_mul_tmp (composite.rs:31-41): a ciphertext of dst's layout with default metadata"""
    return ckks.Ct(dst.base2k, dst.size, 0, 0, dst.cols, VecZnx(dst.data.n, dst.cols, dst.size))


def ckks_add_assign_unsafe(ref, dst: ckks.Ct, a: ckks.Ct, sub=False):
    """add.rs:122-146 / sub.rs:122-146."""
    join, k = ckks._join(dst.log_budget, a.log_budget)
    join_term(ref, dst.base2k, dst.data, a.data, join, k, -1 if sub else 1)
    dst.log_budget = min(dst.log_budget, a.log_budget)
    dst.log_delta = min(dst.log_delta, a.log_delta)


def ckks_add_many(ref, dst: ckks.Ct, inputs):
    """composite.rs:63-93."""
    B = dst.base2k
    if len(inputs) == 0:
        raise ckks.CKKSError("ckks_add_many: inputs must contain at least one ciphertext")
    if len(inputs) == 1:
        offset = ckks.offset_unary(dst, inputs[0])
        so.glwe_lsh(ref, B, offset, dst.data, inputs[0].data)
        dst.log_delta = inputs[0].log_delta
        dst.log_budget = ckks.checked_log_budget_sub("ckks_add_many", inputs[0].log_budget, offset)
        return
    assert len(inputs) <= (1 << (63 - B))
    op = ckks.plan_add_into(dst, inputs[0], inputs[1], normalize=False)
    so.run(ref, op, dst, inputs[0], inputs[1])          # ckks_add_into_unsafe, add.rs:76-104
    op.apply_meta(dst)
    for ct in inputs[2:]:
        ckks_add_assign_unsafe(ref, dst, ct)
    so.glwe_normalize_assign(ref, B, dst.data)


def get_mul_pt_params(res: ckks.Ct, a: ckks.Ct, b: ckks.Pt):
    """mul.rs:480-496 restated here, so that the restatement does not lean on the function under test (checked_mul_pt_log_budget,
    error.rs:177-194, and checked_log_budget_sub, :113-122, written out)"""
    if b.log_delta > a.log_budget:
        raise ckks.CKKSError("mul: multiplication precision underflow")
    res_log_budget = a.log_budget - b.log_delta
    res_log_delta = a.log_delta
    res_offset = max(res_log_budget + res_log_delta - res.size * res.base2k, 0)      # saturating_sub(res.max_k())
    cnv_offset = b.size * b.base2k + res_offset                                      # b.max_k() + res_offset
    if res_offset > res_log_budget:
        raise ckks.CKKSError("mul: insufficient homomorphic capacity")
    return res_log_budget - res_offset, res_log_delta, cnv_offset


def ckks_mul_pt_vec_znx_into(ref, dst: ckks.Ct, a: ckks.Ct, pt: ckks.Pt):
    """mul.rs:243-268; a is dst for the _assign form (:270-293)."""
    log_budget, log_delta, cnv_offset = get_mul_pt_params(dst, a, pt)
    if a is dst:
        po.glwe_mul_plain_assign(ref, cnv_offset, dst.data, dst.effective_k, pt.data, pt.max_k, dst.base2k)
    else:
        po.glwe_mul_plain(ref, cnv_offset, dst.data, dst.base2k, a.data, a.effective_k, pt.data, pt.max_k, a.base2k)
    dst.log_budget, dst.log_delta = log_budget, log_delta


def ckks_mul_add_pt_vec_znx(ref, dst: ckks.Ct, a: ckks.Ct, pt: ckks.Pt, sub=False):
    """composite.rs:256-270 / :389-403: the product into a scratch ciphertext, then ckks_add_assign / ckks_sub_assign (normalized)."""
    tmp = _scratch(dst)
    ckks_mul_pt_vec_znx_into(ref, tmp, a, pt)
    ckks_add_assign_unsafe(ref, dst, tmp, sub)
    so.glwe_normalize_assign(ref, dst.base2k, dst.data)


def ckks_dot_product_pt_vec_znx(ref, dst: ckks.Ct, ops, pts):
    """composite.rs:705-729."""
    n = len(ops)
    assert n >= 1 and n == len(pts) and n <= (1 << (63 - dst.base2k))
    ckks_mul_pt_vec_znx_into(ref, dst, ops[0], pts[0])
    if n <= 1:                                                      # accumulate_unnormalized, :492-494
        return
    tmp = _scratch(dst)
    for i in range(1, n):
        ckks_mul_pt_vec_znx_into(ref, tmp, ops[i], pts[i])
        ckks_add_assign_unsafe(ref, dst, tmp)
    so.glwe_normalize_assign(ref, dst.base2k, dst.data)


def run_sum_plan(ref, plan, dst: ckks.Ct, inputs):
    """A SumPlan's own term list: what its pz_glwe_sum_batched call is asked to compute."""
    if plan.normalize:
        sum_chain(ref, dst.base2k, dst.data, [(inputs[t.index].data, t.join, t.k, t.sign) for t in plan.terms])
    else:                                                           # n = 1: glwe_lsh
        (t,) = plan.terms
        so.glwe_lsh(ref, dst.base2k, t.k, dst.data, inputs[t.index].data)
    plan.apply_meta(dst)


def run_dot_plan(ref, plan, dst: ckks.Ct, ops, pts, slots=None):
    """A DotPlan's products (its own cnv_offsets) and joins, chunked by `slots` as DotPlan.launch chunks them."""
    B = dst.base2k
    prods = []
    for t in plan.terms:
        a, pt = ops[t.index], pts[t.index]
        tmp = VecZnx(dst.data.n, dst.cols, dst.size)
        po.glwe_mul_plain(ref, t.cnv_offset, tmp, B, a.data, a.effective_k, pt.data, pt.max_k, a.base2k)
        prods.append(tmp)
    if not plan.normalize:
        dst.data.data[...] = prods[0].data
    else:
        slots = slots or len(prods)
        for lo in range(0, len(prods), slots):
            terms = [(prods[i], plan.terms[i].join, plan.terms[i].k, plan.terms[i].sign) for i in range(lo, min(lo + slots, len(prods)))]
            if lo:
                terms.insert(0, (dst.data, ckks.PLAIN, 0, 1))
            sum_chain(ref, B, dst.data, terms)
    plan.apply_meta(dst)
