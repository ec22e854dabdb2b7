"""The products of two ciphertexts of poulpy-ckks restated from the CPU oracle's per-op calls, in the reference's own order:

* ckks_mul_into / _assign, ckks_square_into / _assign (leveled/default/mul.rs:47-200) on ref.glwe_tensor_apply / glwe_tensor_square_apply /
  glwe_tensor_relinearize, with get_mul_ct_params (:461-478), checked_mul_ct_log_budget (error.rs:155-175) and checked_log_budget_sub
  (:113-122) written out here, so that the restatement does not lean on the functions under test;
* ckks_mul_add_ct_into / ckks_mul_sub_ct_into (leveled/delegates/composite.rs:239-254, :372-387) with the joins of tests/ckks_sum_oracle.py;
* ckks_mul_many (composite.rs:103-198): the recursion itself, with scratch ciphertexts allocated as it goes - not a plan's node list;
* run_mul_plan / run_mul_many_plan: a poulpy_amd.ckks.MulPlan's / MulManyPlan's own numbers on the same primitives - what its device calls
  are asked to compute.

glwe_tensor_apply asserts size == effective_k.div_ceil(base2k) (poulpy-core operations/glwe.rs:722-723); an operand whose container holds
more limbs is read through `compact` (the reference reallocates there: ckks_compact_limbs, layouts/ciphertext.rs:216-232).

`dst`, `a`, `b`, `inputs[i]`: ckks.Ct with a VecZnx in .data; tsk: Tsk(pmat, dsize, base2k), the oracle's prepared tensor key.  Results and
metadata are written into `dst`."""
from __future__ import annotations

from collections import namedtuple

from poulpy_amd import ckks
from poulpy_amd.layouts import VecZnx
from tests import ckks_sum_oracle as so_sum
from tests import shift_oracle as so

Tsk = namedtuple("Tsk", "pmat dsize base2k")


def div_ceil(a: int, b: int) -> int:
    return -(-a // b)


def get_mul_ct_params(res: ckks.Ct, a: ckks.Ct, b: ckks.Ct):
    """mul.rs:461-478 -> (res_log_budget, res_log_delta, cnv_offset)"""
    if max(a.log_delta, b.log_delta) > min(a.log_budget, b.log_budget):             # checked_mul_ct_log_budget
        raise ckks.CKKSError("mul: multiplication precision underflow")
    res_log_budget = min(a.log_budget, b.log_budget) - max(a.log_delta, b.log_delta)
    res_log_delta = min(a.log_delta, b.log_delta)
    res_offset = max(res_log_budget + res_log_delta - res.size * res.base2k, 0)      # saturating_sub(res.max_k())
    cnv_offset = max(a.log_delta + a.log_budget, b.log_delta + b.log_budget) + res_offset
    if res_offset > res_log_budget:                                                  # checked_log_budget_sub
        raise ckks.CKKSError("mul: insufficient homomorphic capacity")
    return res_log_budget - res_offset, res_log_delta, cnv_offset


def compact(x: VecZnx, size: int) -> VecZnx:
    """the first `size` limbs of x as a container of their own"""
    assert 1 <= size <= x.size
    return VecZnx(x.n, x.cols, size, x.data[:size].copy())


def product(ref, cnv_offset, out: VecZnx, base2k, a: VecZnx, a_effective_k, b, b_effective_k, tensor_size, tsk: Tsk):
    """glwe_tensor_apply (b None: glwe_tensor_square_apply) into a scratch tensor of tensor_size limbs, glwe_tensor_relinearize into out"""
    cols = out.cols
    tmp = VecZnx(out.n, cols * (cols + 1) // 2, tensor_size)
    if b is None:
        ref.glwe_tensor_square_apply(cnv_offset, tmp, base2k, a, a_effective_k, base2k)
    else:
        ref.glwe_tensor_apply(cnv_offset, tmp, base2k, a, a_effective_k, b, b_effective_k, base2k)
    ref.glwe_tensor_relinearize(out, base2k, tmp, base2k, tsk.pmat, tsk.dsize, tsk.base2k)


def ckks_mul_into(ref, dst: ckks.Ct, a: ckks.Ct, b: ckks.Ct | None, tsk: Tsk):
    """mul.rs:47-84; a is dst: ckks_mul_assign (:86-122); b None: ckks_square_into (:145-172), and with a is dst ckks_square_assign
    (:174-200).  The tensor layout has k = max(a.max_k, b.max_k)."""
    B = dst.base2k
    y = a if b is None else b
    log_budget, log_delta, cnv_offset = get_mul_ct_params(dst, a, y)
    tensor_size = div_ceil(max(a.size * B, y.size * B), B)
    av = compact(a.data, div_ceil(a.effective_k, B))
    bv = None if b is None else compact(b.data, div_ceil(b.effective_k, B))
    out = VecZnx(dst.data.n, dst.cols, dst.size)
    product(ref, cnv_offset, out, B, av, a.effective_k, bv, y.effective_k, tensor_size, tsk)
    dst.data.data[...] = out.data
    dst.log_budget, dst.log_delta = log_budget, log_delta


def ckks_mul_add_ct_into(ref, dst: ckks.Ct, a: ckks.Ct, b: ckks.Ct, tsk: Tsk, sub=False):
    """composite.rs:239-254 / :372-387: ckks_mul_into on take_mul_tmp(dst), then ckks_add_assign / ckks_sub_assign (= the _unsafe form
    followed by glwe_normalize_assign, add.rs:107-120)"""
    tmp = so_sum._scratch(dst)
    ckks_mul_into(ref, tmp, a, b, tsk)
    so_sum.ckks_add_assign_unsafe(ref, dst, tmp, sub)
    so.glwe_normalize_assign(ref, dst.base2k, dst.data)


def ceil_log2(n: int) -> int:
    """composite.rs:98-101"""
    return 0 if n <= 1 else (n - 1).bit_length()


def ckks_mul_many(ref, dst: ckks.Ct, inputs, tsk: Tsk, trace=None):
    """composite.rs:103-198, mul_many_rec.  trace: a list that receives (number of inputs, the result's (size, log_delta, log_budget)) of
    every call of the recursion as it returns - the reference's evaluation order."""
    if len(inputs) == 0:
        raise ckks.CKKSError("ckks_mul_many: inputs must contain at least one ciphertext")
    if any(c.log_delta != inputs[0].log_delta for c in inputs):
        raise ckks.CKKSError("ckks_mul_many: all inputs must have the same log_delta")
    B = dst.base2k
    if len(inputs) == 1:
        offset = max(inputs[0].effective_k - dst.size * B, 0)                        # offset_unary
        so.glwe_lsh(ref, B, offset, dst.data, inputs[0].data)
        if offset > inputs[0].log_budget:
            raise ckks.CKKSError("ckks_mul_many: insufficient homomorphic capacity")
        dst.log_delta, dst.log_budget = inputs[0].log_delta, inputs[0].log_budget - offset
    elif len(inputs) == 2:
        ckks_mul_into(ref, dst, inputs[0], inputs[1], tsk)
    else:
        mid = len(inputs) // 2
        halves = []
        for part in (inputs[:mid], inputs[mid:]):
            k = max(min(c.effective_k for c in part) - ceil_log2(len(part)) * inputs[0].log_delta, 0)
            size = div_ceil(k, B)
            halves.append(ckks.Ct(B, size, 0, 0, dst.cols, VecZnx(dst.data.n, dst.cols, size)))
        ckks_mul_many(ref, halves[0], inputs[:mid], tsk, trace)
        ckks_mul_many(ref, halves[1], inputs[mid:], tsk, trace)
        ckks_mul_into(ref, dst, halves[0], halves[1], tsk)
    if trace is not None:
        trace.append((len(inputs), (dst.size, dst.log_delta, dst.log_budget)))


# ---- a plan's own numbers on the oracle ---------------------------------------------------------------------------------------------------
def plan_product(ref, p, out: VecZnx, base2k, a: VecZnx, b, tsk: Tsk):
    """what one pz_glwe_tensor_mul_relinearize_acc_batched of MulPlan p computes before any join: the operands are the first a_size /
    b_size limbs of containers of a_stride / b_stride limbs"""
    assert a.size == p.a_stride and (b is None or b.size == p.b_stride)
    product(ref, p.cnv_offset, out, base2k, compact(a, p.a_size), p.a_effective_k, None if b is None else compact(b, p.b_size), p.b_effective_k,
            p.tensor_size, tsk)


def join(ref, base2k, res: VecZnx, prod: VecZnx, kind: int, k: int, sign: int, normalize: bool):
    """accumulate = 1 of the entry point: res = join(res, product), then glwe_normalize_assign when asked"""
    so_sum.join_term(ref, base2k, res, prod, kind, k, sign)
    if normalize:
        so.glwe_normalize_assign(ref, base2k, res)


def run_mul_plan(ref, plan, dst: ckks.Ct, a: ckks.Ct | None, b: ckks.Ct | None, tsk: Tsk):
    """A MulPlan's call on the oracle; the operands named "dst" in plan.which are dst itself."""
    ops = {"a": a, "b": b, "dst": dst, None: None}
    x, y = ops[plan.which[0]], ops[plan.which[1]]
    out = VecZnx(dst.data.n, dst.cols, dst.size)
    plan_product(ref, plan, out, dst.base2k, x.data, None if y is None else y.data, tsk)
    if plan.join is None:
        dst.data.data[...] = out.data
    else:
        join(ref, dst.base2k, dst.data, out, plan.join, plan.k, plan.sign, True)
    plan.apply_meta(dst)


def run_mul_many_plan(ref, plan, dst: ckks.Ct, inputs, tsk: Tsk):
    """A MulManyPlan's nodes in order, each slot a container of its own; asserts that no slot is written while it is still to be read."""
    slots, unread = {}, set()

    def vec(r):
        return dst.data if r == "dst" else inputs[r[1]].data if r[0] == "in" else slots[r[1]]
    for nd in plan.nodes:
        out = VecZnx(dst.data.n, nd.ct.cols, nd.ct.size)
        if nd.op == "lsh":
            so.glwe_lsh(ref, nd.ct.base2k, nd.shift, out, vec(nd.a))
        else:
            plan_product(ref, nd.mul, out, nd.ct.base2k, vec(nd.a), vec(nd.b), tsk)
            for r in (nd.a, nd.b):
                if r[0] == "slot":
                    unread.discard(r[1])
        if nd.out == "dst":
            dst.data.data[...] = out.data
        else:
            assert nd.out[1] not in unread, ("slot live twice", nd.out)
            assert plan.slot_limbs[nd.out[1]] == nd.ct.size
            slots[nd.out[1]] = out
            unread.add(nd.out[1])
    assert not unread
    plan.apply_meta(dst)
