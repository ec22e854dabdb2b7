"""ckks_dot_product_ct of poulpy-ckks (leveled/delegates/composite.rs:563-703) restated from the CPU oracle's per-op calls, in the reference's
own order and with scratch allocated where the reference takes it - written from the Rust text, not from poulpy_amd.ckks's plan:

* check_lengths (:468-476), ensure_accumulation_fits (:43-51), n = 1 -> ckks_mul_into;
* non-uniform log_delta: ckks_mul_into(dst, a0, b0), then accumulate_unnormalized (:478-506) - ckks_mul_into into a scratch ciphertext of dst's
  layout, ckks_add_assign_unsafe, for every further pair - and the closing glwe_normalize_assign;
* otherwise: on an unaligned side ckks_rescale_into (rescale.rs:39-55: glwe_lsh) of EVERY input into scratch ciphertexts of the target
  effective_k, glwe_tensor_apply on pair 0, glwe_tensor_apply_add_assign on the others - one accumulated GLWETensor - and one
  glwe_tensor_relinearize.

glwe_tensor_apply asserts size == effective_k.div_ceil(base2k) (poulpy-core operations/glwe.rs:722-723); an aligned operand whose container
holds more limbs is read through ckks_mul_oracle.compact (the reference reallocates there: ckks_compact_limbs).

run_dot_plan: a poulpy_amd.ckks.DotCtPlan's own numbers on the same primitives - what its device calls are asked to compute.
accumulated_tensor: the oracle's i64 GLWETensor of a fast-branch call (the tests look at its digits).

`dst`, `a_list[i]`, `b_list[i]`: ckks.Ct with a VecZnx in .data; tsk: ckks_mul_oracle.Tsk.  Results and metadata are written into `dst`."""
from __future__ import annotations

from poulpy_amd import ckks
from poulpy_amd.layouts import VecZnx
from tests import ckks_mul_oracle as mo
from tests import ckks_sum_oracle as so_sum
from tests import shift_oracle as so


def div_ceil(a: int, b: int) -> int:
    return -(-a // b)


def accumulated_tensor(ref, cnv_offset, base2k, n, cols, tensor_size, pairs, a_effective_k, b_effective_k) -> VecZnx:
    """glwe_tensor_apply on pairs[0], glwe_tensor_apply_add_assign on the rest (composite.rs:675-697); pairs: (a: VecZnx, b: VecZnx) of
    exactly the operands' limbs"""
    acc = VecZnx(n, cols * (cols + 1) // 2, tensor_size)
    for i, (a, b) in enumerate(pairs):
        ref.glwe_tensor_apply(cnv_offset, acc, base2k, a, a_effective_k, b, b_effective_k, base2k, add_assign=i > 0)
    return acc


def ckks_dot_product_ct(ref, dst: ckks.Ct, a_list, b_list, tsk: mo.Tsk):
    """composite.rs:563-703."""
    op = "ckks_dot_product_ct"
    if len(a_list) == 0:                                                             # check_lengths
        raise ckks.CKKSError(f"{op}: inputs must contain at least one pair")
    if len(a_list) != len(b_list):
        raise ckks.CKKSError(f"{op}: length mismatch between ct vector ({len(a_list)}) and weight vector ({len(b_list)})")
    n, B = len(a_list), dst.base2k
    if B >= 64 or n > (1 << (63 - B)):                                               # ensure_accumulation_fits
        raise ckks.CKKSError(f"{op}: {n} terms risks i64 overflow at base2k={B}")
    if n == 1:
        return mo.ckks_mul_into(ref, dst, a_list[0], b_list[0], tsk)
    a_min_lhr = min(c.log_budget for c in a_list)
    b_min_lhr = min(c.log_budget for c in b_list)
    a_aligned = all(c.log_budget == a_min_lhr and c.log_delta == a_list[0].log_delta for c in a_list)
    b_aligned = all(c.log_budget == b_min_lhr and c.log_delta == b_list[0].log_delta for c in b_list)
    uniform_ld = all(c.log_delta == a_list[0].log_delta for c in a_list) and all(c.log_delta == b_list[0].log_delta for c in b_list)
    if not uniform_ld:
        mo.ckks_mul_into(ref, dst, a_list[0], b_list[0], tsk)
        tmp = so_sum._scratch(dst)                                                   # accumulate_unnormalized: one scratch ciphertext, reused
        for i in range(1, n):
            mo.ckks_mul_into(ref, tmp, a_list[i], b_list[i], tsk)
            so_sum.ckks_add_assign_unsafe(ref, dst, tmp)
        so.glwe_normalize_assign(ref, B, dst.data)
        return
    a_ld, b_ld = a_list[0].log_delta, b_list[0].log_delta
    a_target_eff_k, b_target_eff_k = a_min_lhr + a_ld, b_min_lhr + b_ld
    N, cols = dst.data.n, dst.cols

    def side(aligned, xs, min_lhr, target_eff_k):
        """the operands glwe_tensor_apply reads: the inputs themselves, or their rescaled copies in take_glwe_slice(n, layout of target_eff_k)"""
        if aligned:
            return [mo.compact(x.data, div_ceil(target_eff_k, B)) for x in xs]
        out = []
        for x in xs:
            shift = x.log_budget - min_lhr
            if shift > x.log_budget:                                                 # checked_log_budget_sub("rescale", ..)
                raise ckks.CKKSError("rescale: insufficient homomorphic capacity")
            buf = VecZnx(N, cols, div_ceil(target_eff_k, B))
            so.glwe_lsh(ref, B, shift, buf, x.data)
            out.append(buf)
        return out
    a_ops = side(a_aligned, a_list, a_min_lhr, a_target_eff_k)
    b_ops = side(b_aligned, b_list, b_min_lhr, b_target_eff_k)
    res_log_delta = min(a_ld, b_ld)
    if max(a_ld, b_ld) > min(a_min_lhr, b_min_lhr):                                  # checked_mul_ct_log_budget
        raise ckks.CKKSError("dot_product_ct: multiplication precision underflow")
    lhr0 = min(a_min_lhr, b_min_lhr) - max(a_ld, b_ld)
    res_offset = max(lhr0 + res_log_delta - dst.size * B, 0)
    if res_offset > lhr0:                                                            # checked_log_budget_sub
        raise ckks.CKKSError("dot_product_ct: insufficient homomorphic capacity")
    res_log_budget = lhr0 - res_offset
    cnv_offset = max(a_target_eff_k, b_target_eff_k) + res_offset
    tensor_size = div_ceil(max(a_target_eff_k, b_target_eff_k), B)
    acc = accumulated_tensor(ref, cnv_offset, B, N, cols, tensor_size, list(zip(a_ops, b_ops)), a_target_eff_k, b_target_eff_k)
    out = VecZnx(N, cols, dst.size)
    ref.glwe_tensor_relinearize(out, B, acc, B, tsk.pmat, tsk.dsize, tsk.base2k)
    dst.data.data[...] = out.data
    dst.log_budget, dst.log_delta = res_log_budget, res_log_delta


# ---- a plan's own numbers on the oracle ---------------------------------------------------------------------------------------------------
def plan_operands(ref, plan, a_list, b_list):
    """the containers the fast branch's device call reads, per side: the inputs, or what the plan's rescales leave in scratch"""
    out = {}
    for side, xs, limbs in (("a", a_list, plan.a_size), ("b", b_list, plan.b_size)):
        if side not in plan.rescales:
            out[side] = [x.data for x in xs]
            continue
        out[side] = []
        for x, rs in zip(xs, plan.rescales[side]):
            tmp = ckks.Ct(plan.base2k, limbs, 0, 0, plan.cols, VecZnx(x.data.n, plan.cols, limbs))
            so.run(ref, rs, tmp, x)
            out[side].append(tmp.data)
    return out


def run_dot_plan(ref, plan, dst: ckks.Ct, a_list, b_list, tsk: mo.Tsk):
    """A DotCtPlan's calls on the oracle.  single / fallback: every MulPlan through ckks_mul_oracle's product and join, normalize only on the
    last one; fast: the rescales, then what ONE pz_glwe_tensor_dot_relinearize_batched computes."""
    B = dst.base2k
    if plan.branch != "fast":
        for i, p in enumerate(plan.muls):
            out = VecZnx(dst.data.n, dst.cols, dst.size)
            mo.plan_product(ref, p, out, B, a_list[i].data, b_list[i].data, tsk)
            if p.join is None:
                dst.data.data[...] = out.data
            else:
                mo.join(ref, B, dst.data, out, p.join, p.k, p.sign, i == len(plan.muls) - 1)
        plan.apply_meta(dst)
        return
    ops = plan_operands(ref, plan, a_list, b_list)
    pairs = []
    for i in range(plan.n):
        a, b = ops["a"][i], ops["b"][i]
        assert a.size == plan.a_strides[i] and b.size == plan.b_strides[i]
        pairs.append((mo.compact(a, plan.a_size), mo.compact(b, plan.b_size)))
    acc = accumulated_tensor(ref, plan.cnv_offset, B, dst.data.n, dst.cols, plan.tensor_size, pairs, plan.a_effective_k, plan.b_effective_k)
    out = VecZnx(dst.data.n, dst.cols, dst.size)
    ref.glwe_tensor_relinearize(out, B, acc, B, tsk.pmat, tsk.dsize, tsk.base2k)
    dst.data.data[...] = out.data
    plan.apply_meta(dst)
