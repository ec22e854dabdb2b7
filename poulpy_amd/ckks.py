"""The linear CKKS operations of poulpy-ckks (src/leveled/default/{add,sub,neg,pow2,rescale,pt_znx}.rs), each as ONE device call, and its
rotations (rotate.rs, conjugate.rs) - one ciphertext batch by many Galois elements in one call (plan_rotate_many).

Every operation there is one overwriting poulpy-core GLWE primitive, at most one accumulating one, and optionally a final
glwe_normalize_assign.  Each primitive adds (or subtracts) a digit stream of its own operand, so an operation is one
pz_glwe_combine_batched call (include/poulpy_hip.h) whose terms this module derives from the ciphertext metadata, with
the reference's branch conditions and the same order of arguments in the shift amounts.  `plan_*` returns the Plan (terms, normalize
flag, new metadata) without touching a device; `Plan.launch` issues the call.  A plan that the reference would reject
(CKKSCompositionError) raises CKKSError before anything is launched.

Products and weighted sums by constants (mul.rs:342-415; leveled/delegates/composite.rs mul_add_pt_const / mul_sub_pt_const /
dot_product_pt_const) are at the end of the file: plan_mul_pt_const_* launch pz_glwe_mul_const_batched, the composites one
pz_glwe_lincomb_const_batched or, where that measured slower, the same sum term by term.

Products by plaintext vectors (mul.rs:243-293), their composites and the normalized sums (composite.rs add_many, mul_add_pt_vec_znx,
mul_sub_pt_vec_znx, dot_product_pt_vec_znx) come after the constants: the sums are ONE pz_glwe_sum_batched or, where that measured
slower, the chain of pz_glwe_combine_batched calls.

Products of two ciphertexts (mul.rs:47-200; composite.rs mul_add_ct / mul_sub_ct / mul_many) close the file: every product is ONE
pz_glwe_tensor_mul_relinearize_acc_batched, which reads operands in larger containers by stride, runs in place, and joins the product to
dst from the module's workspace.  ckks_dot_product_ct (composite.rs:563-703) is plan_dot_product_ct: its fast branch
tensors every pair into one accumulated tensor and relinearizes once - ONE pz_glwe_tensor_dot_relinearize_batched.
"""
from __future__ import annotations

from dataclasses import dataclass, field

RAW, LSH, RSH = 0, 1, 2            # PZ_TERM_RAW / _LSH / _RSH


class CKKSError(ValueError):
    """poulpy-ckks CKKSCompositionError (src/error.rs)."""


@dataclass
class Ct:
    """A CKKS ciphertext's layout and metadata (layouts/ciphertext.rs): GLWE(cols = rank + 1, size limbs) at base2k."""
    base2k: int
    size: int
    log_delta: int
    log_budget: int
    cols: int = 2
    data: object = None            # the host container (tests) or a device pointer (Plan.launch)

    @property
    def max_k(self) -> int:        # poulpy-core layouts/lwe.rs:23-25
        return self.size * self.base2k

    @property
    def effective_k(self) -> int:  # lib.rs:87-89
        return self.log_delta + self.log_budget


@dataclass
class Pt:
    """CKKSPlaintextVecZnx (layouts/plaintext/vec.rs): a VecZnx(1, size) at base2k with its log_delta and, for the products, its log_budget."""
    base2k: int
    size: int
    log_delta: int
    data: object = None
    log_budget: int = 0

    @property
    def max_k(self) -> int:
        return self.size * self.base2k


@dataclass
class Term:
    src: str                       # "a" | "b" | "dst" | "pt"
    kind: int
    k: int = 0
    sign: int = 1


@dataclass
class Plan:
    name: str
    terms: list = field(default_factory=list)
    normalize: bool = False
    log_delta: int = 0             # metadata of dst after the operation
    log_budget: int = 0
    offset: int = 0                # the offset_binary / offset_unary the reference computed
    shift: int = 0                 # pow2 / rescale: the one LSH amount
    pt_shift: int = 0              # plaintext terms: the rsh offset of ensure_plaintext_alignment

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dst: Ct, batch: int, a: Ct | None = None, b: Ct | None = None, pt: Pt | None = None, shared=()):
        """One pz_glwe_combine_batched over `batch` ciphertexts; .data of dst / a / b / pt are device pointers.  `shared`: names of the
        operands that hold one item for the whole batch.  No launch when there are no terms (div_pow2_assign)."""
        ops = {"dst": dst, "a": a, "b": b, "pt": pt}
        terms = []
        for t in self.terms:
            o = ops[t.src]
            terms.append(dict(a=o.data, a_size=o.size, kind=t.kind, k=t.k, sign=t.sign, col0_only=t.src == "pt", shared=t.src in shared,
                              base2k=o.base2k))
        if terms:
            module.glwe_combine_batched(dst.data, dst.cols, dst.size, dst.base2k, terms, self.normalize, batch)
        self.apply_meta(dst)


def checked_log_budget_sub(op: str, available: int, required: int) -> int:   # error.rs:113-122
    if required > available:
        raise CKKSError(f"{op}: insufficient homomorphic capacity (log_budget {available} < {required})")
    return available - required


def ensure_base2k_match(op: str, ct_base2k: int, pt_base2k: int):            # error.rs:124-134
    if ct_base2k != pt_base2k:
        raise CKKSError(f"{op}: plaintext base2k {pt_base2k} != ciphertext base2k {ct_base2k}")


def ensure_plaintext_alignment(op: str, ct_log_budget: int, pt_log_delta: int, pt_max_k: int) -> int:   # error.rs:136-154
    available = ct_log_budget + pt_log_delta
    if available < pt_max_k:
        raise CKKSError(f"{op}: plaintext alignment impossible ({ct_log_budget} + {pt_log_delta} < {pt_max_k})")
    return available - pt_max_k


def offset_binary(dst: Ct, a: Ct, b: Ct) -> int:   # layouts/ciphertext.rs:270-276
    return max(min(a.effective_k, b.effective_k) - dst.max_k, 0)


def offset_unary(dst: Ct, a: Ct) -> int:           # :278-283
    return max(a.effective_k - dst.max_k, 0)


def _same_layout(op, dst: Ct, *xs: Ct):
    for x in xs:
        if x.base2k != dst.base2k:        # glwe_lsh / glwe_lsh_add assert equal bases (poulpy-core operations/glwe.rs:1150)
            raise CKKSError(f"{op}: base2k {x.base2k} != {dst.base2k}")
        if x.cols != dst.cols:
            raise CKKSError(f"{op}: rank differs")


def plan_add_into(dst: Ct, a: Ct, b: Ct, sub=False, normalize=True) -> Plan:
    """add.rs:62-105 / sub.rs:62-105 (normalize=False: the _unsafe forms)."""
    name = "sub_into" if sub else "add_into"
    _same_layout(name, dst, a, b)
    s = -1 if sub else 1
    offset = offset_binary(dst, a, b)
    if offset == 0 and a.log_budget == b.log_budget:
        terms = [Term("a", RAW), Term("b", RAW, 0, s)]
    elif a.log_budget <= b.log_budget:
        terms = [Term("a", LSH, offset), Term("b", LSH, b.log_budget - a.log_budget + offset, s)]
    elif sub:                                                 # sub.rs:97-98: a by the difference + offset, b by offset
        terms = [Term("a", LSH, a.log_budget - b.log_budget + offset), Term("b", LSH, offset, -1)]
    else:                                                     # add.rs:97-98
        terms = [Term("b", LSH, offset), Term("a", LSH, a.log_budget - b.log_budget + offset)]
    log_budget = checked_log_budget_sub(name[:3], min(a.log_budget, b.log_budget), offset)
    return Plan(name, terms, normalize, min(a.log_delta, b.log_delta), log_budget, offset=offset)


def plan_add_assign(dst: Ct, a: Ct, sub=False, normalize=True) -> Plan:
    """add.rs:107-146 / sub.rs:107-146."""
    name = "sub_assign" if sub else "add_assign"
    _same_layout(name, dst, a)
    s = -1 if sub else 1
    if dst.log_budget < a.log_budget:
        terms = [Term("dst", RAW), Term("a", LSH, a.log_budget - dst.log_budget, s)]
    elif dst.log_budget > a.log_budget:
        terms = [Term("dst", LSH, dst.log_budget - a.log_budget), Term("a", RAW, 0, s)]
    else:
        terms = [Term("dst", RAW), Term("a", RAW, 0, s)]
    return Plan(name, terms, normalize, min(dst.log_delta, a.log_delta), min(dst.log_budget, a.log_budget))


def plan_neg_into(dst: Ct, src: Ct) -> Plan:
    """neg.rs:21-40."""
    _same_layout("neg", dst, src)
    offset = offset_unary(dst, src)
    if offset != 0:
        return Plan("neg_into", [Term("a", LSH, offset, -1)], False, src.log_delta, checked_log_budget_sub("neg", src.log_budget, offset),
                    offset=offset)
    return Plan("neg_into", [Term("a", RAW, 0, -1)], False, src.log_delta, src.log_budget)


def plan_neg_assign(dst: Ct) -> Plan:
    """neg.rs:42-48."""
    return Plan("neg_assign", [Term("dst", RAW, 0, -1)], False, dst.log_delta, dst.log_budget)


def plan_mul_pow2_into(dst: Ct, src: Ct, bits: int) -> Plan:
    """pow2.rs:25-36."""
    _same_layout("mul_pow2", dst, src)
    offset = offset_unary(dst, src)
    return Plan("mul_pow2_into", [Term("a", LSH, bits + offset)], False, src.log_delta,
                checked_log_budget_sub("mul_pow2", src.log_budget, offset), offset=offset, shift=bits + offset)


def plan_mul_pow2_assign(dst: Ct, bits: int) -> Plan:
    """pow2.rs:38-50: the metadata stays."""
    return Plan("mul_pow2_assign", [Term("dst", LSH, bits)], False, dst.log_delta, dst.log_budget, shift=bits)


def plan_div_pow2_into(dst: Ct, src: Ct, bits: int) -> Plan:
    """pow2.rs:52-66."""
    _same_layout("div_pow2", dst, src)
    offset = offset_unary(dst, src)
    return Plan("div_pow2_into", [Term("a", LSH, offset)], False, src.log_delta + bits,
                checked_log_budget_sub("div_pow2", src.log_budget, bits + offset), offset=offset, shift=offset)


def plan_div_pow2_assign(dst: Ct, bits: int) -> Plan:
    """pow2.rs:68-71: metadata only, no launch."""
    return Plan("div_pow2_assign", [], False, dst.log_delta, checked_log_budget_sub("div_pow2_assign", dst.log_budget, bits))


def plan_rescale_into(dst: Ct, src: Ct, k: int) -> Plan:
    """rescale.rs:38-52."""
    _same_layout("rescale", dst, src)
    log_budget = checked_log_budget_sub("rescale", src.log_budget, k)
    return Plan("rescale_into", [Term("a", LSH, k)], False, src.log_delta, log_budget, shift=k)


def plan_rescale_assign(dst: Ct, k: int) -> Plan:
    """rescale.rs:23-36."""
    log_budget = checked_log_budget_sub("rescale_assign", dst.log_budget, k)
    return Plan("rescale_assign", [Term("dst", LSH, k)], False, dst.log_delta, log_budget, shift=k)


def plan_align_assign(a: Ct, b: Ct):
    """rescale.rs:54-68: (which ciphertext is rescaled in place: "a" | "b", its plan)."""
    if a.log_budget < b.log_budget:
        return "b", plan_rescale_assign(b, b.log_budget - a.log_budget)
    return "a", plan_rescale_assign(a, a.log_budget - b.log_budget)


def plan_add_pt_into(dst: Ct, a: Ct, pt: Pt, sub=False, normalize=True) -> Plan:
    """add.rs:173-187 / sub.rs:164-181, then pt_znx.rs:17-53 on the result."""
    name = "sub_pt_into" if sub else "add_pt_into"
    _same_layout(name, dst, a)
    offset = offset_unary(dst, a)
    log_budget = checked_log_budget_sub(name[:-5] + "_vec_znx", a.log_budget, offset)
    ensure_base2k_match("ckks_" + name[:-5] + "_vec_znx_into", dst.base2k, pt.base2k)
    pt_shift = ensure_plaintext_alignment("ckks_" + name[:-5] + "_vec_znx_into", log_budget, pt.log_delta, pt.max_k)
    return Plan(name, [Term("a", LSH, offset), Term("pt", RSH, pt_shift, -1 if sub else 1)], normalize, a.log_delta, log_budget,
                offset=offset, pt_shift=pt_shift)


def plan_add_pt_assign(dst: Ct, pt: Pt, sub=False, normalize=True) -> Plan:
    """add.rs:189-210 / sub.rs analogues -> pt_znx.rs:17-53."""
    name = "sub_pt_assign" if sub else "add_pt_assign"
    ensure_base2k_match("ckks_" + name[:-7] + "_vec_znx_into", dst.base2k, pt.base2k)
    pt_shift = ensure_plaintext_alignment("ckks_" + name[:-7] + "_vec_znx_into", dst.log_budget, pt.log_delta, pt.max_k)
    return Plan(name, [Term("dst", RAW), Term("pt", RSH, pt_shift, -1 if sub else 1)], normalize, dst.log_delta, dst.log_budget,
                pt_shift=pt_shift)


@dataclass
class RotatePlan:
    """rotate.rs:23-56 for one source and one destination per Galois element: the metadata every destination takes, and the offset by which
    the reference shifts the source first (glwe_lsh into dst, then glwe_automorphism_assign: :46-48)."""
    name: str
    offset: int
    log_delta: int
    log_budget: int

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dsts, src: Ct, gals, key_ptrs, params, batch: int, tmp=None):
        """One pz_glwe_automorphism_many_batched over `batch` ciphertexts: dsts[0].data = the rotation-major device result (rotation r at
        r * batch ciphertexts), src.data the device source; gals[r] / key_ptrs[r] per destination (conjugation: the element 2N - 1).
        offset != 0: src is shifted first by one pz_glwe_combine_batched into `tmp` (a device pointer to `batch` ciphertexts of the
        destinations' layout), and params.a_size is the destinations' size as in the reference's assign form."""
        if len(gals) != len(dsts) or len(key_ptrs) != len(dsts):
            raise CKKSError(f"{self.name}: one Galois element and one key per destination")
        a = src.data
        if self.offset != 0:
            if tmp is None:
                raise CKKSError(f"{self.name}: offset {self.offset} needs a temporary of the destinations' layout")
            d0 = dsts[0]
            module.glwe_combine_batched(tmp, d0.cols, d0.size, d0.base2k, [dict(a=src.data, a_size=src.size, kind=LSH, k=self.offset)], False, batch)
            a = tmp
        module.glwe_automorphism_many_batched(dsts[0].data, a, gals, key_ptrs, params, batch)
        for d in dsts:
            self.apply_meta(d)


def plan_rotate_many(dsts, src: Ct) -> RotatePlan:
    """rotate.rs:44-55 (conjugate.rs alike) for several destinations of one layout rotated from the same source."""
    if not dsts:
        raise CKKSError("rotate: no destination")
    d0 = dsts[0]
    for d in dsts:
        _same_layout("rotate", d, src)
        if (d.size, d.base2k) != (d0.size, d0.base2k):
            raise CKKSError("rotate: the destinations of one call share one layout")
    offset = offset_unary(d0, src)
    return RotatePlan("rotate_many" if len(dsts) > 1 else "rotate_into", offset, src.log_delta,
                      checked_log_budget_sub("rotate", src.log_budget, offset))


def plan_rotate_into(dst: Ct, src: Ct) -> RotatePlan:
    """rotate.rs:23-56."""
    return plan_rotate_many([dst], src)


# ---- products and weighted sums by constants (leveled/default/mul.rs:342-415, leveled/delegates/composite.rs) ---------------------------
PLAIN, LSH_TERM, LSH_ACC = 0, 1, 2   # PZ_JOIN_PLAIN / _LSH_TERM / _LSH_ACC


@dataclass
class Cst:
    """CKKSPlaintextCstZnx (layouts/plaintext/cst.rs): the digits of re + i im at the ciphertext's base2k (either or both None) and the
    constant's metadata."""
    log_delta: int
    log_budget: int
    re: object = None
    im: object = None

    @property
    def empty(self) -> bool:
        return self.re is None and self.im is None


def min_k(log_delta: int, log_budget: int, base2k: int) -> int:   # lib.rs:79-81
    return -(-(log_delta + log_budget) // base2k) * base2k


def checked_mul_pt_log_budget(op: str, lhs_log_budget: int, rhs_log_budget: int, lhs_log_delta: int, rhs_log_delta: int) -> int:   # error.rs:177-194
    if rhs_log_delta > lhs_log_budget:
        raise CKKSError(f"{op}: multiplication precision underflow (lhs log_budget {lhs_log_budget}, log_delta {lhs_log_delta}; "
                        f"rhs log_budget {rhs_log_budget}, log_delta {rhs_log_delta})")
    return lhs_log_budget - rhs_log_delta


def get_mul_const_params(res: Ct, a: Ct, prec: Cst):
    """leveled/default/mul.rs:498-513 -> (res_log_budget, res_log_delta, cnv_offset)."""
    res_log_budget = checked_mul_pt_log_budget("mul_const", a.log_budget, prec.log_budget, a.log_delta, prec.log_delta)
    res_log_delta = a.log_delta
    res_offset = max(res_log_budget + res_log_delta - res.max_k, 0)
    cnv_offset = min_k(prec.log_delta, prec.log_budget, res.base2k) + res_offset
    return checked_log_budget_sub("mul_const", res_log_budget, res_offset), res_log_delta, cnv_offset


@dataclass
class ConstPlan:
    """ckks_mul_pt_const_znx_into / _assign (mul.rs:342-407): one pz_glwe_mul_const_batched."""
    name: str
    cnv_offset: int
    log_delta: int
    log_budget: int

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dst: Ct, batch: int, a: Ct | None, cst: Cst):
        from .hal import GlweMulConstParams
        assign = self.name.endswith("assign")
        src = dst if assign else a
        p = GlweMulConstParams(rank=dst.cols - 1, a_size=src.size, a_base2k=src.base2k, res_size=dst.size, res_base2k=dst.base2k,
                               cnv_offset=self.cnv_offset)
        module.glwe_mul_const_batched(dst.data, None if assign else a.data, cst.re, cst.im, p, "assign" if assign else "into", batch)
        self.apply_meta(dst)


def plan_mul_pt_const_into(dst: Ct, a: Ct, cst: Cst) -> ConstPlan:
    """mul.rs:342-374."""
    _same_layout("mul_pt_const_into", dst, a)
    log_budget, log_delta, cnv_offset = get_mul_const_params(dst, a, cst)
    return ConstPlan("mul_pt_const_into", cnv_offset, log_delta, log_budget)


def plan_mul_pt_const_assign(dst: Ct, cst: Cst) -> ConstPlan:
    """mul.rs:376-407."""
    log_budget, log_delta, cnv_offset = get_mul_const_params(dst, dst, cst)
    return ConstPlan("mul_pt_const_assign", cnv_offset, log_delta, log_budget)


@dataclass
class LinTerm:
    index: int                     # which operand / constant of the call
    cnv_offset: int
    join: int = PLAIN
    k: int = 0
    sign: int = 1
    log_delta: int = 0             # the product's own metadata (what the reference's scratch ciphertext carries)
    log_budget: int = 0


# Routing by measurement (tools/bench_ckks_lincomb.py): (nterms, complex) -> does the one-pass kernel beat the composition
# of pz_glwe_mul_const_batched into a scratch batch and pz_glwe_combine_batched by more than the run-to-run spread?  Where it does not,
# LincombPlan.launch takes the composition when the caller hands it a scratch batch.  Measured at N = 2^16, 16 limbs, 256 ciphertexts
# (profiles/ckks_lincomb_lines.jsonl): the one-pass kernel takes 1.6 - 2.2 x the composition's time at 1, 2, 8 and 32 terms, real and
# complex, so no case is routed to it; it remains the route that needs no scratch batch.
FUSED_WINS = frozenset()             # (nterms, complex) pairs measured in favour of the one-pass kernel


def fused_route(nterms: int, complex_terms: bool) -> bool:
    return (nterms, bool(complex_terms)) in FUSED_WINS


@dataclass
class LincombPlan:
    """ckks_mul_add_pt_const_* / ckks_mul_sub_pt_const_* / ckks_dot_product_pt_const_znx: one pz_glwe_lincomb_const_batched."""
    name: str
    init_res: bool
    terms: list = field(default_factory=list)
    normalize: bool = False
    log_delta: int = 0
    log_budget: int = 0

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def call_terms(self, ops, csts, shared=()):
        out = []
        for t in self.terms:
            o, c = ops[t.index], csts[t.index]
            out.append(dict(a=o.data, a_size=o.size, cnv_offset=t.cnv_offset, re=c.re, im=c.im, shared=t.index in shared, join=t.join, k=t.k,
                            sign=t.sign))
        return out

    def launch(self, module, dst: Ct, batch: int, ops, csts, shared=(), tmp=None, route=None):
        """ops[i].data / dst.data: device pointers; csts[i]: the constants (host digits); shared: indices of the operands that hold one
        ciphertext for the whole batch.  No launch when there are no terms (an empty constant in mul_add / mul_sub).  route: "fused" |
        "composed" | None (fused_route(); the composition needs `tmp`, a device pointer to `batch` ciphertexts of dst's layout)."""
        if self.terms:
            if route is None:
                fused = tmp is None or fused_route(len(self.terms), any(csts[t.index].im is not None for t in self.terms))
                route = "fused" if fused else "composed"
            if route == "fused":
                module.glwe_lincomb_const_batched(dst.data, dst.cols - 1, dst.size, dst.base2k, self.call_terms(ops, csts, shared), self.init_res,
                                                  self.normalize, batch)
            else:
                self.launch_composed(module, dst, batch, ops, csts, shared, tmp)
        self.apply_meta(dst)

    def launch_composed(self, module, dst: Ct, batch: int, ops, csts, shared, tmp):
        """The same sum term by term, as the reference runs it: pz_glwe_mul_const_batched into `tmp`, then one pz_glwe_combine_batched that
        joins it to dst (the closing glwe_normalize_assign rides on the last one)."""
        from .hal import GlweMulConstParams
        if tmp is None:
            raise CKKSError(f"{self.name}: the composed route needs a scratch batch of dst's layout")
        for n, t in enumerate(self.terms):
            o, c = ops[t.index], csts[t.index]
            p = GlweMulConstParams(rank=dst.cols - 1, a_size=o.size, a_base2k=o.base2k, res_size=dst.size, res_base2k=dst.base2k,
                                   cnv_offset=t.cnv_offset)
            last = n == len(self.terms) - 1
            one = t.index in shared
            if n == 0 and not self.init_res and not one:
                module.glwe_mul_const_batched(dst.data, o.data, c.re, c.im, p, "into", batch)
                if last and self.normalize:
                    module.glwe_combine_batched(dst.data, dst.cols, dst.size, dst.base2k, [dict(a=dst.data, a_size=dst.size, kind=RAW)], True, batch)
                continue
            module.glwe_mul_const_batched(tmp, o.data, c.re, c.im, p, "into", 1 if one else batch)
            prod = dict(a=tmp, a_size=dst.size, kind=LSH if t.join == LSH_TERM else RAW, k=t.k if t.join == LSH_TERM else 0, sign=t.sign, shared=one)
            acc = dict(a=dst.data, a_size=dst.size, kind=LSH if t.join == LSH_ACC else RAW, k=t.k if t.join == LSH_ACC else 0)
            terms = [prod] if n == 0 and not self.init_res else [acc, prod]
            module.glwe_combine_batched(dst.data, dst.cols, dst.size, dst.base2k, terms, last and self.normalize, batch)


def _join(acc_log_budget: int, tmp_log_budget: int):
    """the branch of ckks_add_assign_unsafe / ckks_sub_assign_unsafe (add.rs:132-141, sub.rs:132-141) -> (join, k)"""
    if acc_log_budget < tmp_log_budget:
        return LSH_TERM, tmp_log_budget - acc_log_budget
    if acc_log_budget > tmp_log_budget:
        return LSH_ACC, acc_log_budget - tmp_log_budget
    return PLAIN, 0


def plan_mul_add_pt_const(dst: Ct, a: Ct, cst: Cst, sub=False) -> LincombPlan:
    """composite.rs:290-308 / :423-441: the product into a scratch ciphertext of dst's layout, then ckks_add_assign / ckks_sub_assign
    (normalized).  An empty constant: no launch, dst and its metadata untouched (:301-303)."""
    name = "mul_sub_pt_const" if sub else "mul_add_pt_const"
    if cst.empty:
        return LincombPlan(name, True, [], False, dst.log_delta, dst.log_budget)
    _same_layout(name, dst, a)
    log_budget, log_delta, cnv_offset = get_mul_const_params(dst, a, cst)
    join, k = _join(dst.log_budget, log_budget)
    term = LinTerm(0, cnv_offset, join, k, -1 if sub else 1, log_delta, log_budget)
    return LincombPlan(name, True, [term], True, min(dst.log_delta, log_delta), min(dst.log_budget, log_budget))


def plan_mul_sub_pt_const(dst: Ct, a: Ct, cst: Cst) -> LincombPlan:
    return plan_mul_add_pt_const(dst, a, cst, sub=True)


def plan_dot_product_pt_const(dst: Ct, ops, csts) -> LincombPlan:
    """composite.rs:760-784 with accumulate_unnormalized (:478-506): dst = sum_i csts[i] * ops[i].  n = 1 is the plain product; an
    all-empty constant is a zero product that still takes part in the budget alignment."""
    name = "dot_product_pt_const"
    if len(ops) == 0:                                                     # check_lengths, :468-476
        raise CKKSError(f"{name}: inputs must contain at least one pair")
    if len(ops) != len(csts):
        raise CKKSError(f"{name}: length mismatch between ct vector ({len(ops)}) and weight vector ({len(csts)})")
    n = len(ops)
    if dst.base2k >= 64 or n > (1 << (63 - dst.base2k)):                  # ensure_accumulation_fits, :43-51
        raise CKKSError(f"{name}: {n} terms risks i64 overflow at base2k={dst.base2k}")
    terms = []
    log_delta = log_budget = 0
    for i, (a, c) in enumerate(zip(ops, csts)):
        _same_layout(name, dst, a)
        tb, td, cnv_offset = get_mul_const_params(dst, a, c)
        if i == 0:
            terms.append(LinTerm(0, cnv_offset, PLAIN, 0, 1, td, tb))
            log_delta, log_budget = td, tb
            continue
        join, k = _join(log_budget, tb)
        terms.append(LinTerm(i, cnv_offset, join, k, 1, td, tb))
        log_delta, log_budget = min(log_delta, td), min(log_budget, tb)
    return LincombPlan(name, False, terms, n > 1, log_delta, log_budget)


# ---- products by plaintext vectors, and the normalized sums (leveled/default/mul.rs:243-293, leveled/delegates/composite.rs) -------------
def get_mul_pt_params(res: Ct, a: Ct, pt: Pt):
    """leveled/default/mul.rs:480-496 -> (res_log_budget, res_log_delta, cnv_offset)."""
    res_log_budget = checked_mul_pt_log_budget("mul", a.log_budget, pt.log_budget, a.log_delta, pt.log_delta)
    res_log_delta = a.log_delta
    res_offset = max(res_log_budget + res_log_delta - res.max_k, 0)
    cnv_offset = pt.max_k + res_offset
    return checked_log_budget_sub("mul", res_log_budget, res_offset), res_log_delta, cnv_offset


def _mul_plain_shape(op: str, res: Ct, a: Ct, pt: Pt):
    """what glwe_mul_plain asserts (poulpy-core operations/glwe.rs:207-209): one base2k, sizes that match the effective precisions"""
    _same_layout(op, res, a)
    ensure_base2k_match(op, a.base2k, pt.base2k)
    if a.size != -(-a.effective_k // a.base2k):
        raise CKKSError(f"{op}: ciphertext size {a.size} != effective_k {a.effective_k} / base2k {a.base2k}, rounded up")
    if pt.size != -(-pt.max_k // pt.base2k):
        raise CKKSError(f"{op}: plaintext size {pt.size} != max_k {pt.max_k} / base2k {pt.base2k}, rounded up")


def _mul_plain_call(module, res_ptr, dst: Ct, a: Ct, a_ptr, pt: Pt, cnv_offset: int, pt_shared: bool, mode: str, batch: int):
    from .hal import GlweTensorParams
    p = GlweTensorParams(rank=dst.cols - 1, a_size=a.size, b_size=pt.size, ab_base2k=a.base2k, a_effective_k=a.effective_k,
                         b_effective_k=pt.max_k, res_size=dst.size, res_base2k=dst.base2k, cnv_offset=cnv_offset)
    module.glwe_mul_plain_batched(res_ptr, a_ptr, pt.data, pt_shared, p, mode, batch)


@dataclass
class PtMulPlan:
    """ckks_mul_pt_vec_znx_into / _assign (mul.rs:243-293): one pz_glwe_mul_plain_batched."""
    name: str
    cnv_offset: int
    log_delta: int
    log_budget: int

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dst: Ct, batch: int, a: Ct | None, pt: Pt, pt_shared=False):
        """dst.data / a.data / pt.data: device pointers; pt_shared: one plaintext for the whole batch."""
        assign = self.name.endswith("assign")
        src = dst if assign else a
        _mul_plain_call(module, dst.data, dst, src, None if assign else a.data, pt, self.cnv_offset, pt_shared, "assign" if assign else "into", batch)
        self.apply_meta(dst)


def plan_mul_pt_vec_znx_into(dst: Ct, a: Ct, pt: Pt) -> PtMulPlan:
    """mul.rs:243-268."""
    _mul_plain_shape("mul_pt_vec_znx_into", dst, a, pt)
    log_budget, log_delta, cnv_offset = get_mul_pt_params(dst, a, pt)
    return PtMulPlan("mul_pt_vec_znx_into", cnv_offset, log_delta, log_budget)


def plan_mul_pt_vec_znx_assign(dst: Ct, pt: Pt) -> PtMulPlan:
    """mul.rs:270-293."""
    _mul_plain_shape("mul_pt_vec_znx_assign", dst, dst, pt)
    log_budget, log_delta, cnv_offset = get_mul_pt_params(dst, dst, pt)
    return PtMulPlan("mul_pt_vec_znx_assign", cnv_offset, log_delta, log_budget)


@dataclass
class PtMulAddPlan:
    """ckks_mul_add_pt_vec_znx_into / ckks_mul_sub_pt_vec_znx_into (composite.rs:256-270, :389-403): the product into a scratch batch of
    dst's layout with default metadata, then the normalizing ckks_add_assign / ckks_sub_assign - two launches."""
    name: str
    mul: PtMulPlan
    add: Plan
    log_delta: int
    log_budget: int

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dst: Ct, batch: int, a: Ct, pt: Pt, tmp, pt_shared=False):
        """tmp: a device pointer to `batch` ciphertexts of dst's layout."""
        if tmp is None:
            raise CKKSError(f"{self.name}: needs a scratch batch of dst's layout")
        prod = Ct(dst.base2k, dst.size, 0, 0, dst.cols, tmp)
        self.mul.launch(module, prod, batch, a, pt, pt_shared)
        self.add.launch(module, dst, batch, a=prod)


def plan_mul_add_pt_vec_znx(dst: Ct, a: Ct, pt: Pt, sub=False) -> PtMulAddPlan:
    name = "mul_sub_pt_vec_znx" if sub else "mul_add_pt_vec_znx"
    prod = Ct(dst.base2k, dst.size, 0, 0, dst.cols)
    mul = plan_mul_pt_vec_znx_into(prod, a, pt)
    mul.apply_meta(prod)
    add = plan_add_assign(dst, prod, sub=sub, normalize=True)
    return PtMulAddPlan(name, mul, add, add.log_delta, add.log_budget)


def plan_mul_sub_pt_vec_znx(dst: Ct, a: Ct, pt: Pt) -> PtMulAddPlan:
    return plan_mul_add_pt_vec_znx(dst, a, pt, sub=True)


@dataclass
class SumTerm:
    index: int                     # which input / product of the call
    join: int = PLAIN
    k: int = 0
    sign: int = 1
    log_delta: int = 0             # the term's own metadata
    log_budget: int = 0
    cnv_offset: int = 0            # dot products: the product's cnv_offset


# Routing by measurement (tools/bench_ckks_sum.py): the term counts at which ONE pz_glwe_sum_batched beat the chain of
# pz_glwe_combine_batched calls by more than the spread between two runs of itself.  Measured at N = 2^16, 16 limbs, 256 ciphertexts
# (profiles/ckks_sum_lines.jsonl): at 2 and 4 terms the chain is ONE combine call and the one-pass call takes 1.06 / 1.03 x its time; at 5, 8,
# 16 and 32 terms it takes 0.76 / 0.70 / 0.67 / 0.60 x (0.58 x with mixed joins at 8), spread 0.1 %.  The counts between two measured wins
# are routed with them; 3 terms (one combine call, like 2 and 4) and more than 32 (not measured) take the chain, the code as it stood
# before the one-pass call.
SUM_WINS = frozenset(range(5, 33))


def sum_route(nterms: int) -> bool:
    return nterms in SUM_WINS


def _ensure_accumulation_fits(op: str, dst: Ct, n: int):                  # composite.rs:43-51
    if dst.base2k >= 64 or n > (1 << (63 - dst.base2k)):
        raise CKKSError(f"{op}: {n} terms risks i64 overflow at base2k={dst.base2k}")


def chain_calls(terms, started=False):
    """The joins of `terms` as today's sequence of pz_glwe_combine_batched calls: lists of (src, kind, k, sign) with src "dst" or a term,
    at most four per call; every call but the first re-reads dst, a PZ_JOIN_LSH_ACC shifts it there.  started: dst already holds a
    partial sum, so the first call re-reads it too."""
    calls, cur = [], []
    for t in terms:
        if t.join == LSH_ACC and (started or cur):
            if cur and not (len(cur) == 1 and cur[0][0] == "dst"):
                calls.append(cur)
                started = True
            cur = [("dst", LSH, t.k, 1)]
        elif not cur and started:
            cur = [("dst", RAW, 0, 1)]
        if len(cur) == 4:
            calls.append(cur)
            started = True
            cur = [("dst", RAW, 0, 1)]
        cur.append((t, LSH if t.join == LSH_TERM else RAW, t.k if t.join == LSH_TERM else 0, t.sign))
    calls.append(cur)
    return calls


SUM_MAX_TERMS = 64       # terms of one pz_glwe_sum_batched
INPLACE_MAX_LIMBS = 32   # limbs of res that either call can shift in place (staged in LDS: kSumMaxStage, kCombMaxStage)


def _check_joins(name: str, dst: Ct, terms, route: str, continues=False):
    """What the device calls of _launch_joins would refuse, raised before anything is launched: more than 64 terms in one
    pz_glwe_sum_batched, and a running sum of more than 32 limbs shifted in place by a limb or more - by the one-pass call where it
    continues from dst, by the chain in every call that re-reads dst.  Neither route serves the latter."""
    if route == "sum":
        if len(terms) + continues > SUM_MAX_TERMS:
            raise CKKSError(f"{name}: {len(terms) + continues} terms in one pz_glwe_sum_batched (at most {SUM_MAX_TERMS}); take route=\"chain\" or fewer slots")
        shifted = continues and sum(t.k for t in terms if t.join == LSH_ACC) >= dst.base2k
    else:
        shifted = any(t.join == LSH_ACC and t.k >= dst.base2k and (continues or u > 0) for u, t in enumerate(terms))
    if shifted and dst.size > INPLACE_MAX_LIMBS:
        raise CKKSError(f"{name}: the running sum ({dst.size} limbs) would be shifted in place by a limb or more; at most {INPLACE_MAX_LIMBS} limbs")


def _launch_joins(module, dst: Ct, batch: int, terms, operand, route, continues=False):
    """the normalized sum of `terms` into dst: operand(t) -> (device pointer, size, shared).  route "sum": one pz_glwe_sum_batched;
    "chain": pz_glwe_combine_batched calls, the last one normalizing.  continues: the sum starts from dst's content."""
    if route == "sum":
        call = [dict(a=dst.data, a_size=dst.size)] if continues else []
        for t in terms:
            ptr, size, shared = operand(t)
            call.append(dict(a=ptr, a_size=size, shared=shared, join=t.join, k=t.k, sign=t.sign))
        module.glwe_sum_batched(dst.data, dst.cols, dst.size, dst.base2k, call, batch)
        return
    calls = chain_calls(terms, continues)
    for n, c in enumerate(calls):
        out = []
        for src, kind, k, sign in c:
            ptr, size, shared = (dst.data, dst.size, False) if isinstance(src, str) else operand(src)
            out.append(dict(a=ptr, a_size=size, kind=kind, k=k, sign=sign, shared=shared))
        module.glwe_combine_batched(dst.data, dst.cols, dst.size, dst.base2k, out, n == len(calls) - 1, batch)


@dataclass
class SumPlan:
    """ckks_add_many (composite.rs:63-93): one pz_glwe_sum_batched, or the chain of pz_glwe_combine_batched calls."""
    name: str
    terms: list = field(default_factory=list)
    normalize: bool = False
    log_delta: int = 0
    log_budget: int = 0

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dst: Ct, batch: int, inputs, shared=(), route=None):
        """inputs[i].data / dst.data: device pointers; shared: indices of the inputs that hold one ciphertext for the whole batch.
        route: "sum" | "chain" | None (sum_route())."""
        if route not in ("sum", "chain", None):
            raise CKKSError(f"{self.name}: unknown route {route!r}")
        op = lambda t: (inputs[t.index].data, inputs[t.index].size, t.index in shared)
        if not self.normalize:                                            # n = 1: glwe_lsh, un-normalized
            (t,) = self.terms
            module.glwe_combine_batched(dst.data, dst.cols, dst.size, dst.base2k,
                                        [dict(a=op(t)[0], a_size=op(t)[1], kind=LSH, k=t.k, shared=op(t)[2])], False, batch)
        else:
            if route is None:
                route = "sum" if sum_route(len(self.terms)) else "chain"
            _check_joins(self.name, dst, self.terms, route)
            _launch_joins(module, dst, batch, self.terms, op, route)
        self.apply_meta(dst)


def plan_add_many(dst: Ct, inputs) -> SumPlan:
    """composite.rs:63-93: add_into_unsafe on the first two inputs, add_assign_unsafe on each further one, the closing normalize."""
    name = "add_many"
    n = len(inputs)
    if n == 0:
        raise CKKSError("ckks_add_many: inputs must contain at least one ciphertext")
    for x in inputs:
        _same_layout(name, dst, x)
    if n == 1:
        offset = offset_unary(dst, inputs[0])
        log_budget = checked_log_budget_sub("ckks_add_many", inputs[0].log_budget, offset)
        return SumPlan(name, [SumTerm(0, LSH_TERM, offset, 1, inputs[0].log_delta, inputs[0].log_budget)], False, inputs[0].log_delta,
                       log_budget)
    _ensure_accumulation_fits("ckks_add_many", dst, n)
    first = plan_add_into(dst, inputs[0], inputs[1], normalize=False)     # add.rs:76-104, terms in the reference's order
    terms = []
    for t in first.terms:
        i = 0 if t.src == "a" else 1
        terms.append(SumTerm(i, PLAIN if t.kind == RAW else LSH_TERM, t.k, 1, inputs[i].log_delta, inputs[i].log_budget))
    log_delta, log_budget = first.log_delta, first.log_budget
    for i in range(2, n):
        join, k = _join(log_budget, inputs[i].log_budget)
        terms.append(SumTerm(i, join, k, 1, inputs[i].log_delta, inputs[i].log_budget))
        log_delta, log_budget = min(log_delta, inputs[i].log_delta), min(log_budget, inputs[i].log_budget)
    return SumPlan(name, terms, True, log_delta, log_budget)


@dataclass
class DotPlan:
    """ckks_dot_product_pt_vec_znx (composite.rs:705-729): pz_glwe_mul_plain_batched per product into scratch slots, joined `slots` at a
    time by one pz_glwe_sum_batched (or the chain) per chunk; later chunks continue from dst, stored normalized, as term 0."""
    name: str
    terms: list = field(default_factory=list)
    normalize: bool = False
    log_delta: int = 0
    log_budget: int = 0

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dst: Ct, batch: int, ops, pts, tmp=None, slots=None, pt_shared=(), route=None):
        """ops[i].data / pts[i].data / dst.data: device pointers; pt_shared: indices of the plaintexts that hold one item for the whole
        batch; tmp: a device pointer to slots x batch ciphertexts of dst's layout, 1 <= slots <= n (not needed for n = 1)."""
        if route not in ("sum", "chain", None):
            raise CKKSError(f"{self.name}: unknown route {route!r}")
        n = len(self.terms)
        if not self.normalize:                                            # n = 1: the plain product into dst
            (t,) = self.terms
            _mul_plain_call(module, dst.data, dst, ops[t.index], ops[t.index].data, pts[t.index], t.cnv_offset, t.index in pt_shared, "into", batch)
            self.apply_meta(dst)
            return
        if tmp is None or slots is None or not 1 <= slots <= n:
            raise CKKSError(f"{self.name}: needs a scratch of slots x batch ciphertexts of dst's layout, 1 <= slots <= {n}")
        base = tmp.value if hasattr(tmp, "value") else int(tmp)
        slot_bytes = batch * dst.cols * dst.size * module.n() * 8
        chunks = []                                                       # (first term, terms, route): by the terms of the chunk's own call
        for lo in range(0, n, slots):
            chunk = self.terms[lo:lo + slots]
            chunks.append((lo, chunk, route or ("sum" if sum_route(len(chunk) + (lo > 0)) else "chain")))
            _check_joins(self.name, dst, chunk, chunks[-1][2], continues=lo > 0)
        for lo, chunk, by in chunks:
            where = {}
            for s, t in enumerate(chunk):
                where[id(t)] = base + s * slot_bytes
                _mul_plain_call(module, where[id(t)], dst, ops[t.index], ops[t.index].data, pts[t.index], t.cnv_offset, t.index in pt_shared,
                                "into", batch)
            _launch_joins(module, dst, batch, chunk, lambda t: (where[id(t)], dst.size, False), by, continues=lo > 0)
        self.apply_meta(dst)


def plan_dot_product_pt_vec_znx(dst: Ct, ops, pts) -> DotPlan:
    """composite.rs:705-729 with accumulate_unnormalized (:478-506): dst = sum_i pts[i] * ops[i].  n = 1 is the plain product."""
    name = "dot_product_pt_vec_znx"
    if len(ops) == 0:                                                     # check_lengths, :468-476
        raise CKKSError(f"{name}: inputs must contain at least one pair")
    if len(ops) != len(pts):
        raise CKKSError(f"{name}: length mismatch between ct vector ({len(ops)}) and weight vector ({len(pts)})")
    n = len(ops)
    _ensure_accumulation_fits(name, dst, n)
    terms = []
    log_delta = log_budget = 0
    for i, (a, pt) in enumerate(zip(ops, pts)):
        _mul_plain_shape(name, dst, a, pt)
        tb, td, cnv_offset = get_mul_pt_params(dst, a, pt)
        if i == 0:
            terms.append(SumTerm(0, PLAIN, 0, 1, td, tb, cnv_offset))
            log_delta, log_budget = td, tb
            continue
        join, k = _join(log_budget, tb)
        terms.append(SumTerm(i, join, k, 1, td, tb, cnv_offset))
        log_delta, log_budget = min(log_delta, td), min(log_budget, tb)
    return DotPlan(name, terms, n > 1, log_delta, log_budget)


# ---- products of two ciphertexts (leveled/default/mul.rs:47-200, leveled/delegates/composite.rs:103-165, :239-254) -------------------------
def checked_mul_ct_log_budget(op: str, lhs_log_budget: int, rhs_log_budget: int, lhs_log_delta: int, rhs_log_delta: int) -> int:   # error.rs:155-175
    if max(lhs_log_delta, rhs_log_delta) > min(lhs_log_budget, rhs_log_budget):
        raise CKKSError(f"{op}: multiplication precision underflow (lhs log_budget {lhs_log_budget}, log_delta {lhs_log_delta}; "
                        f"rhs log_budget {rhs_log_budget}, log_delta {rhs_log_delta})")
    return min(lhs_log_budget, rhs_log_budget) - max(lhs_log_delta, rhs_log_delta)


def get_mul_ct_params(res: Ct, a: Ct, b: Ct):
    """leveled/default/mul.rs:461-478 -> (res_log_budget, res_log_delta, cnv_offset)."""
    res_log_budget = checked_mul_ct_log_budget("mul", a.log_budget, b.log_budget, a.log_delta, b.log_delta)
    res_log_delta = min(a.log_delta, b.log_delta)
    res_offset = max(res_log_budget + res_log_delta - res.max_k, 0)
    cnv_offset = max(a.effective_k, b.effective_k) + res_offset
    return checked_log_budget_sub("mul", res_log_budget, res_offset), res_log_delta, cnv_offset


def ceil_log2(n: int) -> int:                                             # composite.rs:98-101
    return 0 if n <= 1 else (n - 1).bit_length()


def _operand_size(op: str, x: Ct) -> int:
    """the limbs of x that enter glwe_tensor_apply: effective_k.div_ceil(base2k) (poulpy-core operations/glwe.rs:722-723).  The container
    may hold more (after a rescale): the device call then takes the container's size as the stride; the reference would reallocate
    (ckks_compact_limbs, layouts/ciphertext.rs:216-232).  It may not hold fewer."""
    size = -(-x.effective_k // x.base2k)
    if size < 1:
        raise CKKSError(f"{op}: an operand of effective_k {x.effective_k} has no limb")
    if size > x.size:
        raise CKKSError(f"{op}: the container ({x.size} limbs) is smaller than effective_k {x.effective_k} / base2k {x.base2k}, rounded up")
    return size


@dataclass
class MulPlan:
    """ckks_mul_into / _assign, ckks_square_into / _assign (mul.rs:47-200), and with `join` ckks_mul_add_ct_into / ckks_mul_sub_ct_into
    (composite.rs:239-254, :372-387): ONE pz_glwe_tensor_mul_relinearize_acc_batched.  which: where a / b come from at launch ("a" | "b" |
    "dst"); b is None for a square."""
    name: str
    cnv_offset: int
    log_delta: int                 # metadata of dst after the operation
    log_budget: int
    which: tuple = ("a", "b")
    a_size: int = 0                # limbs of the operands (effective_k.div_ceil(base2k)) ...
    b_size: int = 0
    a_stride: int = 0              # ... and of their containers
    b_stride: int = 0
    a_effective_k: int = 0
    b_effective_k: int = 0
    tensor_size: int = 0           # limbs of the tensor layout: k = max(a.max_k, b.max_k)
    join: int | None = None        # mul_add / mul_sub: the join of the product to dst, (join, k, sign), always normalized
    k: int = 0
    sign: int = 1
    prod_log_delta: int = 0        # mul_add / mul_sub: what the scratch ciphertext carries (take_mul_tmp)
    prod_log_budget: int = 0

    @property
    def square(self) -> bool:
        return self.which[1] is None

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def params(self, dst: Ct, tsk):
        """(pz_glwe_tensor_params, pz_glwe_op_params) of the call; tsk: the prepared tensor key's (dnum, dsize, key_size, key_base2k)"""
        from .hal import GlweOpParams, GlweTensorParams
        dnum, dsize, key_size, key_base2k = tsk
        rank = dst.cols - 1
        tp = GlweTensorParams(rank=rank, a_size=self.a_size, b_size=self.b_size, ab_base2k=dst.base2k, a_effective_k=self.a_effective_k,
                              b_effective_k=self.b_effective_k, res_size=self.tensor_size, res_base2k=dst.base2k, cnv_offset=self.cnv_offset)
        rp = GlweOpParams(rank=rank, dnum=dnum, dsize=dsize, key_size=key_size, key_base2k=key_base2k, a_size=self.tensor_size,
                          a_base2k=dst.base2k, res_size=dst.size, res_base2k=dst.base2k, rank_out=rank)
        return tp, rp

    def launch(self, module, dst: Ct, batch: int, a: Ct | None = None, b: Ct | None = None, tsk_ptr=None, tsk=None):
        """dst.data / a.data / b.data / tsk_ptr: device pointers; tsk = (dnum, dsize, key_size, key_base2k) of the prepared tensor key.
        The operands named "dst" in `which` are dst itself (the _assign forms)."""
        ops = {"a": a, "b": b, "dst": dst, None: None}
        x, y = ops[self.which[0]], ops[self.which[1]]
        tp, rp = self.params(dst, tsk)
        module.glwe_tensor_mul_relinearize_acc_batched(dst.data, x.data, None if y is None else y.data, tsk_ptr, tp, rp, "square" if self.square else "apply",
                                                       batch, a_stride=self.a_stride, b_stride=self.b_stride, accumulate=self.join is not None,
                                                       join=self.join or PLAIN, k=self.k, sign=self.sign, normalize=True)
        self.apply_meta(dst)


def _mul_plan(name: str, res: Ct, a: Ct, b: Ct | None, which) -> MulPlan:
    """get_mul_ct_params on (res, a, b) and the shapes of the call; b None: the square (get_mul_ct_params(res, a, a))"""
    y = a if b is None else b
    _same_layout(name, res, a, y)
    log_budget, log_delta, cnv_offset = get_mul_ct_params(res, a, y)
    a_size, b_size = _operand_size(name, a), _operand_size(name, y)
    return MulPlan(name, cnv_offset, log_delta, log_budget, which, a_size, b_size, a.size, y.size, a.effective_k, y.effective_k,
                   max(a.size, y.size))


def plan_mul_into(dst: Ct, a: Ct, b: Ct) -> MulPlan:
    """mul.rs:47-84."""
    return _mul_plan("mul_into", dst, a, b, ("a", "b"))


def plan_mul_assign(dst: Ct, a: Ct) -> MulPlan:
    """mul.rs:86-122: dst = dst a."""
    return _mul_plan("mul_assign", dst, dst, a, ("dst", "a"))


def plan_square_into(dst: Ct, a: Ct) -> MulPlan:
    """mul.rs:145-172."""
    return _mul_plan("square_into", dst, a, None, ("a", None))


def plan_square_assign(dst: Ct) -> MulPlan:
    """mul.rs:174-200: dst = dst^2."""
    return _mul_plan("square_assign", dst, dst, None, ("dst", None))


def plan_mul_add_ct(dst: Ct, a: Ct, b: Ct, sub=False) -> MulPlan:
    """composite.rs:239-254 / :372-387: ckks_mul_into on a scratch ciphertext of dst's layout with default metadata (take_mul_tmp), then
    ckks_add_assign / ckks_sub_assign (normalized).  On the device the scratch product exists one wave at a time in the module's workspace."""
    name = "mul_sub_ct" if sub else "mul_add_ct"
    tmp = Ct(dst.base2k, dst.size, 0, 0, dst.cols)
    p = _mul_plan(name, tmp, a, b, ("a", "b"))
    p.prod_log_delta, p.prod_log_budget = p.log_delta, p.log_budget
    p.join, p.k = _join(dst.log_budget, p.prod_log_budget)
    p.sign = -1 if sub else 1
    if p.join == LSH_ACC and p.k >= dst.base2k and dst.size > INPLACE_MAX_LIMBS:
        raise CKKSError(f"{name}: dst ({dst.size} limbs) would be shifted in place by a limb or more; at most {INPLACE_MAX_LIMBS} limbs")
    p.log_delta, p.log_budget = min(dst.log_delta, p.prod_log_delta), min(dst.log_budget, p.prod_log_budget)
    return p


def plan_mul_sub_ct(dst: Ct, a: Ct, b: Ct) -> MulPlan:
    return plan_mul_add_ct(dst, a, b, sub=True)


@dataclass
class MulManyNode:
    """one step of mul_many_rec in the reference's evaluation order.  out / a / b: "dst", ("in", i) or ("slot", s); ct: the layout and
    metadata of the node's result (a scratch ciphertext of the recursion, or dst); op: "lsh" (one input: glwe_lsh by `shift`) | "mul"."""
    op: str
    out: object
    a: object
    b: object = None
    ct: Ct = None
    shift: int = 0
    mul: MulPlan | None = None


@dataclass
class MulManyPlan:
    """ckks_mul_many (composite.rs:103-198).  Every "mul" node is ONE pz_glwe_tensor_mul_relinearize_acc_batched on `batch` ciphertexts,
    every "lsh" node one pz_glwe_combine_batched.  The intermediate products live in scratch slots (slot s: slot_limbs[s] limbs per
    ciphertext); a slot is free again once the node that reads it has run.  Where a node's operand has fewer effective limbs than its
    container (the reference's glwe_tensor_apply would fail its size == effective_k.div_ceil(base2k) assertion there, and the caller
    would reallocate with ckks_compact_limbs), the call gets stride = the container's size and size = the effective one."""
    name: str
    nodes: list = field(default_factory=list)
    slot_limbs: list = field(default_factory=list)
    log_delta: int = 0
    log_budget: int = 0
    cols: int = 2

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def slot_offsets(self, batch: int, n: int):
        """byte offset of every slot in the scratch buffer (256-byte aligned) and the total"""
        offs, at = [], 0
        for limbs in self.slot_limbs:
            offs.append(at)
            at += -(-(batch * self.cols * limbs * n * 8) // 256) * 256
        return offs, at

    def scratch_bytes(self, batch: int, n: int) -> int:
        return self.slot_offsets(batch, n)[1]

    def launch(self, module, dst: Ct, batch: int, inputs, tsk_ptr=None, tsk=None, tmp=None):
        """dst.data / inputs[i].data / tsk_ptr: device pointers; tmp: a device pointer to scratch_bytes(batch, module.n()) bytes (not needed
        for one or two inputs)."""
        offs, total = self.slot_offsets(batch, module.n())
        if total and tmp is None:
            raise CKKSError(f"{self.name}: needs {total} bytes of scratch")
        base = 0 if tmp is None else (tmp.value if hasattr(tmp, "value") else int(tmp))

        def where(ref):
            if ref == "dst":
                return dst.data
            if ref[0] == "in":
                return inputs[ref[1]].data
            return base + offs[ref[1]]
        for nd in self.nodes:
            out = Ct(nd.ct.base2k, nd.ct.size, 0, 0, nd.ct.cols, where(nd.out))
            if nd.op == "lsh":
                src = inputs[nd.a[1]]
                module.glwe_combine_batched(out.data, out.cols, out.size, out.base2k, [dict(a=src.data, a_size=src.size, kind=LSH, k=nd.shift)], False, batch)
                continue
            a = Ct(0, 0, 0, 0, data=where(nd.a))
            b = Ct(0, 0, 0, 0, data=where(nd.b))
            nd.mul.launch(module, out, batch, a, b, tsk_ptr, tsk)
        self.apply_meta(dst)


def plan_mul_many(dst: Ct, inputs) -> MulManyPlan:
    """composite.rs:103-198, mul_many_rec literally: one input is glwe_lsh by offset_unary; two are one multiplication; otherwise the
    halves [0, len/2) and [len/2, len) into scratch ciphertexts of k = min effective_k - ceil_log2(len) log_delta (saturating), left
    first, then their product."""
    name = "mul_many"
    if len(inputs) == 0:
        raise CKKSError("ckks_mul_many: inputs must contain at least one ciphertext")
    plan = MulManyPlan(name, cols=dst.cols)
    live = []                                                             # slot -> in use

    def take(limbs):
        for s, used in enumerate(live):
            if not used and plan.slot_limbs[s] == limbs:
                live[s] = True
                return s
        live.append(True)
        plan.slot_limbs.append(limbs)
        return len(live) - 1

    def rec(out_ref, out: Ct, lo: int, hi: int):
        """writes the node(s) that leave the product of inputs[lo:hi] in `out`; returns out with its metadata"""
        xs = inputs[lo:hi]
        if any(c.log_delta != xs[0].log_delta for c in xs):
            raise CKKSError("ckks_mul_many: all inputs must have the same log_delta")
        for c in xs:
            _same_layout(name, out, c)
        if len(xs) == 1:
            offset = offset_unary(out, xs[0])
            out.log_delta = xs[0].log_delta
            out.log_budget = checked_log_budget_sub("ckks_mul_many", xs[0].log_budget, offset)
            plan.nodes.append(MulManyNode("lsh", out_ref, ("in", lo), None, Ct(out.base2k, out.size, out.log_delta, out.log_budget, out.cols), offset))
            return out
        if len(xs) == 2:
            a_ref, b_ref, a, b = ("in", lo), ("in", lo + 1), xs[0], xs[1]
            freed = ()
        else:
            mid = len(xs) // 2
            log_delta = xs[0].log_delta
            layouts = []
            for part in (xs[:mid], xs[mid:]):
                k = max(min(c.effective_k for c in part) - ceil_log2(len(part)) * log_delta, 0)
                layouts.append(-(-k // out.base2k))
            # take_glwe(left), take_glwe(right), then the two recursions on what is left of the scratch (composite.rs:154-160)
            ls, rs = take(layouts[0]), take(layouts[1])
            a = rec(("slot", ls), Ct(out.base2k, layouts[0], 0, 0, out.cols), lo, lo + mid)
            b = rec(("slot", rs), Ct(out.base2k, layouts[1], 0, 0, out.cols), lo + mid, hi)
            a_ref, b_ref, freed = ("slot", ls), ("slot", rs), (ls, rs)
        mul = _mul_plan(name, out, a, b, ("a", "b"))
        mul.apply_meta(out)
        plan.nodes.append(MulManyNode("mul", out_ref, a_ref, b_ref, Ct(out.base2k, out.size, out.log_delta, out.log_budget, out.cols), 0, mul))
        for s in freed:
            live[s] = False
        return out

    top = rec("dst", Ct(dst.base2k, dst.size, 0, 0, dst.cols), 0, len(inputs))
    plan.log_delta, plan.log_budget = top.log_delta, top.log_budget
    return plan


DOT_MAX_PAIRS = 64       # pairs of one pz_glwe_tensor_dot_relinearize_batched (kDotMaxPairs)


@dataclass
class DotCtPlan:
    """ckks_dot_product_ct (composite.rs:563-703).  branch:
    "single"   n = 1 (:585-587): muls[0] = plan_mul_into, ONE pz_glwe_tensor_mul_relinearize_acc_batched;
    "fallback" non-uniform log_delta on either side (:600-603): muls[0] = plan_mul_into(dst, a0, b0), muls[i] = the product of pair i into a
               scratch ciphertext of dst's layout joined to dst by ckks_add_assign_unsafe's branch (accumulate_unnormalized, :478-506) - one
               pz_glwe_tensor_mul_relinearize_acc_batched each, accumulate = 1, normalize = 0, and normalize = 1 on the last one: the closing
               glwe_normalize_assign;
    "fast"     (:605-702) on an unaligned side EVERY input is rescaled into a scratch ciphertext of ceil(target_eff_k / base2k) limbs (one
               pz_glwe_combine_batched each, rescales[side][i]); then ONE pz_glwe_tensor_dot_relinearize_batched: all pairs tensored into one
               accumulated GLWETensor of tensor_size limbs, one relinearization.  An aligned side is read in place, by the stride of its containers."""
    name: str
    branch: str
    log_delta: int = 0             # metadata of dst after the operation
    log_budget: int = 0
    muls: list = field(default_factory=list)
    n: int = 0
    cnv_offset: int = 0
    a_size: int = 0                # limbs of the operands: target_eff_k.div_ceil(base2k)
    b_size: int = 0
    a_effective_k: int = 0         # a_target_eff_k / b_target_eff_k
    b_effective_k: int = 0
    tensor_size: int = 0           # max(a_target_eff_k, b_target_eff_k).div_ceil(base2k): NOT the mul_into rule
    a_strides: list = field(default_factory=list)   # limbs of the containers the call reads, per pair
    b_strides: list = field(default_factory=list)
    rescales: dict = field(default_factory=dict)    # "a" / "b" -> [Plan per input] on an unaligned side
    cols: int = 2
    base2k: int = 0

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def scratch_offsets(self, batch: int, n: int):
        """byte offset of every rescaled copy, {(side, i): offset} (256-byte aligned), and the total"""
        offs, at = {}, 0
        for side, limbs in (("a", self.a_size), ("b", self.b_size)):
            for i in range(len(self.rescales.get(side, ()))):
                offs[(side, i)] = at
                at += -(-(batch * self.cols * limbs * n * 8) // 256) * 256
        return offs, at

    def scratch_bytes(self, batch: int, n: int) -> int:
        """the rescaled copies' footprint: 0 when both sides are aligned (and on the other branches)"""
        return self.scratch_offsets(batch, n)[1]

    def params(self, dst: Ct, tsk):
        """(pz_glwe_tensor_params, pz_glwe_op_params) of the fast branch's call; tsk: the prepared tensor key's (dnum, dsize, key_size, key_base2k)"""
        from .hal import GlweOpParams, GlweTensorParams
        dnum, dsize, key_size, key_base2k = tsk
        rank = dst.cols - 1
        tp = GlweTensorParams(rank=rank, a_size=self.a_size, b_size=self.b_size, ab_base2k=dst.base2k, a_effective_k=self.a_effective_k,
                              b_effective_k=self.b_effective_k, res_size=self.tensor_size, res_base2k=dst.base2k, cnv_offset=self.cnv_offset)
        rp = GlweOpParams(rank=rank, dnum=dnum, dsize=dsize, key_size=key_size, key_base2k=key_base2k, a_size=self.tensor_size,
                          a_base2k=dst.base2k, res_size=dst.size, res_base2k=dst.base2k, rank_out=rank)
        return tp, rp

    def launch(self, module, dst: Ct, batch: int, a_list, b_list, tsk_ptr=None, tsk=None, tmp=None):
        """dst.data / a_list[i].data / b_list[i].data / tsk_ptr: device pointers; tsk = (dnum, dsize, key_size, key_base2k) of the prepared
        tensor key; tmp: a device pointer to scratch_bytes(batch, module.n()) bytes (fast branch with an unaligned side only)."""
        if len(a_list) != self.n or len(b_list) != self.n:
            raise CKKSError(f"{self.name}: planned for {self.n} pairs")
        if self.branch != "fast":
            for i, p in enumerate(self.muls):
                tp, rp = p.params(dst, tsk)
                module.glwe_tensor_mul_relinearize_acc_batched(dst.data, a_list[i].data, b_list[i].data, tsk_ptr, tp, rp, "apply", batch,
                                                               a_stride=p.a_stride, b_stride=p.b_stride, accumulate=p.join is not None,
                                                               join=p.join or PLAIN, k=p.k, sign=1, normalize=i == len(self.muls) - 1)
            self.apply_meta(dst)
            return
        offs, total = self.scratch_offsets(batch, module.n())
        if total and tmp is None:
            raise CKKSError(f"{self.name}: needs {total} bytes of scratch for the rescaled inputs")
        base = 0 if tmp is None else (tmp.value if hasattr(tmp, "value") else int(tmp))
        ptrs = {"a": [x.data for x in a_list], "b": [x.data for x in b_list]}
        for side, xs, limbs in (("a", a_list, self.a_size), ("b", b_list, self.b_size)):       # :643-654: the a side first
            for i, rs in enumerate(self.rescales.get(side, ())):
                out = Ct(dst.base2k, limbs, 0, 0, dst.cols, base + offs[(side, i)])
                rs.launch(module, out, batch, a=xs[i])
                ptrs[side][i] = out.data
        tp, rp = self.params(dst, tsk)
        module.glwe_tensor_dot_relinearize_batched(dst.data, ptrs["a"], ptrs["b"], tsk_ptr, tp, rp, batch, a_strides=self.a_strides,
                                                   b_strides=self.b_strides)
        self.apply_meta(dst)


def plan_dot_product_ct(dst: Ct, a_list, b_list) -> DotCtPlan:
    """composite.rs:563-703, literally: check_lengths, ensure_accumulation_fits, n = 1 -> ckks_mul_into; non-uniform log_delta -> the
    product of pair 0 into dst and accumulate_unnormalized over the others; otherwise the fast branch: align every side to its lowest
    log_budget, tensor all pairs into one accumulated tensor, relinearize once."""
    name = "dot_product_ct"
    if len(a_list) == 0:                                                  # check_lengths, :468-476
        raise CKKSError(f"ckks_{name}: inputs must contain at least one pair")
    if len(a_list) != len(b_list):
        raise CKKSError(f"ckks_{name}: length mismatch between ct vector ({len(a_list)}) and weight vector ({len(b_list)})")
    n = len(a_list)
    _ensure_accumulation_fits(f"ckks_{name}", dst, n)                     # :583
    for x in (*a_list, *b_list):
        _same_layout(name, dst, x)
    if n == 1:                                                            # :585-587
        p = plan_mul_into(dst, a_list[0], b_list[0])
        return DotCtPlan(name, "single", p.log_delta, p.log_budget, [p], 1, cols=dst.cols, base2k=dst.base2k)
    a_min_lhr = min(c.log_budget for c in a_list)                         # :589-598
    b_min_lhr = min(c.log_budget for c in b_list)
    uniform_ld = all(c.log_delta == a_list[0].log_delta for c in a_list) and all(c.log_delta == b_list[0].log_delta for c in b_list)
    a_aligned = uniform_ld and all(c.log_budget == a_min_lhr for c in a_list)
    b_aligned = uniform_ld and all(c.log_budget == b_min_lhr for c in b_list)
    if not uniform_ld:                                                    # :600-603
        first = plan_mul_into(dst, a_list[0], b_list[0])
        acc = Ct(dst.base2k, dst.size, first.log_delta, first.log_budget, dst.cols)
        muls = [first]
        for i in range(1, n):                                             # accumulate_unnormalized: mul_into(tmp), add_assign_unsafe(dst, tmp)
            p = plan_mul_add_ct(acc, a_list[i], b_list[i])
            p.name = name
            p.apply_meta(acc)
            muls.append(p)
        return DotCtPlan(name, "fallback", acc.log_delta, acc.log_budget, muls, n, cols=dst.cols, base2k=dst.base2k)
    B = dst.base2k
    a_ld, b_ld = a_list[0].log_delta, b_list[0].log_delta                 # :605-608
    a_target_eff_k, b_target_eff_k = a_min_lhr + a_ld, b_min_lhr + b_ld
    a_size, b_size = -(-a_target_eff_k // B), -(-b_target_eff_k // B)     # the scratch layouts, :610-621
    rescales = {}
    for side, aligned, xs, min_lhr, limbs in (("a", a_aligned, a_list, a_min_lhr, a_size), ("b", b_aligned, b_list, b_min_lhr, b_size)):
        if not aligned:                                                   # :643-654: every input of the side, shift 0 included
            rescales[side] = [plan_rescale_into(Ct(B, limbs, 0, 0, dst.cols), x, x.log_budget - min_lhr) for x in xs]
    res_log_delta = min(a_ld, b_ld)                                       # :656-661
    lhr0 = checked_mul_ct_log_budget(name, a_min_lhr, b_min_lhr, a_ld, b_ld)
    res_offset = max(lhr0 + res_log_delta - dst.max_k, 0)
    res_log_budget = checked_log_budget_sub(name, lhr0, res_offset)
    cnv_offset = max(a_target_eff_k, b_target_eff_k) + res_offset
    tensor_size = -(-max(a_target_eff_k, b_target_eff_k) // B)            # :663-669
    if a_size < 1 or b_size < 1:
        raise CKKSError(f"{name}: an operand of effective_k {min(a_target_eff_k, b_target_eff_k)} has no limb")

    def strides(side, xs, limbs):
        """a rescaled side is read from its scratch copies; an aligned side in place: every input has effective_k = the target, in a
        container that may hold more limbs (never fewer: _operand_size)"""
        if side in rescales:
            return [limbs] * n
        for x in xs:
            _operand_size(name, x)
        return [x.size for x in xs]
    a_strides, b_strides = strides("a", a_list, a_size), strides("b", b_list, b_size)
    if n > DOT_MAX_PAIRS:
        raise CKKSError(f"{name}: {n} pairs in one pz_glwe_tensor_dot_relinearize_batched (at most {DOT_MAX_PAIRS})")
    return DotCtPlan(name, "fast", res_log_delta, res_log_budget, [], n, cnv_offset, a_size, b_size, a_target_eff_k, b_target_eff_k, tensor_size,
                     a_strides, b_strides, rescales, dst.cols, B)


@dataclass
class CompactPlan:
    """ckks_compact_limbs into another container (layouts/ciphertext.rs:216-232: reallocate to effective_k.div_ceil(base2k) limbs): one
    pz_vec_znx_copy_batched per column.  For callers who want the memory back; the products above read a larger container in place."""
    name: str
    size: int
    log_delta: int
    log_budget: int

    def apply_meta(self, dst: Ct):
        dst.log_delta, dst.log_budget = self.log_delta, self.log_budget

    def launch(self, module, dst: Ct, batch: int, src: Ct):
        for c in range(dst.cols):
            module.vec_znx_copy_batched(batch, dst.data, dst.cols, dst.size, c, src.data, src.cols, src.size, c)
        self.apply_meta(dst)


def plan_compact_limbs_copy(dst: Ct, src: Ct) -> CompactPlan:
    """dst: a container of exactly src.effective_k.div_ceil(base2k) limbs; takes src's first limbs and its metadata."""
    _same_layout("compact_limbs", dst, src)
    size = _operand_size("compact_limbs", src)
    if dst.size != size:
        raise CKKSError(f"compact_limbs: dst has {dst.size} limbs, effective_k {src.effective_k} / base2k {src.base2k} rounds up to {size}")
    return CompactPlan("compact_limbs_copy", size, src.log_delta, src.log_budget)
