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
    """CKKSPlaintextVecZnx: a VecZnx(1, size) at base2k with its log_delta."""
    base2k: int
    size: int
    log_delta: int
    data: object = None

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
