"""What a CKKS ciphertext, plaintext and constant MEAN, and what every linear CKKS operation must make of them: stated once, exactly, on
Python integers, from poulpy-ckks's layouts and its own test helpers - not from poulpy_amd/ckks.py, whose shift amounts, convolution offsets
and branch conditions appear nowhere below (only its Ct / Pt / Cst containers are imported), and not from the restatements
(tests/shift_oracle.py, tests/ckks_lincomb_oracle.py, tests/plain_oracle.py), which take those amounts from the plan under test.

Limbs x_j at base2k = B are the torus element T = sum_j x_j 2^-(j+1)B mod 1, normalized or not.  Then (layouts/plaintext/{vec,cst}.rs,
leveled/default/pt_znx.rs:17-36, lib.rs:52-90, leveled/default/mul.rs:498-513)

    value(ct)  = T 2^log_budget                 defined mod 2^log_budget
    value(pt)  = T 2^(max_k - log_delta)
    c          = v 2^-log_delta                 the digits of a constant hold v = round(c 2^log_delta) at k = min_k, |v| < 2^(min_k - 1)

and every operation computes, mod 2^(its output's log_budget): value(a) +- value(b), -value(a), 2^+-bits value(a), value(a) +- value(pt)
(column 0 only), value(a) (re + im X^(N/2)), sum_i value(a_i) c_i, phi_p(value(a)).  Nothing is lost except by rounding at the destination's
last limb, so a result is wrong unless it lies within a few 2^-dst.max_k (ulps) of the expectation: `allow` below, from metadata alone.

The allowance.  A digit stream that is brought into the destination with bits falling below the destination's last limb is rounded there:
the dropped part is a tail of balanced digits, at most HALF(B) = 0.5 / (1 - 2^-B) ulp (0.5 ulp but for the digits below the first dropped
one: the one term this derivation adds to the plain count of 0.5 per stream; it stays below 0.5 (1 + 2^-11) for B >= 12).  A stream none of
whose bits fall below costs nothing.  A product by a constant is rounded once per part (re, im) at its own budget b_i; joined into a result
of budget b_out <= b_i it is shifted up by b_i - b_out bits and its rounding with it: HALF 2^(b_i - b_out) per part.  Steps that follow each
other on one destination carry the error along: what was within e ulps at budget b is within e 2^(b - b') at the later budget b' <= b.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from poulpy_amd.ckks import Cst, Ct, Pt  # noqa: F401  (containers only)
from tests import fhe_sk as fs

FINE = 1024            # the common precision of every expectation: torus numerators over 2^FINE

Outcome = namedtuple("Outcome", "want log_delta log_budget allow")     # want: (cols, n) Python ints over 2^FINE


class Refused(Exception):
    """The reference returns a CKKSCompositionError (src/error.rs) for these inputs; .kind names the variant."""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


CAPACITY, BASE2K, ALIGNMENT, UNDERFLOW, LENGTHS = ("InsufficientHomomorphicCapacity", "PlaintextBase2KMismatch", "PlaintextAlignmentImpossible",
                                                   "MultiplicationPrecisionUnderflow", "lengths")


# ---- numbers ----------------------------------------------------------------------------------------------------------------------------
def _arr(x):
    """the (size, cols, n) limbs of a container, of a VecZnx, or the array itself"""
    while not isinstance(x, np.ndarray):
        x = x.data
    return x


class Val:
    """num 2^-e, num a (cols, n) array of Python ints"""

    def __init__(self, num, e):
        self.num, self.e = num, int(e)


def _at(v: Val, e: int):
    assert e >= v.e
    return v.num * (1 << (e - v.e))


def vsum(x: Val, y: Val, sign=1) -> Val:
    e = max(x.e, y.e)
    return Val(_at(x, e) + sign * _at(y, e), e)


def place(v: Val, log_budget: int):
    """value -> torus numerator over 2^FINE of value 2^-log_budget mod 1"""
    sh = FINE - v.e - log_budget
    assert sh >= 0, "FINE is too coarse for this case"
    return (v.num * (1 << sh)) % (1 << FINE)


def torus(limbs, base2k):
    """T of the limbs (axis 0: limb 0 most significant) as numerators over 2^FINE"""
    limbs = _arr(limbs)
    bits = limbs.shape[0] * base2k
    assert bits <= FINE
    return (fs.to_int(limbs, base2k) * (1 << (FINE - bits))) % (1 << FINE)


def max_k(x) -> int:                       # poulpy-core layouts/lwe.rs:23-25
    return x.size * x.base2k


def effective_k(ct) -> int:                # lib.rs:87-89
    return ct.log_delta + ct.log_budget


def value_ct(ct) -> Val:
    return Val(fs.to_int(_arr(ct), ct.base2k), max_k(ct) - ct.log_budget)


def value_pt(pt, cols=1) -> Val:
    """the plaintext's value in column 0 of `cols` columns"""
    num = np.zeros((cols,) + _arr(pt).shape[2:], dtype=object)
    num[0] = fs.to_int(_arr(pt), pt.base2k)[0]
    return Val(num, pt.log_delta)


def cst_k(base2k, log_delta, log_budget) -> int:
    """lib.rs:79-81: the precision a constant's digits are written at, ceil((log_delta + log_budget) / base2k) limbs"""
    return -(-(log_delta + log_budget) // base2k) * base2k


def cst_value(digits, base2k, log_delta, log_budget) -> int:
    """v of a constant's digits: the constant is v 2^-log_delta"""
    digits = [int(d) for d in digits]
    assert len(digits) * base2k == cst_k(base2k, log_delta, log_budget), "a constant holds min_k / base2k digits"
    v = 0
    for d in digits:
        v = (v << base2k) + d
    assert abs(v) < 1 << (len(digits) * base2k - 1)
    return v


def encode_cst(v, base2k, log_delta, log_budget):
    """to_znx (layouts/plaintext/cst.rs:114-148): the balanced digits of v at k = min_k, most significant first"""
    k = cst_k(base2k, log_delta, log_budget)
    assert abs(int(v)) < 1 << (k - 1)
    half, mask, x, out = 1 << (base2k - 1), (1 << base2k) - 1, int(v), []
    for _ in range(k // base2k):
        d = ((x + half) & mask) - half
        out.append(d)
        x = (x - d) >> base2k
    return np.array(out[::-1], dtype=np.int64)


def vtimes(x: Val, cst, base2k) -> Val:
    """value (re + im X^(N/2)) with the constant's own metadata"""
    n = x.num.shape[-1]
    num = np.zeros_like(x.num)
    if cst.re is not None:
        num = num + x.num * cst_value(cst.re, base2k, cst.log_delta, cst.log_budget)
    if cst.im is not None:
        num = num + fs.rotate(x.num.copy(), n // 2) * cst_value(cst.im, base2k, cst.log_delta, cst.log_budget)
    return Val(num, x.e + cst.log_delta)


def parts(cst) -> int:
    return (cst.re is not None) + (cst.im is not None)


def deviation_ulps(got, want, dst_size, base2k) -> float:
    """max |T(got) - want| centred mod 1, in units of 2^-(dst_size base2k); got: (size, cols, n) limbs, want: numerators over 2^FINE"""
    d = (torus(got, base2k) - want) % (1 << FINE)
    d = np.where(d >= 1 << (FINE - 1), d - (1 << FINE), d)
    worst = max(abs(int(x)) for x in d.reshape(-1))
    ulp = 1 << (FINE - dst_size * base2k)
    return worst / ulp


# ---- the allowance ----------------------------------------------------------------------------------------------------------------------
def HALF(base2k) -> float:
    return 0.5 / (1.0 - 2.0 ** -base2k)


def _stream(dst, scale, x_max_k, log_budget) -> float:
    """a stream of x_max_k bits whose value is T 2^scale, brought into dst at log_budget: shifted up by scale - log_budget bits"""
    return HALF(dst.base2k) if x_max_k - (scale - log_budget) > max_k(dst) else 0.0


def _ct_stream(dst, x, log_budget) -> float:
    return _stream(dst, x.log_budget, max_k(x), log_budget)


def _pt_stream(dst, pt, log_budget) -> float:
    return _stream(dst, max_k(pt) - pt.log_delta, max_k(pt), log_budget)


def carried(allow, budget_before, budget_after) -> float:
    assert budget_after <= budget_before
    return allow * 2.0 ** (budget_before - budget_after)


# ---- the reference's offsets and refusals (layouts/ciphertext.rs:270-283, error.rs) -----------------------------------------------------
def _sub(kind, available, required):
    if required > available:
        raise Refused(kind)
    return available - required


def _offset_unary(dst, a):
    return max(effective_k(a) - max_k(dst), 0)


def _offset_binary(dst, a, b):
    return max(min(effective_k(a), effective_k(b)) - max_k(dst), 0)


def _same_base(dst, *xs):
    for x in xs:
        assert x.base2k == dst.base2k and x.cols == dst.cols, "the cases keep to one base and one rank (poulpy-core asserts it)"


# ---- output metadata: helpers.rs:861-891, default/{add,sub,neg,pow2,rescale}.rs ---------------------------------------------------------
def meta_unary(dst, a):
    """assert_unary_output_meta"""
    return a.log_delta, _sub(CAPACITY, a.log_budget, _offset_unary(dst, a))


def meta_binary(dst, a, b):
    """assert_binary_output_meta"""
    return min(a.log_delta, b.log_delta), _sub(CAPACITY, min(a.log_budget, b.log_budget), _offset_binary(dst, a, b))


def meta_binary_assign(dst, a):
    """add.rs:143-144, sub.rs:143-144 (the suite's cases have equal log_delta, where its max() and the code's min() agree)"""
    return min(dst.log_delta, a.log_delta), min(dst.log_budget, a.log_budget)


def meta_mul_pt(dst, a, c):
    """assert_mul_pt_output_meta, for c.log_delta <= a.log_delta (every case of the suite; mul.rs:498-513 subtracts c.log_delta and keeps
    a.log_delta, which is the same thing there)"""
    if c.log_delta > a.log_budget:
        raise Refused(UNDERFLOW)
    assert c.log_delta <= a.log_delta
    log_budget = a.log_budget - min(a.log_delta, c.log_delta)
    log_delta = max(a.log_delta, c.log_delta)
    return log_delta, _sub(CAPACITY, log_budget, max(log_budget + log_delta - max_k(dst), 0))


def meta_div_pow2(dst, a, bits):
    """pow2.rs:57-74"""
    return a.log_delta + bits, _sub(CAPACITY, a.log_budget, bits + _offset_unary(dst, a))


def meta_rescale(src, k):
    """rescale.rs:23-55"""
    return src.log_delta, _sub(CAPACITY, src.log_budget, k)


def align(a, b):
    """rescale.rs:57-70 -> (which one is rescaled in place: "a" | "b", by how many bits)"""
    return ("b", b.log_budget - a.log_budget) if a.log_budget < b.log_budget else ("a", a.log_budget - b.log_budget)


def _pt_checks(dst, log_budget, pt):
    if pt.base2k != dst.base2k:
        raise Refused(BASE2K)
    if log_budget + pt.log_delta < max_k(pt):
        raise Refused(ALIGNMENT)


# ---- one outcome per operation ----------------------------------------------------------------------------------------------------------
def outcome_add(dst, a, b, sub=False) -> Outcome:
    """add.rs / sub.rs, the _unsafe forms alike: value(a) +- value(b)"""
    _same_base(dst, a, b)
    ld, lb = meta_binary(dst, a, b)
    v = vsum(value_ct(a), value_ct(b), -1 if sub else 1)
    return Outcome(place(v, lb), ld, lb, _ct_stream(dst, a, lb) + _ct_stream(dst, b, lb))


def outcome_add_assign(dst, a, sub=False) -> Outcome:
    _same_base(dst, a)
    ld, lb = meta_binary_assign(dst, a)
    v = vsum(value_ct(dst), value_ct(a), -1 if sub else 1)
    return Outcome(place(v, lb), ld, lb, _ct_stream(dst, dst, lb) + _ct_stream(dst, a, lb))


def outcome_add_many(dst, inputs) -> Outcome:
    """composite.rs:63-93: one input is a copy into dst; more are add_into_unsafe of the first two, add_assign_unsafe of the others, one
    normalization"""
    if not inputs:
        raise Refused(LENGTHS)
    _same_base(dst, *inputs)
    if len(inputs) == 1:
        return outcome_mul_pow2(dst, inputs[0], 0)
    if dst.base2k >= 64 or len(inputs) > 1 << (63 - dst.base2k):
        raise Refused(LENGTHS)
    ld, lb = meta_binary(dst, inputs[0], inputs[1])
    v = vsum(value_ct(inputs[0]), value_ct(inputs[1]))
    allow = _ct_stream(dst, inputs[0], lb) + _ct_stream(dst, inputs[1], lb)
    for x in inputs[2:]:
        nb = min(lb, x.log_budget)
        allow = carried(allow, lb, nb) + _ct_stream(dst, x, nb)
        v, ld, lb = vsum(v, value_ct(x)), min(ld, x.log_delta), nb
    return Outcome(place(v, lb), ld, lb, allow)


def outcome_neg(dst, a=None) -> Outcome:
    """neg.rs; a = None: the assign form, metadata untouched"""
    src = dst if a is None else a
    ld, lb = (dst.log_delta, dst.log_budget) if a is None else meta_unary(dst, a)
    v = value_ct(src)
    return Outcome(place(Val(-v.num, v.e), lb), ld, lb, _ct_stream(dst, src, lb))


def outcome_mul_pow2(dst, a=None, bits=0) -> Outcome:
    """pow2.rs:25-55: value 2^bits; the assign form keeps the metadata"""
    src = dst if a is None else a
    ld, lb = (dst.log_delta, dst.log_budget) if a is None else meta_unary(dst, a)
    v = value_ct(src)
    return Outcome(place(Val(v.num * (1 << bits), v.e), lb), ld, lb, _stream(dst, src.log_budget + bits, max_k(src), lb))


def outcome_div_pow2(dst, a=None, bits=0) -> Outcome:
    """pow2.rs:57-85: value 2^-bits, log_delta + bits (into), log_budget - bits; the assign form touches no limb"""
    src = dst if a is None else a
    ld, lb = (dst.log_delta, _sub(CAPACITY, dst.log_budget, bits)) if a is None else meta_div_pow2(dst, a, bits)
    v = value_ct(src)
    return Outcome(place(Val(v.num, v.e + bits), lb), ld, lb, _stream(dst, src.log_budget - bits, max_k(src), lb))


def outcome_rescale(dst, a=None, k=0) -> Outcome:
    """rescale.rs: the value stays, log_budget - k"""
    src = dst if a is None else a
    ld, lb = meta_rescale(src, k)
    return Outcome(place(value_ct(src), lb), ld, lb, _ct_stream(dst, src, lb))


def outcome_add_pt(dst, a, pt, sub=False) -> Outcome:
    """add.rs:148-210, sub.rs alike, pt_znx.rs:17-57: value(a) +- value(pt) in column 0; a = None: the assign form"""
    src = dst if a is None else a
    ld, lb = (dst.log_delta, dst.log_budget) if a is None else meta_unary(dst, a)
    _pt_checks(dst, lb, pt)
    v = vsum(value_ct(src), value_pt(pt, dst.cols), -1 if sub else 1)
    return Outcome(place(v, lb), ld, lb, _ct_stream(dst, src, lb) + _pt_stream(dst, pt, lb))


def outcome_mul_cst(dst, a, cst) -> Outcome:
    """mul.rs:342-407: value(a) (re + im X^(N/2)); a = None: the assign form; a constant with neither part: zero"""
    src = dst if a is None else a
    ld, lb = meta_mul_pt(dst, src, cst)
    return Outcome(place(vtimes(value_ct(src), cst, dst.base2k), lb), ld, lb, parts(cst) * HALF(dst.base2k))


def outcome_mul_add_cst(dst, a, cst, sub=False) -> Outcome:
    """composite.rs:290-308 / :423-441: dst +- value(a) c through a scratch ciphertext of dst's layout; an empty constant leaves dst and
    its metadata alone"""
    if cst.re is None and cst.im is None:
        return Outcome(place(value_ct(dst), dst.log_budget), dst.log_delta, dst.log_budget, 0.0)
    _same_base(dst, a)
    pd, pb = meta_mul_pt(dst, a, cst)
    ld, lb = min(dst.log_delta, pd), min(dst.log_budget, pb)
    v = vsum(value_ct(dst), vtimes(value_ct(a), cst, dst.base2k), -1 if sub else 1)
    return Outcome(place(v, lb), ld, lb, carried(parts(cst) * HALF(dst.base2k), pb, lb))


def outcome_dot_cst(dst, ops, csts) -> Outcome:
    """composite.rs:760-784: sum_i value(a_i) c_i, every product at its own budget, the sum at the least"""
    if len(ops) == 0 or len(ops) != len(csts) or dst.base2k >= 64 or len(ops) > 1 << (63 - dst.base2k):
        raise Refused(LENGTHS)
    _same_base(dst, *ops)
    metas = [meta_mul_pt(dst, a, c) for a, c in zip(ops, csts)]
    ld, lb = min(m[0] for m in metas), min(m[1] for m in metas)
    v = None
    for a, c in zip(ops, csts):
        t = vtimes(value_ct(a), c, dst.base2k)
        v = t if v is None else vsum(v, t)
    allow = sum(carried(parts(c) * HALF(dst.base2k), m[1], lb) for c, m in zip(csts, metas))
    return Outcome(place(v, lb), ld, lb, allow)


def outcome_automorphism(dst, a, p) -> Outcome:
    """rotate.rs:23-56, conjugate.rs: phi_p(value(a)) (conjugation: p = 2N - 1), before the key switch's noise"""
    _same_base(dst, a)
    ld, lb = meta_unary(dst, a)
    v = value_ct(a)
    return Outcome(place(Val(fs.automorphism(v.num, p), v.e), lb), ld, lb, _ct_stream(dst, a, lb))


def _want(f):
    def g(*args, **kw):
        return f(*args, **kw).want
    g.__name__, g.__doc__ = f.__name__.replace("outcome", "expect"), f.__doc__
    return g


# expect_<op>: the expected torus numerators alone
expect_add, expect_add_assign, expect_add_many = _want(outcome_add), _want(outcome_add_assign), _want(outcome_add_many)
expect_neg, expect_mul_pow2, expect_div_pow2 = _want(outcome_neg), _want(outcome_mul_pow2), _want(outcome_div_pow2)
expect_rescale, expect_add_pt, expect_mul_cst = _want(outcome_rescale), _want(outcome_add_pt), _want(outcome_mul_cst)
expect_mul_add_cst, expect_dot_cst, expect_automorphism = _want(outcome_mul_add_cst), _want(outcome_dot_cst), _want(outcome_automorphism)
