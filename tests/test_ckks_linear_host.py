"""CPU checks of the accumulating-shift restatement (tests/shift_oracle.py) against the C oracle where the two overlap, and of the CKKS
mapping in poulpy_amd/ckks.py on cases derived by hand from poulpy-ckks src/leveled/default/*.rs and src/error.rs."""
import os
import re

import numpy as np
import pytest

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH, RAW, RSH, Ct, Pt
from poulpy_amd.layouts import VecZnx
from tests import shift_oracle as so
from tests.helpers import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


def _vz(rng, cols, size, wide):
    return VecZnx(N, cols, size).fill_uniform(63 if wide else 12, rng)


SHAPES = [(b, k, rs, as_) for b in (12, 17, 50) for rs, as_ in ((3, 5), (4, 4), (6, 2)) for k in (0, 1, b - 1, b, b + 1, 3 * b + 2, 7 * b)]


@pytest.mark.parametrize("base2k,k,res_size,a_size", SHAPES)
@pytest.mark.parametrize("wide", [False, True])
def test_accumulating_shifts_into_zeros_are_the_oracle_shifts(ref, base2k, k, res_size, a_size, wide):
    rng = seeded(base2k * 1000 + k * 10 + res_size)
    a = _vz(rng, 2, a_size, wide)
    for name in ("lsh", "rsh"):
        want = VecZnx(N, 2, res_size).fill_uniform(20, rng)
        getattr(ref, f"vec_znx_{name}")(base2k, k, want, 1, a, 0)
        acc = so.vec_znx_lsh_acc if name == "lsh" else so.vec_znx_rsh_acc
        got = VecZnx(N, 2, res_size)
        acc(base2k, k, got, 1, a, 0)
        assert np.array_equal(got.data[:, 1], want.data[:, 1]), name
        neg = VecZnx(N, 2, res_size)
        acc(base2k, k, neg, 1, a, 0, sub=True)
        # sub into zeros = the negation of the shift's digits, except that rsh_sub renormalizes the limbs above the shifted digits with
        # the negated carry (shift.rs, vec_znx_rsh_sub): there the digits are the normalization of -carry, not -(the digits of +carry)
        if name == "lsh":
            assert np.array_equal(neg.data[:, 1], -want.data[:, 1])
        assert not neg.data[:, 0].any() and not got.data[:, 0].any()


def test_lsh_early_return_and_min_size(ref):
    rng = seeded(3)
    a = _vz(rng, 1, 4, False)
    res = VecZnx(N, 1, 3).fill_uniform(30, rng)
    before = res.data.copy()
    so.vec_znx_lsh_acc(12, 12 * 4, res, 0, a, 0)        # steps >= max(res_size, a_size): untouched (shift.rs:92-100)
    assert np.array_equal(res.data, before)
    so.vec_znx_lsh_acc(12, 12 * 3, res, 0, a, 0)        # steps = 3 < 4: min_size = min(3, 1) = 1, limbs 1.. untouched
    assert np.array_equal(res.data[1:], before[1:]) and not np.array_equal(res.data[0], before[0])


def test_header_library_and_binding_carry_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "poulpy_hip.h")).read()
    names = ["pz_glwe_combine_batched", "pz_vec_znx_lsh_add_into_batched", "pz_vec_znx_lsh_sub_batched", "pz_vec_znx_rsh_add_into_batched",
             "pz_vec_znx_rsh_sub_batched"]
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr), n
    assert "pz_glwe_term" in hdr and "PZ_TERM_RSH" in hdr
    from poulpy_amd import hal
    lib = hal.load_library()
    for n in names:
        assert hasattr(lib, n), n
    assert {f for f, _ in hal.GlweTerm._fields_} == {"a_size", "k", "base2k", "kind", "sign", "col0_only", "shared"}


def _t(p):
    return [(t.src, t.kind, t.k, t.sign) for t in p.terms]


def test_add_into_branches_offsets_and_metadata():
    # dst 4 limbs of 12 bits: max_k 48.  a: delta 20 + budget 30 = 50, b: 20 + 30 -> offset_binary = 50 - 48 = 2
    dst, a, b = Ct(12, 4, 0, 0), Ct(12, 5, 20, 30), Ct(12, 5, 20, 30)
    p = ckks.plan_add_into(dst, a, b)
    assert p.offset == 2 and _t(p) == [("a", LSH, 2, 1), ("b", LSH, 2, 1)] and (p.log_delta, p.log_budget) == (20, 28) and p.normalize
    big = Ct(12, 8, 0, 0)                               # offset 0, equal budgets: glwe_add_into
    p = ckks.plan_add_into(big, a, b, normalize=False)
    assert _t(p) == [("a", RAW, 0, 1), ("b", RAW, 0, 1)] and p.log_budget == 30 and not p.normalize
    lo = Ct(12, 5, 18, 25)                              # a.budget < b.budget: lsh(a, off) + lsh_add(b, Δ + off)
    p = ckks.plan_add_into(big, lo, b)
    assert _t(p) == [("a", LSH, 0, 1), ("b", LSH, 5, 1)] and (p.log_delta, p.log_budget) == (18, 25)
    p = ckks.plan_add_into(big, b, lo)                  # a.budget > b.budget: lsh(b, off) + lsh_add(a, Δ + off)
    assert _t(p) == [("b", LSH, 0, 1), ("a", LSH, 5, 1)]
    p = ckks.plan_add_into(big, b, lo, sub=True)        # sub.rs:97-98: a by Δ + off, b by off
    assert _t(p) == [("a", LSH, 5, 1), ("b", LSH, 0, -1)]
    p = ckks.plan_add_into(dst, b, lo, sub=True)        # offset = min(50, 43) - 48 = 0 -> still the shifted branch (budgets differ)
    assert p.offset == 0 and _t(p) == [("a", LSH, 5, 1), ("b", LSH, 0, -1)]
    with pytest.raises(ckks.CKKSError):                 # budget 3 - offset 50 - 24
        ckks.plan_add_into(Ct(12, 2, 0, 0), Ct(12, 5, 47, 3), Ct(12, 5, 47, 3))


def test_assign_forms_neg_pow2_rescale():
    dst, a = Ct(12, 4, 20, 30), Ct(12, 4, 21, 25)
    p = ckks.plan_add_assign(dst, a)                    # dst budget higher: lsh_assign(dst, 5) then add_assign(a)
    assert _t(p) == [("dst", LSH, 5, 1), ("a", RAW, 0, 1)] and (p.log_delta, p.log_budget) == (20, 25)
    p = ckks.plan_add_assign(a, dst, sub=True)          # dst budget lower: lsh_sub(a, Δ)
    assert _t(p) == [("dst", RAW, 0, 1), ("a", LSH, 5, -1)]
    p = ckks.plan_add_assign(dst, Ct(12, 4, 20, 30))
    assert _t(p) == [("dst", RAW, 0, 1), ("a", RAW, 0, 1)]
    src = Ct(12, 5, 20, 40)                             # effective_k 60, dst max_k 48: offset 12
    p = ckks.plan_neg_into(Ct(12, 4, 0, 0), src)
    assert _t(p) == [("a", LSH, 12, -1)] and p.log_budget == 28 and not p.normalize
    p = ckks.plan_neg_into(Ct(12, 5, 0, 0), src)
    assert _t(p) == [("a", RAW, 0, -1)] and p.log_budget == 40
    assert _t(ckks.plan_neg_assign(src)) == [("dst", RAW, 0, -1)]
    p = ckks.plan_mul_pow2_into(Ct(12, 4, 0, 0), src, 3)
    assert _t(p) == [("a", LSH, 15, 1)] and p.log_budget == 28
    p = ckks.plan_div_pow2_into(Ct(12, 4, 0, 0), src, 3)
    assert _t(p) == [("a", LSH, 12, 1)] and (p.log_delta, p.log_budget) == (23, 25)
    p = ckks.plan_div_pow2_assign(src, 7)
    assert p.terms == [] and (p.log_delta, p.log_budget) == (20, 33)
    assert _t(ckks.plan_mul_pow2_assign(src, 9)) == [("dst", LSH, 9, 1)]
    p = ckks.plan_rescale_into(Ct(12, 4, 0, 0), src, 13)
    assert _t(p) == [("a", LSH, 13, 1)] and p.log_budget == 27
    with pytest.raises(ckks.CKKSError):
        ckks.plan_rescale_assign(src, 41)
    which, p = ckks.plan_align_assign(Ct(12, 4, 20, 10), Ct(12, 4, 20, 17))
    assert which == "b" and _t(p) == [("dst", LSH, 7, 1)] and p.log_budget == 10
    which, p = ckks.plan_align_assign(Ct(12, 4, 20, 17), Ct(12, 4, 20, 17))
    assert which == "a" and _t(p) == [("dst", LSH, 0, 1)]


def test_plaintext_alignment_and_refusals():
    dst, a = Ct(12, 4, 0, 0), Ct(12, 5, 20, 34)         # offset_unary 54 - 48 = 6, budget 28
    pt = Pt(12, 2, 20)                                  # max_k 24: available 28 + 20 = 48 -> rsh by 24
    p = ckks.plan_add_pt_into(dst, a, pt)
    assert _t(p) == [("a", LSH, 6, 1), ("pt", RSH, 24, 1)] and p.log_budget == 28 and p.pt_shift == 24
    p = ckks.plan_add_pt_assign(Ct(12, 4, 20, 10), Pt(12, 3, 30), sub=True)   # 10 + 30 - 36 = 4
    assert _t(p) == [("dst", RAW, 0, 1), ("pt", RSH, 4, -1)]
    with pytest.raises(ckks.CKKSError):                 # 10 + 20 < 36
        ckks.plan_add_pt_assign(Ct(12, 4, 20, 10), Pt(12, 3, 20))
    with pytest.raises(ckks.CKKSError):                 # ensure_base2k_match
        ckks.plan_add_pt_assign(Ct(12, 4, 20, 10), Pt(13, 3, 30))
    with pytest.raises(ckks.CKKSError):                 # one base2k for the GLWE operands
        ckks.plan_add_into(Ct(12, 4, 0, 0), Ct(12, 4, 20, 10), Ct(13, 4, 20, 10))


def test_oracle_sequences_match_the_plans_term_by_term(ref):
    """The host restatement of each CKKS sequence (shift_oracle.run) equals the plan's terms applied one after the other with the
    per-column primitives: the mapping the device kernel implements."""
    rng = seeded(11)
    B = 12
    cases = [(ckks.plan_add_into, ("a", "b"), (Ct(B, 4, 0, 0), Ct(B, 5, 20, 30), Ct(B, 5, 18, 25))),
             (lambda d, a, b: ckks.plan_add_into(d, a, b, sub=True), ("a", "b"), (Ct(B, 4, 0, 0), Ct(B, 5, 20, 30), Ct(B, 5, 18, 25))),
             (ckks.plan_add_assign, ("a",), (Ct(B, 4, 20, 30), Ct(B, 4, 21, 25)))]
    for mk, names, cts in cases:
        for c in cts:
            c.data = VecZnx(N, 2, c.size).fill_uniform(B, rng)
        dst, *ops = cts
        plan = mk(dst, *ops)
        want = dst.data.copy()
        so.run(ref, plan, Ct(B, dst.size, dst.log_delta, dst.log_budget, data=want), *[Ct(B, o.size, o.log_delta, o.log_budget, data=o.data) for o in ops])
        env = dict(zip(names, ops))
        env["dst"] = dst
        got = VecZnx(N, 2, dst.size)
        for t in plan.terms:
            src = env[t.src].data
            for col in range(2):
                if t.kind == RAW:
                    m = min(src.size, got.size)
                    got.data[:m, col] += t.sign * src.data[:m, col]
                else:
                    so.vec_znx_lsh_acc(B, t.k, got, col, src, col, sub=t.sign < 0)
        if plan.normalize:
            so.glwe_normalize_assign(ref, B, got)
        assert np.array_equal(got.data, want.data), plan.name
