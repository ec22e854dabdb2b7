"""Inputs shared by tests/test_ckks_sum_host.py and tests/test_gpu_ckks_sum.py: random join chains for pz_glwe_sum_batched, and the
scenarios of the CKKS plans built on it (the reference's own cases from poulpy-ckks leveled/tests/test_suite/{add_many,mul,mul_add,mul_sub,
dot_product}.rs restated as layouts and metadata, plus unequal budgets that reach all three joins)."""
from __future__ import annotations

import numpy as np

from poulpy_amd import ckks
from poulpy_amd.ckks import LSH_ACC, LSH_TERM, PLAIN, Ct, Pt
from poulpy_amd.layouts import VecZnx


def fill(rng, v: VecZnx, base2k: int, normalized: bool):
    """normalized digits, or un-normalized limbs below 2^(base2k + 4) in magnitude"""
    h = 1 << (base2k - 1 if normalized else base2k + 3)
    v.data[...] = rng.integers(-h, h, v.data.shape, dtype=np.int64)
    return v


def random_shift(rng, base2k: int) -> int:
    """0 .. 3 base2k, with the multiples of base2k (no bit shift; 3 base2k: three whole limbs) drawn often"""
    return int(rng.choice([0, base2k, 2 * base2k, 3 * base2k])) if rng.random() < 0.3 else int(rng.integers(0, 3 * base2k + 1))


def random_chain(rng, n, cols, base2k, res_size, nterms, normalized=True, res: VecZnx | None = None, acc_shift=None, max_a=7, res_k=None):
    """terms (a, join, k, sign) for sum_chain.  res: term 0 is this container itself - a plain join, or with res_k a PZ_JOIN_LSH_TERM by
    res_k bits (its own shift moves it); acc_shift: None - random joins; False - no PZ_JOIN_LSH_ACC at all; True - at least one after
    term 0."""
    terms = []
    for u in range(nterms):
        join = int(rng.choice([PLAIN, LSH_TERM, LSH_ACC] if acc_shift is None or acc_shift else [PLAIN, LSH_TERM]))
        if acc_shift and u == min(1, nterms - 1):
            join = LSH_ACC
        k = 0 if join == PLAIN else random_shift(rng, base2k)
        sign = int(rng.choice([1, -1]))
        if u == 0 and res is not None:
            terms.append((res, PLAIN, 0, sign) if res_k is None else (res, LSH_TERM, res_k, sign))
            continue
        a = fill(rng, VecZnx(n, cols, int(rng.integers(1, max_a + 1))), base2k, normalized)
        terms.append((a, join, k, sign))
    return terms


def write_chain(f, base2k, res: VecZnx, terms, want: VecZnx):
    """one case of tests/cpp/test_sum_walk.cpp"""
    f.write("%d %d %d %d %d\n" % (res.n, res.cols, res.size, base2k, len(terms)))
    for a, join, k, sign in terms:
        f.write("%d %d %d %d %d\n" % (a.size, join, k, sign < 0, a is res))
        f.write(" ".join(str(int(v)) for v in a.data.reshape(-1)) + "\n")
    f.write(" ".join(str(int(v)) for v in want.data.reshape(-1)) + "\n")


# ---- the plans' scenarios -------------------------------------------------------------------------------------------------------------
def _ct(B, size, log_delta, log_budget, cols=2):
    return Ct(B, size, log_delta, log_budget, cols)


def add_many_scenarios(B):
    """(label, dst, inputs).  add_many.rs's five: aligned, single_input, mixed_budgets, delta_log_delta (the first of five inputs encoded
    12 bits lower, log_delta - 12 in a ciphertext of max_k - 12 bits, so the result takes the lower log_delta), smaller_output.  Then
    more unequal budgets: every join, a term at position >= 2 below everything before it (the only way PZ_JOIN_LSH_ACC arises), and
    a lower log_delta that comes late, with a lower budget."""
    d = 2 * B + 3                                   # log_delta
    full = lambda size, budget=None: _ct(B, size, d, size * B - d if budget is None else budget)   # effective_k = max_k by default
    low = _ct(B, -(-(5 * B - 12) // B), d - 12, 5 * B - d)            # encrypt_with_prec(max_k - 12, log_delta - 12): the budget stays
    out = [
        ("single_aligned", _ct(B, 5, 0, 0), [full(5)]),
        ("single_smaller_output", _ct(B, 3, 0, 0), [full(5)]),
        ("two_aligned", _ct(B, 5, 0, 0), [full(5), full(5)]),
        ("four_aligned", _ct(B, 5, 0, 0), [full(5)] * 4),
        ("four_smaller_output", _ct(B, 3, 0, 0), [full(5)] * 4),
        ("two_first_lower", _ct(B, 5, 0, 0), [full(5, 2 * B), full(5)]),
        ("two_second_lower", _ct(B, 5, 0, 0), [full(5), full(4, B + 5)]),
        ("five_mixed", _ct(B, 5, 0, 0), [full(5, 2 * B + 1), full(5), full(4, 2 * B + 1), full(5, B - 2), full(5, 2 * B + 7)]),
        ("late_drop_whole_limb", _ct(B, 4, 0, 0), [full(5), full(5), full(5, 3 * B - d), full(3)]),
        ("smaller_output_mixed", _ct(B, 3, 0, 0), [full(5), full(4), full(5, B)]),
        ("delta_log_delta", _ct(B, 5, 0, 0), [low] + [full(5)] * 4),
        ("delta_log_delta_late_and_lower", _ct(B, 5, 0, 0), [full(5), full(5), _ct(B, 4, d - 7, 2 * B), full(5), _ct(B, 5, d + 2, 3 * B - d - 2)]),
    ]
    return out


def pt_scenarios(B):
    """(label, dst, a, pt) for mul_pt_vec_znx / mul_add / mul_sub: mul.rs test_mul_pt_vec_znx_{aligned, smaller_output, assign-shaped,
    delta_lower} and the mul_add / mul_sub pairs (aligned, smaller output), as layouts: the plaintext's size is max_k / base2k."""
    d = 2 * B + 3
    a5 = _ct(B, 5, d, 5 * B - d)
    return [
        ("aligned", _ct(B, 5, d, 5 * B - d), a5, Pt(B, 2, B + 3, log_budget=B - 3)),
        ("smaller_output", _ct(B, 3, d, 3 * B - d), a5, Pt(B, 2, B + 3, log_budget=B - 3)),
        ("one_limb_pt", _ct(B, 5, d, 2 * B), a5, Pt(B, 1, B - 2, log_budget=2)),
        ("three_limb_pt", _ct(B, 4, d - 1, B - 1), a5, Pt(B, 3, 2 * B + 1, log_budget=B - 1)),
    ]


def dot_scenarios(B):
    """(label, dst, ops, pts).  dot_product.rs::test_dot_product_pt_vec_znx_aligned (equal layouts), one pair, unequal budgets /
    plaintext deltas that reach every join, with LSH_ACC at position >= 2, and ciphertexts of different log_delta (the products carry
    them: the lowest comes second, a higher one last)."""
    d = 2 * B + 3
    a5 = _ct(B, 5, d, 5 * B - d)
    p2 = Pt(B, 2, B + 3, log_budget=B - 3)
    return [
        ("aligned", _ct(B, 5, 0, 0), [a5] * 3, [p2] * 3),
        ("single", _ct(B, 5, 0, 0), [a5], [p2]),
        ("mixed", _ct(B, 4, 0, 0), [a5, _ct(B, 4, d, 4 * B - d), a5, _ct(B, 4, d, 4 * B - d - 5), a5],
         [p2, Pt(B, 1, B - 2, log_budget=2), Pt(B, 2, B + 7, log_budget=B - 7), p2, Pt(B, 1, 5, log_budget=B - 5)]),
        ("smaller_output", _ct(B, 3, 0, 0), [a5, a5, a5, a5], [p2, Pt(B, 2, B + 5, log_budget=B - 5), p2, Pt(B, 2, B + 1, log_budget=B - 1)]),
        ("delta_log_delta", _ct(B, 5, 0, 0), [a5, _ct(B, 5, d - 9, 5 * B - d + 9), _ct(B, 5, d - 4, 5 * B - d + 4), _ct(B, 5, d + 3, 5 * B - d - 3)],
         [p2, p2, Pt(B, 2, B + 5, log_budget=B - 5), p2]),
    ]


def materialize(rng, n, ct: Ct, normalized=True) -> Ct:
    return Ct(ct.base2k, ct.size, ct.log_delta, ct.log_budget, ct.cols, fill(rng, VecZnx(n, ct.cols, ct.size), ct.base2k, normalized))


def materialize_pt(rng, n, pt: Pt) -> Pt:
    return Pt(pt.base2k, pt.size, pt.log_delta, fill(rng, VecZnx(n, 1, pt.size), pt.base2k, True), log_budget=pt.log_budget)


def clone(ct: Ct) -> Ct:
    return Ct(ct.base2k, ct.size, ct.log_delta, ct.log_budget, ct.cols, ct.data.copy())
