"""Inputs shared by tests/test_ckks_dot_host.py and tests/test_gpu_ckks_dot.py: the five ct x ct scenarios of poulpy-ckks
leveled/tests/test_suite/dot_product.rs restated as layouts and metadata (three pairs each, dot_product.rs:31), and one more for the path the
reference's suite does not reach - an aligned side whose containers hold more limbs than its effective_k uses, read in place by stride.

A fresh ciphertext of the reference's test context is encrypted at k with log_delta d: effective_k = max_k = k (tests/ckks_mul_cases.fresh)."""
from __future__ import annotations

from poulpy_amd.ckks import Ct
from tests.ckks_mul_cases import D, fresh

NPAIRS = 3                 # dot_product.rs:31
DELTA_LOG_DELTA = 8        # dot_product.rs:32


def dot_scenarios(B, cols=2, limbs=5):
    """(label, branch, dst size, a_list, b_list)"""
    K = limbs * B
    full = lambda: [fresh(B, K, cols) for _ in range(NPAIRS)]                         # noqa: E731
    one_short = lambda: [fresh(B, K - B + 1 if i == 1 else K, cols) for i in range(NPAIRS)]   # noqa: E731  (dot_product.rs:139, :181)
    # encrypt_with_prec(max_k - 8, .., precision_at(log_delta - 8)): log_budget stays max_k - log_delta (dot_product.rs:242-248)
    low = Ct(B, -(-(K - DELTA_LOG_DELTA) // B), D - DELTA_LOG_DELTA, K - D, cols)
    rescaled = lambda: [Ct(B, limbs, D, K - D - B - 3, cols) for _ in range(NPAIRS)]   # noqa: E731  rescale_assign by base2k + 3 bits
    return [("aligned", "fast", limbs, full(), full()),
            ("one a-side input rescaled", "fast", limbs, one_short(), full()),
            ("one b-side input rescaled", "fast", limbs, full(), one_short()),
            ("non-uniform log_delta", "fallback", limbs, full(), [low] + full()[1:]),
            ("output narrower than the inputs", "fast", -(-(K - B - 1) // B), full(), full()),
            ("aligned a side in larger containers", "fast", limbs, rescaled(), full())]
