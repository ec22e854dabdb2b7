"""Encrypt, operate, decrypt: poulpy-core's core_backend_test_suite! procedures (poulpy-core/src/test_suite/mod.rs:26-88) restated
against the oracle, at the reference's FFT64Ref parameters (N = 256, base2k 17: poulpy-cpu-ref/src/tests.rs:154-158).

The parity suite compares the device with the oracle and the oracle with exact statements on uniform key digits, so a convention that
every side shares cannot fail there.  Here the keys are real encryptions under a secret key (tests/fhe_sk.py) and the check is the
reference's: the noise of phase - plaintext against its closed-form bound.  Each convention also has a negative control run through the
same procedure, and the test asserts that the control fails its bound.  The cases live in tests/core_cases.py;
tests/test_gpu_core_semantics.py runs the same cases through the batched entry points."""
import math

import numpy as np
import pytest

from tests import core_cases as cc
from tests import fhe_sk as fs
from tests.helpers import seeded


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(cc.N)


# ---- the toolkit itself ----
def test_toolkit_products_and_fresh_noise():
    """The FFT product equals the schoolbook one at N = 8192; a fresh encryption's noise is sigma at 2^-k; phi_p^-1 undoes phi_p."""
    rng = seeded(1)
    n = 8192
    a = fs.uniform_digits((2, n), 17, rng)
    s = fs.ternary_secret(n, 1, rng)[0]
    old = fs.SCHOOLBOOK_MAX_N, fs.FFT_MIN_N
    try:
        fs.SCHOOLBOOK_MAX_N, fs.FFT_MIN_N = n, 2 * n
        slow = fs.mul_small(a, s)
    finally:
        fs.SCHOOLBOOK_MAX_N, fs.FFT_MIN_N = old
    assert np.array_equal(fs.mul_small(a, s), slow)
    assert np.array_equal(fs.mul_small(fs.rotate(a, 3), s), fs.rotate(slow, 3))
    for (n, rank, base2k, k) in ((256, 2, 17, 65), (65536, 1, 12, 96)):
        sk = fs.ternary_secret(n, rank, rng)
        pt = fs.uniform_digits((fs.limbs_for(k, base2k), n), base2k, rng)
        ct = fs.glwe_encrypt(sk, pt, base2k, k, rng)
        have = fs.noise_log2(ct, base2k, sk, pt, base2k)
        assert abs(have - math.log2(fs.SIGMA * 2.0 ** -k)) < 0.1, (n, have)
        assert fs.noise_log2(ct, base2k, sk, fs.rotate(pt, 1), base2k) > -4   # a wrong plaintext is noise of order 1
    x = fs.uniform_digits((1, 256), 12, rng)
    assert np.array_equal(fs.automorphism(fs.automorphism(x, cc.P_AUTO), fs.galois_inv(cc.P_AUTO, 256)), x)


# ---- the reference tests against the oracle ----
@pytest.mark.parametrize("kind", ["ep", "ep_assign", "ks", "ks_assign", "auto", "auto_assign"])
def test_reference_procedures_on_oracle(ref, kind):
    for label, c, _ in cc.reference_cases(kind, batch=2):
        cc.check(label, c, cc.run_oracle(ref, c))


def test_negative_controls_fail_on_oracle(ref):
    for label, c, _ in cc.control_cases(batch=2):
        cc.check(label, c, cc.run_oracle(ref, c), fail=True)
