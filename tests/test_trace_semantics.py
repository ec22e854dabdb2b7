"""Encrypt, trace / pack, decrypt: poulpy-core's test_glwe_trace_assign (poulpy-core/src/test_suite/trace.rs) and test_glwe_packing
(test_suite/glwe_packing.rs) restated against the oracle, at the reference's FFT64Ref parameters (N = 256, base2k 17:
poulpy-cpu-ref/src/tests.rs:154-158; the packing at N = 64) and at the device's route shapes that the oracle finishes quickly.

The parity suite runs both operations with one uniform-digit "key" per Galois element, so the order of the elements and which key
serves which step, g against g^-1, the one-bit shift in front of each step and the tree walk from a ciphertext's index to a coefficient
are shared by the device, the oracle and the exact statements.  Here every key is a real automorphism key, `want` follows from the
definition on the plaintext, and the check is the reference's noise formula; each convention has a negative control that must fail it.
Cases: tests/trace_cases.py; the device runs the same ones in tests/test_gpu_trace_semantics.py.  noise_have / noise_want are printed (`-s`)."""
import numpy as np
import pytest

from tests import fhe_sk as fs
from tests import trace_cases as tc
from tests.helpers import seeded

BATCH = 3     # the cases of tests/test_gpu_trace_semantics.py, so that a failure there is the device's


@pytest.fixture(scope="module")
def refs():
    from oracle.ref import RefModule
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = RefModule(n)
        return cache[n]
    return get


def test_toolkit_trace_and_pack_on_plaintexts():
    """The Galois elements are the reference's; the definition, applied to exact integers, keeps 2^steps x_0 over the full trace and the
    coefficients that are multiples of 2^t over its last t steps; the tree walk sends the ciphertext of index j to coefficient j (as
    tests/test_oracle_exact.py::test_P11_glwe_pack_tree_walk walks it) and leaves the coefficients off the output gap empty."""
    n = 64
    assert tc.trace_gals(n) == [-1, 5, 25, 625 % 128, pow(5, 8, 128), pow(5, 16, 128)]
    rng = seeded(3)
    x0 = fs.to_int(fs.uniform_digits((2, n), 12, rng), 12)
    x = x0
    for g in tc.trace_gals(n)[-3:]:
        x = tc._step(x, g)
    keep = np.arange(n) % 8 == 0
    assert np.array_equal(x[keep], x0[keep] * 8) and not np.any(x[~keep])
    for indices, gap in (([0, 5, 17, 32, 33, 63], 0), ([0, 8, 48], 3)):
        pts = {j: fs.rotate(x0, -j) for j in indices}
        packed = tc._pack_plain(pts, n, gap)
        for j in indices:
            assert packed[j] == pts[j][0] * n, (indices, j)
        off = np.arange(n) % (1 << gap) != 0
        assert not np.any(packed[off])


@pytest.mark.parametrize("kind", ["trace", "pack"])
def test_reference_procedures_on_oracle(refs, kind):
    for label, c in tc.reference_cases(kind, batch=BATCH):
        tc.check(label, c, tc.run_oracle(refs(c.n), c))


def test_negative_controls_fail_on_oracle(refs):
    for label, c in tc.control_cases(batch=BATCH):
        tc.check(label, c, tc.run_oracle(refs(c.n), c), fail=True)


@pytest.mark.parametrize("name", [k for k, v in tc.ROUTES.items() if v[2].host])
def test_route_shapes_on_oracle(refs, name):
    c, _ = tc.route_case(name, batch=BATCH)
    tc.check(name, c, tc.run_oracle(refs(c.n), c))
