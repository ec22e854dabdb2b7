"""Encrypt, multiply, decrypt: poulpy-core's tensoring tests (poulpy-core/src/test_suite/glwe_tensor.rs: test_glwe_tensoring,
_apply_add_assign, _square) restated against the oracle, at the reference's FFT64Ref parameters (N = 256, base2k 17:
poulpy-cpu-ref/src/tests.rs:154-158) with every res_offset and rank 1..3, and at the device's route shapes that the oracle finishes quickly.

The parity suite (tests/test_gpu_cnv.py, tests/test_oracle_cnv.py) compares the device with the oracle on uniform digits and the oracle
with exact column products; the pair order of the tensor columns, which tensor-key column meets which pair, the meaning of cnv_offset and
of a masked bottom limb, and the square form's doubled cross terms are shared by all of them.  Here the tensor key is a real encryption
of s_i s_j, the inputs encrypt messages, and the results must decrypt to the exact product of the messages within the reference's
bound; each convention has a negative control that must fail it.  Cases: tests/tensor_cases.py; the device runs the same ones in
tests/test_gpu_tensor_semantics.py.  noise_have / noise_want are printed (`-s`)."""
import math

import numpy as np
import pytest

from tests import fhe_sk as fs
from tests import tensor_cases as tc
from tests.helpers import seeded

BATCH = 3     # the cases of tests/test_gpu_tensor_semantics.py, so that a failure there is the device's


@pytest.fixture(scope="module")
def refs():
    from oracle.ref import RefModule
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = RefModule(n)
        return cache[n]
    return get


# ---- the toolkit itself ----
def test_toolkit_tensor_products_and_phase():
    """secret_tensor against a schoolbook product at N = 64; mul_msg's FFT path against its schoolbook path at N = 8192; encode and
    torus_from_int agree; a fresh GLWE read as a tensor with zero pair columns has the fresh phase."""
    rng = seeded(2)
    n, rank = 64, 3
    sk = fs.ternary_secret(n, rank, rng)
    st = fs.secret_tensor(sk)
    assert st.shape == (6, n)
    for i in range(rank):
        for j in range(i, rank):
            want = np.zeros(n, dtype=np.int64)
            for x in range(n):
                for y in range(n):
                    s = int(sk[i, x]) * int(sk[j, y])
                    if x + y < n:
                        want[x + y] += s
                    else:
                        want[x + y - n] -= s
            assert np.array_equal(st[i * rank + j - i * (i + 1) // 2], want), (i, j)
    assert [fs.pair_index(i, j, 2) for (i, j) in ((0, 0), (0, 1), (1, 1))] == [0, 1, 2]     # (s0^2, s0 s1, s1^2): glwe_secret_tensor.rs:201
    n = 8192
    a, b = rng.integers(-4, 4, n), rng.integers(-4, 4, n)
    old = fs.SCHOOLBOOK_MAX_N
    try:
        fs.SCHOOLBOOK_MAX_N = n
        slow = fs.mul_msg(a, b)
    finally:
        fs.SCHOOLBOOK_MAX_N = old
    assert np.array_equal(fs.mul_msg(a, b), slow) and np.array_equal(fs.mul_msg(b, a), slow)
    assert np.array_equal(fs.mul_msg(fs.rotate(a, 1), b), fs.rotate(slow, 1))
    # the same torus element two ways, and a value of more than one limb
    m = rng.integers(-4, 4, 256)
    assert np.abs(fs.torus_diff(fs.encode(m, 16, 32, 9), 16, fs.torus_from_int(m, 32, 12), 12)).max() == 0.0
    assert np.abs(fs.torus_diff(fs.encode(m, 15, 32, 3), 15, fs.torus_from_int(m << 5, 37), 16)).max() == 0.0
    assert fs.torus_diff(fs.torus_from_int(np.array([3]), 2), 16, fs.torus_from_int(np.array([-1]), 2), 16)[0] == 0.0   # mod 1
    for (n, rank, base2k, k) in ((256, 2, 15, 137), (8192, 1, 12, 60)):
        sk = fs.ternary_secret(n, rank, rng)
        size = fs.limbs_for(k, base2k)
        pt = fs.uniform_digits((size, n), base2k, rng)
        t = np.zeros((size, (rank + 1) * (rank + 2) // 2, n), dtype=np.int64)
        t[:, :rank + 1] = fs.glwe_encrypt(sk, pt, base2k, k, rng)
        e = fs.torus_diff(fs.glwe_tensor_phase(t, sk, base2k), base2k, pt, base2k)
        assert abs(math.log2(float(np.std(e))) - math.log2(fs.SIGMA * 2.0 ** -k)) < 0.1
    assert fs.var_noise_gglwe_product(256.0, 17, 0.5, 0.5, 0.0, 10.24, 0.0, 1.0, 54, 71) == \
        pytest.approx(4 * 256 * (2.0 ** 34 / 12.0) * 10.24 / 4.0 ** 71)


# ---- the reference tests against the oracle ----
@pytest.mark.parametrize("rank", [1, 2, 3])
@pytest.mark.parametrize("kind", tc.MODES)
def test_reference_procedures_on_oracle(refs, kind, rank):
    """Every res_offset in 0..scale, as glwe_tensor.rs:159 and :386 loop, on the three message pairs the device suite takes."""
    for label, c in tc.reference_cases(kind, batch=BATCH, ranks=(rank,)):
        tc.check(label, c, tc.run_oracle(refs(tc.N), c))


def test_negative_controls_fail_on_oracle(refs):
    for label, c in tc.control_cases(batch=BATCH):
        tc.check(label, c, tc.run_oracle(refs(tc.N), c), fail=True)


# ---- the device's route shapes: a failure of tests/test_gpu_tensor_semantics.py there is then the device's ----
@pytest.mark.parametrize("name", [k for k, v in tc.ROUTES.items() if v[1].host])
def test_route_shapes_on_oracle(refs, name):
    c, _ = tc.route_case(name, batch=BATCH)
    assert c.margin > 1.0, (name, c.margin)
    tc.check(name, c, tc.run_oracle(refs(c.n), c))


def test_large_controls_fail_on_oracle(refs):
    for label, kw in tc.LARGE_CONTROLS.items():
        c = tc.tensor_case(batch=BATCH, **kw)
        tc.check(label, c, tc.run_oracle(refs(c.n), c), fail=True)


# ---- plaintext and constant products (glwe_tensor.rs:433-682) ----
@pytest.mark.parametrize("kind", ["plain", "const"])
def test_plain_reference_procedures_on_oracle(refs, kind):
    """test_glwe_mul_plain / test_glwe_mul_const: rank 1..3, every res_offset in 0..scale, full-width uniform plaintexts; the oracle side is
    tests/plain_oracle.py's composition, `want` the exact product of the plaintext integers."""
    for label, c in tc.plain_reference_cases(kind, batch=BATCH):
        tc.check_plain(label, c, tc.run_plain_oracle(refs(tc.N), c))


def test_plain_negative_controls_fail_on_oracle(refs):
    for label, c in tc.plain_control_cases(batch=BATCH):
        tc.check_plain(label, c, tc.run_plain_oracle(refs(tc.N), c), fail=True)


@pytest.mark.parametrize("name", [k for k, v in tc.PLAIN_ROUTES.items() if v[2]])
def test_plain_route_shapes_on_oracle(refs, name):
    c = tc.plain_route_case(name, batch=BATCH)
    tc.check_plain(name, c, tc.run_plain_oracle(refs(c.n), c))
