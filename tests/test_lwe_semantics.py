"""Encrypt, convert / rotate, decrypt on the LWE side: poulpy-core's LWE key-switch and conversion tests (test_suite/keyswitch/lwe_ct.rs,
test_suite/conversion.rs) and poulpy-bin-fhe's blind-rotation test (blind_rotation/tests/test_suite/generic_blind_rotation.rs, the shapes of
tests/fft64_ref.rs:24-40) restated against the oracle with real keys (tests/fhe_sk.py), and the gate bootstrap chain on top.

Parity on uniform digits cannot see a sign or an index that kernels, oracle and exact statements share; here the body sits at index 0 of an
LWE, a secret enters a key as phi_{-1}(s || 0), the table has its half-step drift, key row i meets LWE coefficient i, and every one of these
has a negative control that must fail to decrypt.  The cases live in tests/lwe_cases.py; tests/test_gpu_lwe_semantics.py runs them through
the batched entry points.  noise_have / noise_want are printed (`-s`)."""
import numpy as np
import pytest

from tests import fhe_sk as fs
from tests import lwe_cases as lc
from tests.helpers import seeded


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
def test_lwe_toolkit():
    """A fresh LWE's error is sigma at 2^-k and decodes to its message; encode / decode round-trip where the message spans limbs; a block
    holds at most one 1; the embedded secret's product has <a, s> as its constant coefficient."""
    rng = seeded(5)
    for base2k, k, bits in ((17, 69, 8), (19, 24, 5), (12, 30, 14)):
        sk = fs.ternary_lwe_secret(100, rng)
        errs = []
        for m in range(-16, 16):
            pt = fs.encode_int(m, base2k, bits)
            ct = fs.lwe_encrypt(sk, pt, base2k, k, rng)
            assert fs.decode_coeff(fs.lwe_decrypt(ct, sk, base2k), base2k, bits) == m
            assert fs.decode_coeff(pt, base2k, bits) == m
            errs.append(fs.lwe_error(ct, base2k, sk, pt, base2k))
        assert abs(fs.rms_log2(errs) - np.log2(fs.SIGMA * 2.0 ** -k)) < 0.6, (base2k, k, fs.rms_log2(errs))
    s = fs.binary_block_secret(7 * 32, 7, rng)
    assert set(np.unique(s)) <= {0, 1} and s.reshape(-1, 7).sum(axis=1).max() <= 1 and 0 < s.sum() < 32
    sk = fs.ternary_lwe_secret(22, rng)
    a = np.zeros((1, 64), dtype=np.int64)
    a[0, :22] = rng.integers(-50, 50, 22)
    assert fs.mul_small(a, fs.lwe_as_glwe_secret(sk, 64)[0])[0, 0] == a[0, :22] @ sk
    assert fs.mul_small(a, fs.lwe_as_glwe_secret(sk, 64, embed=False)[0])[0, 0] == a[0, 0] * sk[0]


def test_lut_properties():
    """The reference's test_lut_standard / test_lut_extended (tests/test_suite/generic_lut.rs): turning the table by -i step brings f(i) to
    coefficient 0 of polynomial 0, and - the drift - so does every turn within half a step of it; ext = 1 and 2 agree through the ring
    switch; lut_rotate composes."""
    # the reference's own two tests (generic_lut.rs:7-85, N = 32): base2k 20, a scale of 21 bits (two limbs), f(i) = i - 8, extension factor 1 / 4;
    # with the drift turned back every coefficient of every polynomial decodes to f of its step
    f = [i - 8 for i in range(16)]
    for ext in (1, 4):
        lut, drift = fs.lut_set(f, 21, 32, ext, 20, 40)
        assert drift == (32 * ext + 16) // 32
        back = fs.lut_rotate(lut, drift)
        for j in range(ext):
            assert [fs.decode_coeff(back[j], 20, 21, i) for i in range(32)] == [f[i // 2] for i in range(32)], (ext, j)
    base2k, k_lut, log_mod = 10, 20, 4
    f = [(-1) ** i * i for i in range(1 << log_mod)]
    for n, ext in ((32, 1), (32, 2), (64, 4)):
        lut, drift = fs.lut_set(f, log_mod + 1, n, ext, base2k, k_lut)
        step = n * ext // len(f)
        assert drift == step // 2 and lut.shape == (ext, 2, n)
        for i in range(len(f)):
            for j in range(-drift, step - drift):
                r = fs.lut_rotate(lut, -(i * step + j))
                assert fs.decode_coeff(r[0], base2k, log_mod + 1, 0) == f[i], (n, ext, i, j)
        assert np.array_equal(fs.lut_rotate(fs.lut_rotate(lut, 5), -5), lut)
        assert np.array_equal(fs.lut_rotate(fs.lut_rotate(lut, 3), 2 * n * ext - 7), fs.lut_rotate(lut, -4))
        no_drift, _ = fs.lut_set(f, log_mod + 1, n, ext, base2k, k_lut, with_drift=False)
        assert fs.decode_coeff(fs.lut_rotate(no_drift, -(3 * step - 1))[0], base2k, log_mod + 1, 0) == f[2]


@pytest.mark.parametrize("negate", [False, True])
def test_mod_switch_2n_branches(refs, negate):
    """The exact restatement equals the oracle on both branches of algorithms/mod.rs:136-171.  What the branches compute: with one limb
    wider than log2n the exponents are round(+-lwe 2N), and b + <a, s> follows the phase; where limbs are concatenated (base2k <= log2n)
    the reference keeps log2n bits, one more than 2N has, and negates limb 0 only - the exponent is then twice the phase (mod 2N) at best.
    Oracle and device restate both; the cases of tests/lwe_cases.py keep to the first."""
    ref = refs(256)
    rng = seeded(9 + negate)
    n_lwe = 40
    sk = fs.ternary_lwe_secret(n_lwe, rng)
    for n2, base2k, size, rounds in ((2048, 17, 2, True), (2048, 19, 2, True), (2048, 12, 2, False), (8192, 13, 3, False), (64, 7, 1, False)):
        off = []
        for m in range(4):
            lwe = fs.lwe_encrypt(sk, fs.encode_int(3 + 4 * m, base2k, 5), base2k, size * base2k, rng)
            have = ref.mod_switch_2n(n2, lwe, base2k, negate)
            assert np.array_equal(have, fs.mod_switch_2n(n2, lwe, base2k, negate)), (n2, base2k, size)
            phase = (int(have[0]) + int(have[1:] @ sk)) * (-1 if negate else 1)
            want = (3 + 4 * m) * n2 // 32
            off.append(min((phase - want) % n2, (want - phase) % n2))
        if rounds:
            assert max(off) <= 8, (n2, base2k, off)       # rounding of n_lwe / 2 exponents: a few units
        else:
            assert min(off) > n2 // 32, (n2, base2k, off)


# ---- conversions ----
def test_conversions_on_oracle(refs):
    for label, c in lc.reference_conversions():
        lc.check_conversion(label, c, lc.run_conversion_oracle(refs(c.n), c))


def test_conversion_controls_fail_on_oracle(refs):
    for label, c in lc.conversion_controls():
        lc.check_conversion(label, c, lc.run_conversion_oracle(refs(c.n), c), fail=True)


# ---- blind rotation ----
@pytest.mark.parametrize("block_size,ext", [(1, 1), (7, 1), (7, 2)], ids=["standard", "block_binary", "block_binary_extended"])
def test_blind_rotation_on_oracle(refs, block_size, ext):
    """fft64_ref.rs:24-40: N = 512, n_lwe = 224, block 1 / 7, extension factor 2; 16 table values and a noise-free first limb."""
    c = lc.blind_rotation_case(block_size=block_size, ext=ext, seed=100 + block_size + ext, **lc.REF_ROTATION)
    assert c.log_mod == 4 and c.limb0
    lc.check_rotation(("reference shape", block_size, ext), c, *lc.run_rotation_oracle(refs(c.n), c))


@pytest.mark.parametrize("label,kw,fail", lc.ROTATION_CONTROLS, ids=[c[0] for c in lc.ROTATION_CONTROLS])
def test_rotation_controls_on_oracle(refs, label, kw, fail):
    """Each control next to its positive twin: the same calls, one convention flipped."""
    c = lc.blind_rotation_case(**{**lc.SMALL, **kw}, seed=300)
    lc.check_rotation(label, c, *lc.run_rotation_oracle(refs(c.n), c), fail=fail)
    if fail and "tail_bit" not in kw and "plant" not in kw:
        twin = lc.blind_rotation_case(**lc.SMALL, seed=300)
        lc.check_rotation(label + ": twin", twin, *lc.run_rotation_oracle(refs(c.n), twin))


@pytest.mark.parametrize("n,block_size", [(256, 7), (1024, 7), (1024, 1)])
def test_gate_bootstrap_on_oracle(refs, n, block_size):
    """LWE -> mod_switch_2n -> rotation -> lwe_from_glwe at coefficient 0 under a real GLWE -> LWE key -> LWE decryption = f(x)."""
    c = lc.blind_rotation_case(n, 1, 28, block_size, 2, 3, 2, 17, seed=400 + n + block_size, gate=True)
    ref = refs(n)
    lwe_2n, acc = lc.run_rotation_oracle(ref, c)
    lc.check_rotation(("gate: rotation", n, block_size), c, lwe_2n, acc)
    lc.check_gate(("gate: LWE", n, block_size), c, lc.run_gate_oracle(ref, c, acc))


# ---- circuit bootstrapping ----
def _cbt_on_oracle(ref, label, c, fail=False):
    return lc.check_cbt_on(lambda c: lc.run_cbt_oracle(ref, c), lambda c, g, cts: lc.run_cbt_end_oracle(ref, c, g, cts), label, c, fail=fail)


@pytest.mark.parametrize("bases", [lc.REF_CBT_BASES, lc.ONE_BASE], ids=["reference bases", "one base"])
@pytest.mark.parametrize("mode", ["constant", "exponent"])
def test_circuit_bootstrap_on_oracle(refs, mode, bases):
    """tests/circuit_bootstrapping.rs at its own shape (N = 256, n_lwe = 77, block 7, rank 1) and bases, and a one-base twin."""
    c = lc.cbt_case(256, 1, 77, 7, bases, mode, seed=600)
    _cbt_on_oracle(refs(c.n), ("circuit bootstrap", mode, bases), c)


@pytest.mark.parametrize("label,kw,fail", lc.CBT_CONTROLS, ids=[c[0] for c in lc.CBT_CONTROLS])
def test_circuit_bootstrap_controls_on_oracle(refs, label, kw, fail):
    c = lc.cbt_case(**kw, seed=700)
    _cbt_on_oracle(refs(c.n), label, c, fail=fail)
