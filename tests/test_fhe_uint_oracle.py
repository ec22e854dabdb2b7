"""FheUintPrepared::prepare on the oracle (tests/fhe_uint_oracle.py), under real keys, on the reference's own shape
(bdd_arithmetic/tests/test_suite/mod.rs:138-209, the LWE dimension cut to 14): every (row, column) of every prepared bit stays within the
reference's own bound (test_suite/prepare.rs:77-84), and the external product of a fresh GLWE with bit i's GGSW decrypts to bit_i * pt.
Each negative control stands next to its positive twin and must miss.  About forty oracle circuit bootstrappings in all."""
import math

import numpy as np
import pytest

from poulpy_amd.layouts import VecZnx
from tests import fhe_sk as fs
from tests import fhe_uint_cases as fc
from tests import fhe_uint_oracle as fo
from tests import lwe_cases as lc
from tests.helpers import seeded


@pytest.fixture(scope="module")
def ref_case():
    from oracle.ref import RefModule
    c = fc.bdd_key_case(fc.REF_SHAPE, 45000)
    ref = RefModule(c.n)
    return ref, c, fo.PreparedKey(ref, c)


def noise_max(c, col):
    """prepare.rs:77-84"""
    log_n = c.n.bit_length() - 1
    bound = -(c.res_size * c.res_b) + math.log2(fs.SIGMA) + 2.0 + 0.5 * log_n
    return bound + (0.5 * log_n if col != 0 else 0.0)


def worst_noise(c, ggsw, bit):
    """max over (row, column) of noise_have - noise_max for the GGSW of the constant `bit`"""
    msg = np.zeros(c.n, dtype=np.int64)
    msg[0] = bit
    worst = -math.inf
    for row in range(c.res_dnum):
        pt0 = fs._row_plaintext(msg, c.res_size, row, c.res_b)
        for col in range(c.rank + 1):
            pt = pt0 if col == 0 else fs.normalize(fs.mul_small(pt0, c.sk_glwe[col - 1]), c.res_b)
            worst = max(worst, fs.noise_log2(ggsw[row, col], c.res_b, c.sk_glwe, pt, c.res_b) - noise_max(c, col))
    return worst


def selected(ref, c, ggsw, rng):
    """The external product of a fresh GLWE with the GGSW, decrypted: 0 when it is the zero plaintext, 1 when it is the GLWE's own, else None.
    The plaintext has a value of {-1, 0, 1} on every coefficient, encoded at k = 2 as the words' bits are and decoded at k = 2 as
    FheUint::decrypt does (fhe_uint.rs:199-210).  A GGSW at the reference's noise bound, 2^-31.3 on column 0, leaves an error of about
    2^-31.3 2^12 sqrt(n (rank + 1) dnum) = 2^-14 behind the product: far below the 2^-3 that decoding at k = 2 tolerates, and far above
    what an exact comparison of limb 0 (13 bits) would."""
    cols = c.rank + 1
    data = rng.integers(-1, 2, c.n)
    data[0] = 1
    a = VecZnx(c.n, cols, c.res_size, np.ascontiguousarray(fs.glwe_encrypt(c.sk_glwe, fs.encode(data, c.res_b, 2, c.res_size), c.res_b, c.k_ggsw, rng)))
    res = VecZnx(c.n, cols, c.res_size)
    ref.glwe_external_product(res, c.res_b, a, c.res_b, lc.prepare(ref, ggsw), 1, c.res_b)
    pt = fs.normalize(fs.glwe_phase(res.data, c.sk_glwe), c.res_b)
    got = np.array([fs.decode_coeff(pt, c.res_b, 2, j) for j in range(c.n)])
    got = ((got + 2) % 4) - 2          # two bits, signed
    return 0 if not got.any() else 1 if np.array_equal(got, data) else None


def check_word(ref, c, key, value, word_bits, bit_start, bit_count, with_ks_glwe, seed, index=fc.coefficient, fail=False):
    """Prepares the word and reads every bit of the range back; a control must miss: a bit beyond its bound, or a wrong selection."""
    rng = seeded(seed)
    word = fc.encrypt_word(c, value, word_bits, rng)
    assert fc.decrypt_word(c, word, word_bits) == value
    r = fo.prepare_word(ref, c, key, word, word_bits, bit_start, bit_count, with_ks_glwe, index)
    bits = [(value >> i) & 1 for i in range(word_bits)]
    worst, read = -math.inf, []
    for i in range(bit_start, bit_start + bit_count):
        worst = max(worst, worst_noise(c, r.ggsw[i], bits[i]))
        read.append(selected(ref, c, r.ggsw[i], rng))
    want = bits[bit_start:bit_start + bit_count]
    print(f"[noise] {word_bits}-bit word {value:#x} bits [{bit_start}, {bit_start + bit_count}), ks_glwe {with_ks_glwe}: worst noise_have - noise_max "
          f"{worst:.2f}, bits read {read}, want {want}")
    for i in list(range(bit_start)) + list(range(bit_start + bit_count, word_bits)):
        assert not r.ggsw[i].any() and not r.pmat[i].any(), "a bit outside the range is not zero"
    if fail:
        assert worst > 0 or read != want, "a negative control prepared the word"
    else:
        assert worst <= 0, worst
        assert read == want


@pytest.mark.parametrize("with_ks_glwe", [True, False], ids=["ks_glwe", "direct"])
def test_u8_word(ref_case, with_ks_glwe):
    ref, c, key = ref_case
    check_word(ref, c, key, 0xA5, 8, 0, 8, with_ks_glwe, 45100)


def test_u32_sub_range_and_its_uninterleaved_control(ref_case):
    """bits [5, 12) of a u32 word; read at i << log_gap instead of bit_index(i) << log_gap the same call selects other bits of the word."""
    ref, c, key = ref_case
    value = 0x9E3779B9
    check_word(ref, c, key, value, 32, 5, 7, True, 45200)
    check_word(ref, c, key, value, 32, 5, 7, True, 45200, index=lambda i, w, n: i * (n // w), fail=True)


def test_ks_lwe_for_another_lwe_secret_must_miss(ref_case):
    ref, c, key = ref_case
    other = fc.bdd_key_case(fc.REF_SHAPE, 45000, wrong_lwe_secret=True)
    assert np.array_equal(other.sk_glwe, c.sk_glwe) and np.array_equal(other.sk_lwe, c.sk_lwe)
    check_word(ref, other, fo.PreparedKey(ref, other), 0xA5, 8, 0, 8, True, 45100, fail=True)
