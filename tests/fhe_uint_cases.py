"""Cases for FheUintPrepared::prepare (poulpy-bin-fhe/src/bdd_arithmetic/ciphertexts/fhe_uint_prepared.rs:399-460): the secrets, the BDD key
(blind-rotation key, automorphism keys, tensor key, ks_glwe, ks_lwe; bdd_arithmetic/key.rs:199-245) and FheUint words encrypted as
FheUint::encrypt_sk does (fhe_uint.rs:84-130): bit i at coefficient bit_index(i) << log_gap, encoded at k = 2.

REF_SHAPE is the reference's own (bdd_arithmetic/tests/test_suite/mod.rs:138-209) with the LWE dimension cut from 77 to 14, as
lwe_cases.CBT_CONTROLS does; ONE_BASE_SHAPE has one base2k for every object and rank 1.

The base2k = 4 of that test suite (TEST_LWE_BASE2K) is the base of the two key-switching keys and of get_bit_lwe's intermediate GLWE
(fhe_uint.rs:386-391).  The LWE handed to the circuit bootstrapping is `scratch.take_lwe(bits)` (fhe_uint_prepared.rs:443): it has the
WORD's base and precision (13, k 26), so mod_switch_2n rounds one limb.  REF_SHAPE_LWE4 puts the LWE itself in base 4 (k 16), where
mod_switch_2n concatenates limbs and negates the first one only (mod.rs:136-171): that shape is run for bit-exactness, and its result
does not decrypt - on the oracle either."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests import fhe_sk as fs
from tests import key_ops_cases as kc
from tests import trace_cases as tc
from tests.helpers import seeded

# (k, dnum) of the two key-switching keys; key_k / key_dnum: the blind-rotation, automorphism and tensor keys
REF_SHAPE = dict(n=256, rank=2, word_b=13, k_word=26, res_b=13, k_ggsw=39, res_dnum=2, brk_b=12, atk_b=11, tsk_b=10, key_k=52, key_dnum=4,
                 ks_b=4, lwe_b=13, k_lwe=26, ks_glwe=(20, 3), ks_lwe=(16, 3), block_size=7, n_lwe=14)
REF_SHAPE_LWE4 = dict(REF_SHAPE, lwe_b=4, k_lwe=16)
ONE_BASE_SHAPE = dict(n=256, rank=1, word_b=13, k_word=26, res_b=13, k_ggsw=39, res_dnum=2, brk_b=13, atk_b=13, tsk_b=13, key_k=52, key_dnum=4,
                      ks_b=13, lwe_b=13, k_lwe=26, ks_glwe=(39, 2), ks_lwe=(39, 2), block_size=7, n_lwe=14)


def _cdiv(a, b):
    return -(-a // b)


def bit_index(i: int, word_bits: int) -> int:
    """bdd_arithmetic/mod.rs:97-99: the bytes of a word are interleaved, bit i of byte j lies at (i << LOG_BYTES) | j."""
    log_bytes = (word_bits // 8).bit_length() - 1
    return ((i & 7) << log_bytes) | (i >> 3)


def coefficient(i: int, word_bits: int, n: int) -> int:
    """fhe_uint.rs:384: bit_index(i) << log_gap."""
    return bit_index(i, word_bits) * (n // word_bits)


def encrypt_word(c, value: int, word_bits: int, rng, index=coefficient) -> np.ndarray:
    """FheUint::encrypt_sk: (size, rank + 1, n) at the word's base.  index (a negative control): where bit i goes."""
    data = np.zeros(c.n, dtype=np.int64)
    for i in range(word_bits):
        data[index(i, word_bits, c.n)] = (value >> i) & 1
    size = fs.limbs_for(c.k_word, c.word_b)
    return np.ascontiguousarray(fs.glwe_encrypt(c.sk_glwe, fs.encode(data, c.word_b, 2, size), c.word_b, c.k_word, rng))


def decrypt_word(c, ct: np.ndarray, word_bits: int, index=coefficient) -> int:
    """FheUint::decrypt (fhe_uint.rs:186-222): decode at k = 2, read bit i at its coefficient."""
    pt = fs.normalize(fs.glwe_phase(ct, c.sk_glwe), c.word_b)
    value = 0
    for i in range(word_bits):
        value |= (fs.decode_coeff(pt, c.word_b, 2, index(i, word_bits, c.n)) & 1) << i
    return value


def bdd_key_case(shape, seed, wrong_lwe_secret=False):
    """The secrets and the BDD key of one shape.  ks_lwe["direct"] switches from the word's secret (no ks_glwe), ks_lwe["mid"] from the
    intermediate rank-1 secret ks_glwe switches to (key.rs:214-230).  wrong_lwe_secret (a negative control): both ks_lwe are made for another
    LWE secret than the blind-rotation key's."""
    s = SimpleNamespace(**shape)
    rng = seeded(seed)
    n, rank = s.n, s.rank
    sk_glwe = fs.ternary_secret(n, rank, rng)
    sk_lwe = fs.binary_block_secret(s.n_lwe, s.block_size, rng)
    sk_mid = fs.ternary_secret(n, 1, rng)
    brk = fs.blind_rotation_key(sk_glwe, sk_lwe, s.brk_b, s.key_k, s.key_dnum, rng)
    gals = tc.trace_gals(n)
    atk = [fs.automorphism_key(sk_glwe, g, s.atk_b, s.key_k, s.key_dnum, 1, rng) for g in gals]
    tsk = kc.tensor_key(sk_glwe, s.tsk_b, s.key_k, s.key_dnum, 1, rng)
    sk_ks = fs.binary_block_secret(s.n_lwe, s.block_size, rng) if wrong_lwe_secret else sk_lwe
    if wrong_lwe_secret:
        assert not np.array_equal(sk_ks, sk_lwe)
    ks_glwe = fs.switching_key(sk_glwe, sk_mid, s.ks_b, s.ks_glwe[0], s.ks_glwe[1], 1, rng)
    ks_lwe = {"direct": fs.glwe_to_lwe_key(sk_ks, sk_glwe, s.ks_b, s.ks_lwe[0], s.ks_lwe[1], rng),
              "mid": fs.glwe_to_lwe_key(sk_ks, sk_mid, s.ks_b, s.ks_lwe[0], s.ks_lwe[1], rng)}
    # circuit.rs:258-301 in constant mode with log_domain = 1 (fhe_uint_prepared.rs:446)
    res_size = fs.limbs_for(s.k_ggsw, s.res_b)
    alpha = 1 << (s.res_dnum - 1).bit_length()
    f = [0] * (2 * alpha)
    for i in range(s.res_dnum):
        f[alpha + i] = 1 << (s.res_b * (s.res_dnum - 1 - i))
    lut, drift = fs.lut_set(f, s.res_b * s.res_dnum, n, 1, s.brk_b, s.res_b * s.res_dnum)
    sh = dict(glwe_size=_cdiv(s.key_k, s.brk_b), atk_glwe_size=_cdiv(s.key_k, s.atk_b), trace_size=_cdiv(max(s.key_k, s.k_ggsw), s.atk_b))
    word_size = fs.limbs_for(s.k_word, s.word_b)
    # get_bit_lwe's intermediate (fhe_uint.rs:386-391): the LWE key's base, k = min(ks_lwe.max_k, word.max_k)
    mid_size = fs.limbs_for(min(s.ks_lwe[0], s.k_word), s.ks_b)
    lwe_size = fs.limbs_for(s.k_lwe, s.lwe_b)
    return SimpleNamespace(**shape, bases=(s.brk_b, s.atk_b, s.tsk_b, s.res_b), sk_glwe=sk_glwe, sk_lwe=sk_lwe, sk_mid=sk_mid, brk=brk, gals=gals,
                           atk=atk, tsk=tsk, ks_glwe_key=ks_glwe, ks_lwe_key=ks_lwe, lut=lut, gap=2 * drift, sh=sh, res_size=res_size,
                           word_size=word_size, mid_size=mid_size, lwe_size=lwe_size, brk_dnum=s.key_dnum, atk_dnum=s.key_dnum,
                           tsk_dnum=s.key_dnum, n2=2 * n)


def words_case(c, word_bits, values, seed, index=coefficient):
    """(batch, size, rank + 1, n): one encrypted word per value."""
    rng = seeded(seed)
    return np.stack([encrypt_word(c, v, word_bits, rng, index) for v in values])


def prepare_params(c, with_ks_glwe, word_bits, bit_start, bit_count):
    """pz_fhe_uint_prepare_params of a case (poulpy_amd.hal.FheUintPrepareParams)."""
    from poulpy_amd.hal import BlindRotationParams, CircuitBootstrappingParams, FheUintPrepareParams, GlweOpParams
    brk_b, atk_b, tsk_b, res_b = c.bases
    cbt = CircuitBootstrappingParams(
        br=BlindRotationParams(rank=c.rank, n_lwe=c.n_lwe, block_size=c.block_size, dnum=c.brk_dnum, brk_size=c.sh["glwe_size"], base2k=brk_b,
                               res_size=c.sh["glwe_size"], lut_size=c.lut.shape[1]),
        atk_dnum=c.atk_dnum, atk_size=c.atk[0].shape[2], tsk_dnum=c.tsk_dnum, tsk_size=c.tsk[0].shape[2], res_dnum=c.res_dnum, res_size=c.res_size,
        gap=c.gap, atk_base2k=atk_b, tsk_base2k=tsk_b, res_base2k=res_b, atk_glwe_size=c.sh["atk_glwe_size"], trace_size=c.sh["trace_size"])
    kg, kl = c.ks_glwe_key, c.ks_lwe_key["mid" if with_ks_glwe else "direct"]
    ks_glwe = GlweOpParams(rank=c.rank, dnum=kg.shape[0], dsize=1, key_size=kg.shape[2], key_base2k=c.ks_b, a_size=c.word_size, a_base2k=c.word_b,
                           res_size=c.mid_size, res_base2k=c.ks_b, rank_out=1)
    ks_lwe = GlweOpParams(rank=1 if with_ks_glwe else c.rank, dnum=kl.shape[0], dsize=1, key_size=kl.shape[2], key_base2k=c.ks_b,
                          a_size=c.mid_size if with_ks_glwe else c.word_size, a_base2k=c.ks_b if with_ks_glwe else c.word_b,
                          res_size=c.lwe_size, res_base2k=c.lwe_b, rank_out=1)
    return FheUintPrepareParams(cbt=cbt, ks_glwe=ks_glwe if with_ks_glwe else GlweOpParams(), ks_lwe=ks_lwe, n_lwe=c.n_lwe, lwe_size=c.lwe_size,
                                lwe_base2k=c.lwe_b, word_bits=word_bits, bit_start=bit_start, bit_count=bit_count)
