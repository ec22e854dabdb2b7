"""Inputs shared by tests/test_ckks_mul_host.py and tests/test_gpu_ckks_mul.py: the scenarios of the ciphertext products (the reference's own
cases from poulpy-ckks leveled/tests/test_suite/{mul,mul_add,mul_sub,mul_many,composition}.rs restated as layouts and metadata), random
containers and tensor keys for the limb comparisons, and the decrypted cases under a real key with what they must decrypt to.

A fresh ciphertext of the reference's test context is encrypted at k with log_delta d: effective_k = max_k = k (helpers.rs:411-417)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from poulpy_amd import ckks
from poulpy_amd.ckks import Ct
from poulpy_amd.layouts import MatZnx, VecZnx
from tests import fhe_sk as fs
from tests import tensor_cases as tc
from tests.helpers import seeded

D = 20            # log_delta of every scenario


def fresh(B, k, cols=2, log_delta=D) -> Ct:
    """ctx.encrypt(k, ...): a container of k.div_ceil(base2k) limbs, log_budget = k - log_delta"""
    return Ct(B, -(-k // B), log_delta, k - log_delta, cols)


def mul_scenarios(B, cols=2, limbs=5):
    """(label, dst layout (size), a, b): mul.rs's aligned / one input one limb short (encrypted at max_k - base2k + 1) / smaller output
    (max_k - base2k - 1), and an operand that a rescale has left with fewer effective limbs than its container holds."""
    K = limbs * B
    short = fresh(B, K - B + 1, cols)
    rescaled = Ct(B, limbs, D, K - D - B - 3, cols)            # rescale_assign by base2k + 3 bits: the container keeps its limbs
    return [("aligned", limbs, fresh(B, K, cols), fresh(B, K, cols)),
            ("one input one limb short", limbs, fresh(B, K, cols), short),
            ("smaller output", -(-(K - B - 1) // B), fresh(B, K, cols), fresh(B, K, cols)),
            ("rescaled operand in its container", limbs, rescaled, fresh(B, K, cols)),
            ("both rescaled, smaller output", limbs - 2, rescaled, Ct(B, limbs, D, K - D - B, cols))]


def mul_many_scenarios(B, cols=2, limbs=10):
    """(label, dst size, inputs): mul_many.rs's aligned (4), single into a narrower output, odd tree (5), one input one limb short (input 2
    of 4), smaller output (4); then every count 1 .. 9 with input 1 at a lower budget (7 bits; from 5 inputs on by more than a limb, so
    that its effective limbs are fewer than its container's)."""
    K = limbs * B
    out = [("aligned", limbs, [fresh(B, K, cols) for _ in range(4)]),
           ("single, smaller output", -(-(K - B - 1) // B), [fresh(B, K, cols)]),
           ("odd tree", limbs, [fresh(B, K, cols) for _ in range(5)]),
           ("unaligned log_budget", limbs, [fresh(B, K - B + 1 if i == 2 else K, cols) for i in range(4)]),
           ("smaller output", -(-(K - B - 1) // B), [fresh(B, K, cols) for _ in range(4)])]
    for n in range(1, 10):
        out.append((f"n = {n}, one lower budget", limbs, [Ct(B, limbs, D, K - D - ((7 if n < 5 else 15) if i == 1 else 0), cols) for i in range(n)]))
    return out


def fill_ct(rng, n, ct: Ct, normalized=True) -> Ct:
    """a copy of the layout with random digits in EVERY limb of the container (the limbs past effective_k too: the product must not read them)"""
    v = VecZnx(n, ct.cols, ct.size)
    h = 1 << (ct.base2k - 1 if normalized else ct.base2k + 3)
    v.data[...] = rng.integers(-h, h, v.data.shape, dtype=np.int64)
    return Ct(ct.base2k, ct.size, ct.log_delta, ct.log_budget, ct.cols, v)


def random_tensor_key(rng, n, B, rank, dnum, key_size) -> MatZnx:
    """a tensor key's shape with uniform digits: enough for limb comparisons"""
    return MatZnx(n, dnum, rank * (rank + 1) // 2, rank + 1, key_size).fill_uniform(B, rng)


# ---- decrypted cases ----------------------------------------------------------------------------------------------------------------------
# A ciphertext (log_delta, log_budget) of effective_k E that holds the integer polynomial M has the phase M 2^-E (+ noise at 2^-E, + an
# integer polynomial I).  ckks_mul_into at res_offset 0 has cnv_offset = E: the tensor's phase is phase_a phase_b 2^E (tests/tensor_cases.py),
# I_a (M_b + e_b) 2^(E - E_b) is an integer polynomial, and what is left is (M_a + e_a)(M_b + e_b) 2^(E - E_a - E_b).  Messages are
# M = m 2^s with m ternary, so that a product stands 2^s above the noise M e it carries.
#
# Bounds.  tests/tensor_cases.py::reference_bound(n, rank, k, cnv_offset) with k the inputs' encryption precision is asserted as it stands;
# at cnv_offset = k it is log2 N + 0.5, which no torus element misses.  The statement that tells a right result from a wrong one is the
# second bound, from the number format: the deviation stays below 1 / 8 of the unit the exact product is counted in, `unit_bits - 3`.
def _ternary(n, rng):
    return rng.integers(-1, 2, n, dtype=np.int64)


def _encrypt(sk, m, shift, B, E, size, rng):
    return fs.glwe_encrypt(sk, fs.encode(m << shift, B, E, size), B, E, rng)


def _noise(ct_data, B, sk, want_int, bits):
    """log2 of the deviation of phase(ct) - want 2^-bits mod 1"""
    e = fs.torus_diff(fs.glwe_phase(ct_data, sk), B, fs.torus_from_int(want_int, bits, tc.WANT_BASE2K), tc.WANT_BASE2K)
    sd = float(np.std(e))
    return math.log2(sd) if sd > 0 else -math.inf


def check_decrypt(label, c, ct_data, want_int, bits, cnv_offset, fail=False):
    have = _noise(ct_data, c.B, c.sk, want_int, bits)
    ref_bound = tc.reference_bound(c.n, c.rank, c.E, cnv_offset)
    unit_bound = -bits - 3.0
    print(f"[noise] {label}: noise_have {have:.2f} reference_bound {ref_bound:.2f} unit bound {unit_bound:.2f}")
    if fail:
        assert have > min(ref_bound, unit_bound), (label, have, "a negative control met the bound")
    else:
        assert have <= ref_bound and have <= unit_bound, (label, have, ref_bound, unit_bound)
    return have


def decrypt_case(n, rank, seed, B=12, E=72, s=16):
    """secret, tensor key and four fresh ciphertexts a, b, c, d (E bits, log_delta 20, messages m 2^s) - and what the host and the device
    tests build from them."""
    rng = seeded(seed)
    size = E // B
    sk = fs.ternary_secret(n, rank, rng)
    key = fs.tensor_key(sk, B, E + B, size, 1, rng)          # dnum = the widest tensor's limbs, one limb more of precision
    ms = [_ternary(n, rng) for _ in range(4)]
    cts = [_encrypt(sk, m, s, B, E, size, rng) for m in ms]
    return SimpleNamespace(n=n, rank=rank, cols=rank + 1, B=B, E=E, s=s, size=size, sk=sk, key=key, ms=ms, cts=cts, rng=rng,
                           tsk=(size, 1, size + 1, B))


def ct_of(c, i) -> Ct:
    x = c.cts[i]
    return Ct(c.B, c.size, D, c.E - D, c.cols, VecZnx(c.n, c.cols, c.size, np.ascontiguousarray(x.copy())))
