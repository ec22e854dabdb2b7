"""pz_glwe_automorphism_many_batched under real keys: three ciphertexts encrypted under one secret key (tests/fhe_sk.py), rotated by three
Galois elements - each with its own real automorphism key - in one call.  Device == oracle bit for bit, every output decrypts to phi_p of its
own plaintext within the reference's noise bound (tests/core_cases.py), and with two keys swapped the decryption fails.
noise_have / noise_want are printed (`-s`)."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

from tests import core_cases as cs
from tests import test_gpu_rotations as rot

pytestmark = pytest.mark.gpu

N, LIMBS, BASE2K, BATCH = 8192, 3, 12, 3
GALS = (5, 3, 2 * N - 1)


@pytest.fixture(scope="module")
def mods():
    from oracle.ref import RefModule
    from poulpy_amd.hal import Module
    return RefModule(N), Module(N)


@pytest.fixture(scope="module")
def cases():
    """one case per Galois element from the same seed: the same secret key and ciphertexts, the automorphism key of that element"""
    k = LIMBS * BASE2K
    cc = [cs.automorphism_case(N, 1, 1, LIMBS, BASE2K, BASE2K, BASE2K, k, k, k, 1, BATCH, 7331, p=p) for p in GALS]
    for c in cc[1:]:
        assert np.array_equal(c.a, cc[0].a) and np.array_equal(c.sk_out, cc[0].sk_out)
    return cc


def _rotate(hip, cc, keys):
    c0 = cc[0]
    rows, cols_in, ksz, cols_out, n = c0.key.shape
    from poulpy_amd.layouts import MatZnx
    mats = [MatZnx(n, rows, cols_in, cols_out, ksz, np.ascontiguousarray(k)) for k in keys]
    a = np.ascontiguousarray(c0.a)
    c = SimpleNamespace(n=n, rank=1, cols=cols_out, a_size=a.shape[1], a_base2k=BASE2K, key_size=ksz, key_base2k=BASE2K, dnum=rows, dsize=1,
                            res_size=c0.res_size, res_base2k=BASE2K, batch=len(a), gals=[p % (2 * n) for p in GALS], mats=mats, a=a)
    got, notes, _, _, _ = rot.run_device(hip, c)
    return got, notes


def test_rotations_decrypt_each_under_its_own_key(mods, cases):
    ref, hip = mods
    got, notes = _rotate(hip, cases, [c.key for c in cases])
    assert rot.HOISTED in notes, notes
    for r, c in enumerate(cases):
        assert np.array_equal(got[r], cs.run_oracle(ref, c)), ("device != oracle", GALS[r])
        cs.check(("rotation", GALS[r]), c, got[r])


def test_swapped_keys_fail_to_decrypt(mods, cases):
    ref, hip = mods
    keys = [cases[1].key, cases[0].key, cases[2].key]
    got, _ = _rotate(hip, cases, keys)
    for r in (0, 1):
        wrong = copy.copy(cases[r])
        wrong.key = keys[r]
        assert np.array_equal(got[r], cs.run_oracle(ref, wrong)), ("device != oracle", GALS[r])
        cs.check(("swapped keys", GALS[r]), wrong, got[r], fail=True)
    cs.check(("untouched rotation", GALS[2]), cases[2], got[2])
