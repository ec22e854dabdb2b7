"""CPU: the restatement of the conditional swap and of blind retrieval (tests/cswap_oracle.py) means what it should - under real keys
(tests/fhe_sk.py: exact integer arithmetic, neither the oracle nor the device), following the reference's own tests
(poulpy-bin-fhe/src/bdd_arithmetic/tests/test_suite/swap.rs:21-91 and :93-153) - and the dense level list the device entry point walks is the
reference's pair list."""
import math

import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import cmux_oracle as co
from tests import cswap_oracle as cs
from tests import fhe_sk
from tests.helpers import seeded

N, RANK, BASE2K, SIZE, DNUM, K_PT = 256, 1, 12, 3, 3, 7
K_GLWE, K_GGSW = BASE2K * SIZE, BASE2K * (SIZE + 1)

_refs = {}


def _ref(n):
    from oracle.ref import RefModule
    if n not in _refs:
        _refs[n] = RefModule(n)
    return _refs[n]


def _bit_ggsw(ref, sk, bit, rng):
    msg = np.zeros(sk.shape[1], dtype=np.int64)
    msg[0] = bit
    g = fhe_sk.ggsw_encrypt(sk, msg, BASE2K, K_GGSW, DNUM, 1, rng)
    dnum, cols, size, _, n = g.shape
    pm = ref.vmp_pmat_alloc(dnum, cols, cols, size)
    ref.vmp_prepare(pm, MatZnx(n, dnum, cols, cols, size, np.ascontiguousarray(g)))
    return pm


def _ct(sk, data, rng) -> VecZnx:
    ct = fhe_sk.glwe_encrypt(sk, fhe_sk.encode(data, BASE2K, K_PT, SIZE), BASE2K, K_GLWE, rng)
    return VecZnx(sk.shape[1], sk.shape[0] + 1, SIZE, np.ascontiguousarray(ct))


def _decode(ct: VecZnx, sk):
    return co.decode_i64(fhe_sk.glwe_phase(ct.data, sk), BASE2K, K_PT)


def _noise(ct: VecZnx, sk, msg) -> float:
    return fhe_sk.noise_log2(ct.data, BASE2K, sk, fhe_sk.encode(msg, BASE2K, K_PT, SIZE), BASE2K)


def noise_bound() -> float:
    """One external product plus the added operand: the reference's bound for the product (external_product/glwe_ct.rs:133-152, as
    fhe_sk.external_product_bound states it, its + 1 bit of slack included) and the fresh operand's own encryption noise (sigma 2^-k),
    added as variances.  The difference b - a that enters the product carries two fresh noises and a message of 2 x 60 2^-K_PT at most; the
    bound's var_msg = 1 / n model is for a monomial message, so the message term is restated for this one."""
    var_msg = (120.0 * 2.0 ** -K_PT) ** 2
    prod = fhe_sk.noise_ggsw_product(N, BASE2K, 0.5, var_msg, 2 * fhe_sk.SIGMA ** 2, 2.0 / 12.0, fhe_sk.SIGMA ** 2, 0.0, RANK, K_GLWE, K_GGSW) + 1.0
    return 0.5 * math.log2(4.0 ** prod + (fhe_sk.SIGMA * 2.0 ** -K_GLWE) ** 2)


def test_cswap_swaps_under_one_and_keeps_under_zero():
    """swap.rs:21-91: after cswap the pair decrypts to (a, b) under GGSW(0) and to (b, a) under GGSW(1), within the noise of one external
    product plus the operand; with the GGSW of the other bit the decoded pair is the wrong one (negative control)."""
    ref, rng = _ref(N), seeded(9100)
    sk = fhe_sk.ternary_secret(N, RANK, rng)
    bits = {v: _bit_ggsw(ref, sk, v, rng) for v in (0, 1)}
    bound = noise_bound()
    for trial in range(2):
        a_msg, b_msg = rng.integers(-60, 60, N, dtype=np.int64), rng.integers(-60, 60, N, dtype=np.int64)
        assert not np.array_equal(a_msg, b_msg)
        for bit in (0, 1):
            a, b = _ct(sk, a_msg, rng), _ct(sk, b_msg, rng)
            cs.cswap(ref, a, b, bits[bit], BASE2K)
            want_a, want_b = (b_msg, a_msg) if bit else (a_msg, b_msg)
            assert np.array_equal(_decode(a, sk), want_a) and np.array_equal(_decode(b, sk), want_b), (trial, bit)
            na, nb = _noise(a, sk, want_a), _noise(b, sk, want_b)
            print(f"cswap bit {bit}: noise log2 a' {na:.2f} b' {nb:.2f} bound {bound:.2f}")
            assert na <= bound and nb <= bound, (na, nb, bound)
            # negative control: the pair the other bit would have given is not what came out
            assert not np.array_equal(_decode(a, sk), want_b) and not np.array_equal(_decode(b, sk), want_a)
            assert np.abs(a.data).max() <= 1 << (BASE2K - 1) and np.abs(b.data).max() <= 1 << (BASE2K - 1)


def test_cswap_is_one_product_and_reads_the_big_value_for_both_results():
    """The two results come from ONE glwe_external_product_internal: one vmp call, and a' + b' = a + b on the torus (the big value cancels)."""
    ref, rng = _ref(N), seeded(9150)
    sk = fhe_sk.ternary_secret(N, RANK, rng)
    calls = []

    class Rec:
        def __getattr__(self, name):
            attr = getattr(ref, name)
            if not callable(attr):
                return attr

            def call(*args, **kw):
                calls.append(name)
                return attr(*args, **kw)
            return call

    a, b = VecZnx(N, RANK + 1, SIZE).fill_uniform(BASE2K, rng), VecZnx(N, RANK + 1, SIZE).fill_uniform(BASE2K, rng)
    a0, b0 = a.copy(), b.copy()
    cs.cswap(Rec(), a, b, _bit_ggsw(ref, sk, 1, rng), BASE2K)
    assert calls.count("vmp_apply_dft_to_dft") == 1
    for col in range(RANK + 1):
        before = fhe_sk.to_int(a0.data[:, col], BASE2K) + fhe_sk.to_int(b0.data[:, col], BASE2K)
        after = fhe_sk.to_int(a.data[:, col], BASE2K) + fhe_sk.to_int(b.data[:, col], BASE2K)
        assert all(int(x) % (1 << (BASE2K * SIZE)) == 0 for x in (after - before))


@pytest.mark.parametrize("idx", range(5))
def test_blind_retrieval_moves_the_indexed_element_to_slot_zero_and_back(idx):
    """swap.rs:93-153 shrunk to 5 slots (the smallest length with a full and a clipped level), bit_mask 3, behind a bit_rsh of 1: slot 0
    decrypts to data[idx]; _rev restores all 5."""
    ref, rng = _ref(N), seeded(9200 + idx)
    sk = fhe_sk.ternary_secret(N, RANK, rng)
    bit_rsh, bit_mask = 1, 3
    k = (idx << bit_rsh) | int(rng.integers(0, 2))
    bits = [_bit_ggsw(ref, sk, (k >> i) & 1, rng) for i in range(bit_rsh + bit_mask)]
    msgs = [rng.integers(-60, 60, N, dtype=np.int64) for _ in range(5)]
    slots = [_ct(sk, m, rng) for m in msgs]
    cs.glwe_blind_retrieval(ref, slots, lambda i: bits[i], bit_rsh, bit_mask, BASE2K)
    assert np.array_equal(_decode(slots[0], sk), msgs[idx])
    others = [j for j in range(5) if j != idx]
    assert all(not np.array_equal(_decode(slots[0], sk), msgs[j]) for j in others)
    cs.glwe_blind_retrieval_rev(ref, slots, lambda i: bits[i], bit_rsh, bit_mask, BASE2K)
    for j in range(5):
        assert np.array_equal(_decode(slots[j], sk), msgs[j]), (idx, j)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("nslots", [1, 2, 3, 5, 8, 9])
def test_retrieval_levels_are_the_reference_loops(nslots, reverse):
    """Level (t, bit, cnt) of the dense form = the pairs (j, j + t), j < cnt, under that bit - the reference's pair list, in its order."""
    nbits = 3
    pairs = []
    for t, bit, cnt in cs.retrieval_levels(nslots, nbits, reverse):
        assert cnt <= t and (cnt == 0 or t + cnt <= nslots)
        pairs += [(bit, j, j + t) for j in range(cnt)]
    assert pairs == cs.reference_pairs(nslots, nbits, reverse)
    assert len(cs.retrieval_levels(nslots, nbits, reverse)) == nbits
