"""CPU: the restatement of CMUX, blind rotation by encrypted bits and blind selection (tests/cmux_oracle.py) means what it should - under
real keys (tests/fhe_sk.py: exact integer arithmetic, neither the oracle nor the device), with the reference's own test of the blind
rotation (poulpy-bin-fhe/src/bdd_arithmetic/tests/test_suite/glwe_blind_rotation.rs), and with the dense level-by-level blind selection of
poulpy_amd.bdd against the reference's sparse map."""
import numpy as np
import pytest

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import cmux_oracle as co
from tests import fhe_sk
from tests.helpers import seeded

_refs = {}


def _ref(n):
    from oracle.ref import RefModule
    if n not in _refs:
        _refs[n] = RefModule(n)
    return _refs[n]


def _prepared(ref, ggsw: np.ndarray):
    """fhe_sk.ggsw_encrypt's (dnum, rank + 1, size, rank + 1, n) array -> the oracle's prepared GGSW."""
    dnum, cols, size, _, n = ggsw.shape
    pm = ref.vmp_pmat_alloc(dnum, cols, cols, size)
    ref.vmp_prepare(pm, MatZnx(n, dnum, cols, cols, size, np.ascontiguousarray(ggsw)))
    return pm


def _bit_ggsw(ref, sk, bit, base2k, k_ggsw, dnum, dsize, rng):
    msg = np.zeros(sk.shape[1], dtype=np.int64)
    msg[0] = bit
    return _prepared(ref, fhe_sk.ggsw_encrypt(sk, msg, base2k, k_ggsw, dnum, dsize, rng))


def _ct(sk, data, base2k, k, k_pt, rng) -> VecZnx:
    size = fhe_sk.limbs_for(k, base2k)
    ct = fhe_sk.glwe_encrypt(sk, fhe_sk.encode(data, base2k, k_pt, size), base2k, k, rng)
    return VecZnx(sk.shape[1], sk.shape[0] + 1, size, np.ascontiguousarray(ct))


def _decode(ct: VecZnx, sk, base2k, k_pt):
    return co.decode_i64(fhe_sk.glwe_phase(ct.data, sk), base2k, k_pt)


# ---- 1. decode ------------------------------------------------------------------------------------------------------------------------
DECODE = [
    # n, rank, base2k, k_t, k_f, k_res, k_ggsw, dnum, dsize
    (256, 1, 13, 26, 26, 26, 39, 3, 1),
    (256, 2, 13, 26, 26, 26, 39, 3, 1),
    (512, 1, 12, 36, 24, 24, 48, 4, 1),      # t longer than f and res
    (256, 1, 10, 30, 30, 30, 50, 2, 2),      # dsize 2
]


@pytest.mark.parametrize("n,rank,base2k,k_t,k_f,k_res,k_ggsw,dnum,dsize", DECODE)
def test_every_form_decodes_to_t_or_f(n, rank, base2k, k_t, k_f, k_res, k_ggsw, dnum, dsize):
    """GGSW(1) selects t, GGSW(0) selects f, on every coefficient of every ciphertext, for cmux, cmux_assign and cmux_assign_neg."""
    ref, rng = _ref(n), seeded(8100 + n + rank + base2k)
    sk = fhe_sk.ternary_secret(n, rank, rng)
    k_pt, batch = 7, 3
    bits = {b: _bit_ggsw(ref, sk, b, base2k, k_ggsw, dnum, dsize, rng) for b in (0, 1)}
    for b in range(batch):
        t_msg = rng.integers(-60, 60, n, dtype=np.int64)
        f_msg = rng.integers(-60, 60, n, dtype=np.int64)
        for bit in (0, 1):
            want = t_msg if bit else f_msg
            t, f = _ct(sk, t_msg, base2k, k_t, k_pt, rng), _ct(sk, f_msg, base2k, k_f, k_pt, rng)
            res = VecZnx(n, rank + 1, fhe_sk.limbs_for(k_res, base2k))
            co.cmux(ref, res, t, f, bits[bit], base2k, dsize)
            assert np.array_equal(_decode(res, sk, base2k, k_pt), want), ("cmux", b, bit)
            # cmux_assign: res = t (layout of res), a = f
            r = _ct(sk, t_msg, base2k, k_res, k_pt, rng)
            co.cmux_assign(ref, r, f, bits[bit], base2k, dsize)
            assert np.array_equal(_decode(r, sk, base2k, k_pt), want), ("cmux_assign", b, bit)
            # cmux_assign_neg: res = f (layout of res), a = t
            r = _ct(sk, f_msg, base2k, k_res, k_pt, rng)
            co.cmux_assign_neg(ref, r, t, bits[bit], base2k, dsize)
            assert np.array_equal(_decode(r, sk, base2k, k_pt), want), ("cmux_assign_neg", b, bit)


class _Recorded:
    """The oracle module with the name of every per-op call kept, in order."""

    def __init__(self, ref):
        self._ref, self.calls = ref, []

    def __getattr__(self, name):
        attr = getattr(self._ref, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            self.calls.append(name)
            return attr(*args, **kw)
        return call


def test_a_ggsw_under_another_secret_gives_the_same_digits_and_no_decode():
    """Negative control: the restatement does not look at the secret.  With a GGSW of the bit under ANOTHER secret each of the three forms
    makes the same per-op calls in the same order as with the right one and returns digits of the same kind (shape, dtype, normalized);
    with the right GGSW the result decodes to t, with the other one to neither branch."""
    n, rank, base2k, k, k_ggsw, dnum, k_pt = 256, 1, 13, 26, 39, 3, 7
    ref, rng = _ref(n), seeded(8200)
    sk, other = fhe_sk.ternary_secret(n, rank, rng), fhe_sk.ternary_secret(n, rank, rng)
    t_msg, f_msg = rng.integers(-60, 60, n, dtype=np.int64), rng.integers(-60, 60, n, dtype=np.int64)
    t, f = _ct(sk, t_msg, base2k, k, k_pt, rng), _ct(sk, f_msg, base2k, k, k_pt, rng)
    ggsw = {"same": _bit_ggsw(ref, sk, 1, base2k, k_ggsw, dnum, 1, rng), "other": _bit_ggsw(ref, other, 1, base2k, k_ggsw, dnum, 1, rng)}

    def forms(rec, key):
        """-> the results of cmux, cmux_assign (res = t) and cmux_assign_neg (res = f) on copies of t and f"""
        res = VecZnx(n, rank + 1, t.size)
        co.cmux(rec, res, t, f, key, base2k)
        r_t = VecZnx(n, rank + 1, t.size, t.data.copy())
        co.cmux_assign(rec, r_t, f, key, base2k)
        r_f = VecZnx(n, rank + 1, f.size, f.data.copy())
        co.cmux_assign_neg(rec, r_f, t, key, base2k)
        return res, r_t, r_f

    recs = {which: _Recorded(ref) for which in ggsw}
    out = {which: forms(recs[which], ggsw[which]) for which in ggsw}
    assert recs["same"].calls and recs["other"].calls == recs["same"].calls
    for good, bad in zip(out["same"], out["other"]):
        assert bad.data.shape == good.data.shape and bad.data.dtype == good.data.dtype == np.int64
        assert np.abs(bad.data).max() <= 1 << (base2k - 1) and np.abs(good.data).max() <= 1 << (base2k - 1)
        assert np.array_equal(_decode(good, sk, base2k, k_pt), t_msg)
        got = _decode(bad, sk, base2k, k_pt)
        assert not np.array_equal(got, t_msg) and not np.array_equal(got, f_msg)
        assert np.count_nonzero(got != t_msg) > n // 2


def test_internal_product_restatement_matches_the_oracles_external_product():
    """glwe_external_product_internal + normalize = the oracle's own glwe_external_product, dsize 1 and 2."""
    n, cols, k = 256, 2, 12
    ref, rng = _ref(n), seeded(8300)
    for dsize, a_size, ksz, dnum, res_size in ((1, 3, 4, 3, 3), (2, 4, 5, 2, 3), (2, 3, 4, 2, 4)):
        pm = ref.vmp_pmat_alloc(dnum, cols, cols, ksz)
        ref.vmp_prepare(pm, MatZnx(n, dnum, cols, cols, ksz).fill_uniform(k, rng))
        a = VecZnx(n, cols, a_size).fill_uniform(k, rng)
        want = VecZnx(n, cols, res_size)
        ref.glwe_external_product(want, k, a, k, pm, dsize, k)
        big = co.glwe_external_product_internal(ref, a, pm, dsize)
        got = VecZnx(n, cols, res_size)
        for j in range(cols):
            ref.vec_znx_big_normalize(got, k, 0, j, big, k, j)
        assert np.array_equal(got.data, want.data), (dsize, a_size, ksz)


# ---- 2. the reference's own blind-rotation test ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rotation_setup():
    """test_suite/glwe_blind_rotation.rs:36-91: N = 256, base2k 13, rank 2, k_glwe 26, k_ggsw 39, dnum 3, data[i] = i, a 32-bit k."""
    n, base2k, rank, k_glwe, k_ggsw, dnum = 256, 13, 2, 26, 39, 3
    ref, rng = _ref(n), seeded(8400)
    sk = fhe_sk.ternary_secret(n, rank, rng)
    k = int(rng.integers(0, 1 << 32))
    bits = [_bit_ggsw(ref, sk, (k >> i) & 1, base2k, k_ggsw, dnum, 1, rng) for i in range(32)]
    size = fhe_sk.limbs_for(k_glwe, base2k)
    # the reference rotates the PLAINTEXT container (a GLWE whose mask is zero, :69-72 / :113-122)
    test_glwe = VecZnx(n, rank + 1, size)
    test_glwe.data[:, 0] = fhe_sk.encode(np.arange(n, dtype=np.int64), base2k, base2k, size)
    return dict(n=n, base2k=base2k, rank=rank, sk=sk, k=k, bits=bits, size=size, test_glwe=test_glwe, ref=ref)


def test_blind_rotation_passes_the_references_own_test(rotation_setup):
    s = rotation_setup
    ref, k = s["ref"], s["k"]
    for bit_start, bit_size, bit_step, mask in co.blind_rotation_walk(s["n"]):
        res = VecZnx(s["n"], s["rank"] + 1, s["size"])
        co.glwe_blind_rotation(ref, res, s["test_glwe"], lambda i: s["bits"][i], False, bit_start, bit_size, bit_step, s["base2k"])
        got = _decode(res, s["sk"], s["base2k"], s["base2k"])
        assert int(got[0]) == ((k >> bit_start) & mask) << bit_step, (bit_start, bit_size, bit_step)


def test_blind_rotation_rotates_every_coefficient_both_ways(rotation_setup):
    """Beyond coefficient 0: res = a X^{+-r} on the whole polynomial, and the assign form equals the out-of-place one."""
    s = rotation_setup
    ref, k, n = s["ref"], s["k"], s["n"]
    data = np.arange(n, dtype=np.int64)
    for sign in (False, True):
        r = ((k >> 3) & 7) << 2
        res = VecZnx(n, s["rank"] + 1, s["size"])
        co.glwe_blind_rotation(ref, res, s["test_glwe"], lambda i: s["bits"][i], sign, 3, 3, 2, s["base2k"])
        assert np.array_equal(_decode(res, s["sk"], s["base2k"], s["base2k"]), fhe_sk.rotate(data, r if sign else -r))
        inplace = s["test_glwe"].copy()
        co.glwe_blind_rotation_assign(ref, inplace, lambda i: s["bits"][i], sign, 3, 3, 2, s["base2k"])
        assert np.array_equal(inplace.data, res.data)


def test_ggsw_blind_rotation_is_the_same_call_on_the_entries(rotation_setup):
    """ggsw_blind_rotation (blind_rotation.rs:70-106) = glwe_blind_rotation on each of the dnum (rank + 1) contiguous GLWE entries."""
    s = rotation_setup
    ref, n, cols = s["ref"], s["n"], s["rank"] + 1
    rng = seeded(8450)
    a = MatZnx(n, 2, cols, cols, s["size"]).fill_uniform(s["base2k"], rng)
    res = MatZnx(n, 2, cols, cols, s["size"])
    co.ggsw_blind_rotation(ref, res, a, lambda i: s["bits"][i], True, 1, 2, 0, s["base2k"])
    flat_a, flat_r = a.data.reshape(2 * cols, s["size"], cols, n), res.data.reshape(2 * cols, s["size"], cols, n)
    for e in range(2 * cols):
        one = VecZnx(n, cols, s["size"])
        co.glwe_blind_rotation(ref, one, VecZnx(n, cols, s["size"], np.ascontiguousarray(flat_a[e])), lambda i: s["bits"][i], True, 1, 2, 0, s["base2k"])
        assert np.array_equal(flat_r[e], one.data), e


# ---- 3. blind selection: the dense level-by-level sequence against the sparse map -----------------------------------------------------
@pytest.mark.parametrize("present", [tuple(range(8)), (0, 2, 3, 7), (5,), (1, 4, 6), ()], ids=["full", "holes", "one", "odd", "empty"])
def test_dense_blind_selection_equals_the_sparse_map(present):
    """All layouts equal: one cmux_assign per pair over the last 2t slots, absent entries as zero ciphertexts, gives the digits of the
    reference's HashMap walk (blind_selection.rs:59-103) - and selects entry (k >> bit_rsh) mod 8."""
    n, rank, base2k, k_glwe, k_ggsw, dnum, k_pt, bit_mask, bit_rsh = 256, 1, 13, 26, 39, 3, 7, 3, 1
    ref, rng = _ref(n), seeded(8500 + len(present))
    sk = fhe_sk.ternary_secret(n, rank, rng)
    k = int(rng.integers(0, 1 << 8))
    bits = [_bit_ggsw(ref, sk, (k >> i) & 1, base2k, k_ggsw, dnum, 1, rng) for i in range(bit_rsh + bit_mask)]
    size = fhe_sk.limbs_for(k_glwe, base2k)
    msgs = {i: rng.integers(-60, 60, n, dtype=np.int64) for i in present}
    cts = {i: _ct(sk, msgs[i], base2k, k_glwe, k_pt, rng) for i in present}
    sparse = VecZnx(n, rank + 1, size)
    sparse.data[...] = 0x5A
    co.glwe_blind_selection(ref, sparse, {i: c.copy() for i, c in cts.items()}, lambda i: bits[i], bit_rsh, bit_mask, base2k)
    slots = [cts[i].copy() if i in cts else VecZnx(n, rank + 1, size) for i in range(1 << bit_mask)]
    dense = co.glwe_blind_selection_dense(ref, slots, lambda i: bits[i], bit_rsh, bit_mask, base2k)
    assert np.array_equal(dense.data, sparse.data)
    sel = (k >> bit_rsh) & ((1 << bit_mask) - 1)
    want = msgs.get(sel, np.zeros(n, dtype=np.int64))
    assert np.array_equal(_decode(sparse, sk, base2k, k_pt), want), (sel, present)
