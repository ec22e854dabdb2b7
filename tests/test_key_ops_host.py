"""Key composition and the GGSW forms of key switching on the host side (no GPU): the reference's encrypt / compose / measure test of
glwe_automorphism_key_automorphism restated on the oracle (tests/key_ops_cases.py), the identity the device's fast form rests on stated
on exact integers, and the three entry points in the built library, the C header and poulpy_amd.hal."""
import ctypes as C
import os

import numpy as np
import pytest

from poulpy_amd.layouts import VecZnx
from tests import fhe_sk as fs
from tests import key_ops_cases as kc
from tests.helpers import seeded

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_SYMBOLS = ("pz_glwe_automorphism_key_automorphism_batched", "pz_ggsw_keyswitch_batched", "pz_ggsw_automorphism_batched")
N, BASE2K = 256, 17


@pytest.fixture(scope="module")
def ref():
    from oracle.ref import RefModule
    return RefModule(N)


def _max_dsize():
    return -(-(4 * (BASE2K - 1) + 1) // BASE2K)


# ---- 1. semantics on the oracle (test_suite/automorphism/gglwe_atk.rs:20-185) ----
@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("dsize", range(1, _max_dsize() + 1))
def test_key_composition_semantics_on_the_oracle(ref, rank, dsize):
    c = kc.composition_case(N, BASE2K, rank, dsize, seed=100 * rank + dsize)
    pm = kc.prepare(ref, c.key_apply)
    out = kc.key_composition(ref, c.key_in, c.in_b, c.p0, pm, dsize, c.key_b, c.dnum_in, c.res_size)
    have = kc.composition_noise(c, out)
    print(f"[noise] key composition rank {rank} dsize {dsize}: noise_have {max(have):.2f} noise_want {c.bound:.2f}")
    assert max(have) <= c.bound, (have, c.bound)
    # negative control: the input key declared with the Galois element of the applied one
    bad = kc.key_composition(ref, c.key_in, c.in_b, c.p1, pm, dsize, c.key_b, c.dnum_in, c.res_size)
    have_bad = kc.composition_noise(c, bad)
    assert min(have_bad) > c.bound, (have_bad, c.bound, "a negative control met the bound")
    # the derived key works: glwe_automorphism with gal = p0 p1 decrypts to phi_{p0 p1}(pt)
    gal = (c.p0 * c.p1) % (2 * N)
    pmd = kc.prepare(ref, out)
    a_size = fs.limbs_for(c.k_in, c.in_b)
    pt = fs.uniform_digits((a_size, N), c.in_b, c.rng)
    ct = fs.glwe_encrypt(c.sk, pt, c.in_b, c.k_in, c.rng)
    res = VecZnx(N, rank + 1, c.res_size)
    ref.glwe_automorphism(res, c.in_b, VecZnx(N, rank + 1, a_size, ct), c.in_b, pmd, 1, c.in_b, gal, "automorphism")
    noise = fs.noise_log2(res.data, c.in_b, c.sk, fs.automorphism(pt, gal), c.in_b)
    want = kc.derived_key_bound(c)
    print(f"[noise] automorphism by the derived key: noise_have {noise:.2f} noise_want {want:.2f}")
    assert noise <= want, (noise, want)
    assert want < -(c.in_b + 2), "the bound itself must leave the top limb of the message intact"


# ---- 2. the identity, FFT-free: phi_g(normalize(phi_p(B))) == s .* normalize(s .* B) ----
def _phi_obj(x, p):
    n = x.shape[-1]
    idx = (np.arange(n, dtype=np.int64) * (int(p) % (2 * n))) % (2 * n)
    out = np.zeros_like(x)
    pos = idx < n
    out[..., idx[pos]] = x[..., pos]
    out[..., idx[~pos] - n] = -x[..., ~pos]
    return out


@pytest.mark.parametrize("n,base2k,limbs", [(64, 12, 4), (256, 5, 3)])
def test_signs_around_the_carry_chain_identity(n, base2k, limbs):
    rng = seeded(n + base2k)
    h = 1 << (base2k - 1)
    big = rng.integers(-(1 << (base2k + 6)), 1 << (base2k + 6), (limbs, n)).astype(object)
    # planted ties: digits exactly +-2^(base2k-1) in every limb position, alone and stacked (a tie whose carry lands on a tie)
    for j in range(limbs):
        big[j, 2 * j] = h
        big[j, 2 * j + 1] = -h
        big[:, 2 * limbs + j] = 0
        big[j, 2 * limbs + j] = h if j % 2 else -h
    big[:, 3 * limbs] = h
    big[:, 3 * limbs + 1] = -h
    big[:, 3 * limbs + 2] = h - 1
    big[limbs - 1, 3 * limbs + 2] = h
    differs = False
    for p in (1, 5, n + 1, 3, -1, -5, 2 * n - 1, 2 * n - 5, 2 * n - 3):
        assert (p % 4) in (1, 3)
        g = fs.galois_inv(p, n)
        want = _phi_obj(kc.normalize_big(_phi_obj(big, p), base2k), g)
        s = kc.galois_signs(n, p)
        got = s * kc.normalize_big(s * big, base2k)
        assert np.array_equal(want, got), p
        plain = kc.normalize_big(big, base2k)
        if p % (2 * n) == 1:
            assert np.array_equal(got, plain)
        elif not np.array_equal(got, plain):
            differs = True
            assert kc.has_tie_sign(got.astype(np.int64), base2k)
    assert differs, "no planted tie met a minus sign: the cases would not tell the sign rule from a plain carry chain"
    assert {p % 4 for p in (5, -5)} == {1, 3}


# ---- 3. bindings ----
def test_library_exports_the_entry_points():
    from poulpy_amd.hal import load_library
    lib = load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None


def test_header_and_mirrors_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "poulpy_hip.h")) as f:
        h = f.read()
    for name in NEW_SYMBOLS:
        assert name in h, name
    with open(os.path.join(ROOT, "include", "poulpy_hip.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")) as f:
        rs = f.read()
    for name in NEW_SYMBOLS:
        assert name[3:] in hpp and name[3:] in rs, name


class _FakeLib:
    """Stands in for the library where no device exists: records the call, reports success."""
    def __init__(self, n):
        self.n, self.calls = n, []

    def pz_glwe_automorphism_key_automorphism_batched(self, *args):
        self.calls.append(args)
        return 0


@pytest.mark.parametrize("a_gal,key_gal", [(-1, -5), (5, 25), (2 * 256 - 5, 3), (1, 1)])
def test_hal_returns_the_galois_element_of_the_result(a_gal, key_gal):
    from poulpy_amd import hal
    m = object.__new__(hal.Module)
    m.lib, m.handle, m._n = _FakeLib(256), None, 256
    p = hal.GlweOpParams(rank=1, dnum=2, dsize=1, key_size=2, key_base2k=12, a_size=2, a_base2k=12, res_size=2, res_base2k=12, rank_out=1)
    got = m.glwe_automorphism_key_automorphism_batched(None, 2, None, 2, a_gal, None, key_gal, p, 1)
    assert got == (a_gal * key_gal) % 512 and 0 <= got < 512 and got % 2 == 1
    assert len(m.lib.calls) == 1 and m.lib.calls[0][5] == a_gal
    for name in ("ggsw_keyswitch_batched", "ggsw_automorphism_batched"):
        assert callable(getattr(hal.Module, name)), name


def _params(hal, **kw):
    d = dict(rank=1, dnum=2, dsize=1, key_size=2, key_base2k=12, a_size=2, a_base2k=12, res_size=2, res_base2k=12, rank_out=1)
    d.update(kw)
    return hal.GlweOpParams(**d)


def test_bad_arguments_are_refused_before_any_launch():
    """The argument checks come before the module is touched: with no module at all an even Galois element, more result rows than input
    rows and two bases are named as such (and good arguments reach the module check)."""
    from poulpy_amd import abi, hal
    lib = hal.load_library()
    f = lib.pz_glwe_automorphism_key_automorphism_batched

    def call(res_dnum, a_dnum, a_gal, p):
        st = f(None, None, res_dnum, None, a_dnum, a_gal, None, C.byref(p), 1)
        return st, lib.pz_last_error().decode()
    st, msg = call(2, 2, 4, _params(hal))
    assert st == abi.PZ_ERR_INVALID and "odd" in msg, msg
    st, msg = call(3, 2, 5, _params(hal))
    assert st == abi.PZ_ERR_INVALID and "rows" in msg, msg
    st, msg = call(2, 2, 5, _params(hal, res_base2k=11))
    assert st == abi.PZ_ERR_INVALID and "base2k" in msg, msg
    st, msg = call(2, 2, 5, _params(hal))
    assert st == abi.PZ_ERR_INVALID and "null module" in msg, msg
    g = lib.pz_ggsw_automorphism_batched
    arr = (C.c_void_p * 1)(None)
    st = g(None, None, 2, None, 2, None, 6, arr, C.byref(_params(hal)), C.byref(_params(hal)), 1)
    assert st == abi.PZ_ERR_INVALID and "odd" in lib.pz_last_error().decode()
    st = g(None, None, 3, None, 2, None, 5, arr, C.byref(_params(hal)), C.byref(_params(hal)), 1)
    assert st == abi.PZ_ERR_INVALID and "rows" in lib.pz_last_error().decode()


# ---- 1b. the GGSW forms on the oracle (test_suite/keyswitch/ggsw_ct.rs, test_suite/automorphism/ggsw_ct.rs) ----
@pytest.mark.parametrize("op", ["ks", "auto"])
@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("dsize", range(1, _max_dsize() + 1))
def test_ggsw_forms_semantics_on_the_oracle(ref, op, rank, dsize):
    c = kc.ggsw_case(op, N, BASE2K, rank, dsize, seed=300 + 10 * rank + dsize)
    kc.ggsw_check((op, rank, dsize), c, kc.ggsw_run_oracle(ref, c))
    bad = kc.ggsw_case(op, N, BASE2K, rank, dsize, seed=300 + 10 * rank + dsize, control=True)
    kc.ggsw_check((op, rank, dsize, "control"), bad, kc.ggsw_run_oracle(ref, bad), fail=True)
