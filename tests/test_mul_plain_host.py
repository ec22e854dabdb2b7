"""GLWE x plaintext / x constant on the host side (no GPU): the oracle compositions of tests/plain_oracle.py against an FFT-free exact
statement (oracle/exact.py), and the new entry points in the built library, the C header and poulpy_amd.hal."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.exact import negacyclic_mul, normalize_exact, torus_equal
from poulpy_amd.layouts import VecZnx
from tests import plain_oracle as po
from tests.helpers import seeded

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_SYMBOLS = ("pz_glwe_mul_plain_workspace_bytes", "pz_glwe_mul_plain_batched", "pz_glwe_mul_const_batched")


@pytest.fixture(scope="module")
def refs():
    from oracle.ref import RefModule
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = RefModule(n)
        return cache[n]
    return get


def _masked(a: np.ndarray, base2k: int, k: int) -> np.ndarray:
    out = a.copy()
    out[-1] &= np.int64(po.msb_mask_bottom_limb(base2k, k))
    return out


def _big_plain(a_col: np.ndarray, b_col: np.ndarray, hi: int, big_size: int) -> np.ndarray:
    """res_big limb kk = sum_j a[kk + hi - j] * b[j] in Z[X]/(X^N + 1), exactly (convolution.rs:210-260 without the FFT)."""
    a_size, b_size, n = a_col.shape[0], b_col.shape[0], a_col.shape[1]
    out = np.zeros((big_size, n), dtype=object)
    for kk in range(big_size):
        k = kk + hi
        for j in range(b_size):
            if 0 <= k - j < a_size:
                out[kk] = out[kk] + negacyclic_mul(a_col[k - j], b_col[j])
    return out


def _big_const(a_col: np.ndarray, b, hi: int, big_size: int) -> np.ndarray:
    a_size, n = a_col.shape
    out = np.zeros((big_size, n), dtype=object)
    for kk in range(big_size):
        k = kk + hi
        for j, bj in enumerate(b):
            if 0 <= k - j < a_size:
                out[kk] = out[kk] + a_col[k - j].astype(object) * int(bj)
    return out


def _check_column(big: np.ndarray, in_base2k: int, res_col: np.ndarray, res_base2k: int, lo: int):
    """lo = 0 at one base: the exact digits; otherwise the torus criterion of the reference's normalize tests."""
    if lo == 0 and in_base2k == res_base2k:
        assert np.array_equal(normalize_exact(big, in_base2k, res_col.shape[0]), res_col)
    else:
        assert torus_equal(big, in_base2k, res_col, res_base2k, res_offset=lo, slack_bits=1)


# (n, rank, a_size, b_size, res_size, ab_base2k, res_base2k, cnv_offset, a_bits_off, b_bits_off)
PLAIN_CASES = [
    (64, 1, 4, 3, 5, 12, 12, 24, 0, 0),      # hi = 1, lo = 0: exact digits
    (64, 2, 3, 2, 4, 13, 13, 5, 3, 2),       # cnv_offset < base2k: hi = 0, lo < 0; masked bottom limbs
    (256, 1, 4, 4, 6, 12, 15, 30, 7, 0),     # cross-base, lo > 0
    (256, 2, 5, 1, 4, 14, 14, 42, 0, 5),     # one-limb plaintext
]


@pytest.mark.parametrize("case", PLAIN_CASES)
def test_glwe_mul_plain_oracle_vs_exact(refs, case):
    n, rank, a_size, b_size, res_size, ab, rb, off, abo, bbo = case
    ref = refs(n)
    rng = seeded(n + rank + off)
    cols = rank + 1
    a = VecZnx(n, cols, a_size).fill_uniform(ab, rng)
    b = VecZnx(n, 1, b_size).fill_uniform(ab, rng)
    a_k, b_k = ab * a_size - abo, ab * b_size - bbo
    res = VecZnx(n, cols, res_size)
    po.glwe_mul_plain(ref, off, res, rb, a, a_k, b, b_k, ab)
    hi, lo = po.offset_split(off, ab)
    am = np.stack([_masked(a.data[:, c], ab, a_k) for c in range(cols)], axis=1)
    bm = _masked(b.data[:, 0], ab, b_k)
    for c in range(cols):
        _check_column(_big_plain(am[:, c], bm, hi, a_size + b_size - hi), ab, res.data[:, c], rb, lo)
    if rb == ab:   # the assign form on the same operand gives the same digits
        r2 = VecZnx(n, cols, a_size, a.data.copy())
        if res_size == a_size:
            po.glwe_mul_plain_assign(ref, off, r2, a_k, b, b_k, ab)
            assert np.array_equal(r2.data, res.data)


CONST_CASES = [
    (64, 1, 4, 3, 12, 12, 24),    # hi = 1, lo = 0
    (64, 2, 3, 5, 13, 13, 7),     # hi = 0, lo < 0
    (256, 1, 5, 4, 12, 16, 40),   # cross-base
]


@pytest.mark.parametrize("case", CONST_CASES)
def test_glwe_mul_const_oracle_vs_exact(refs, case):
    n, rank, a_size, res_size, ab, rb, off = case
    ref = refs(n)
    rng = seeded(7 * n + off)
    cols = rank + 1
    a = VecZnx(n, cols, a_size).fill_uniform(ab, rng)
    b = rng.integers(-(1 << (ab - 1)), 1 << (ab - 1), 3, dtype=np.int64)
    res = VecZnx(n, cols, res_size)
    po.glwe_mul_const(ref, off, res, rb, a, ab, b)
    hi, lo = po.offset_split(off, ab)
    for c in range(cols):
        _check_column(_big_const(a.data[:, c], b, hi, a_size + b.size - hi), ab, res.data[:, c], rb, lo)


def test_glwe_mul_const_assign_truncates_res_big(refs):
    """operations/glwe.rs:119: the assign form's res_big has res.size() limbs, so the product limbs beyond it are dropped, not carried - the
    digits differ from glwe_mul_const on the same operand."""
    n, cols, size, base2k, off = 64, 2, 4, 12, 12   # hi = 0, lo = 0: a.size + b.len - hi = 7 > 4 limbs of res_big
    ref = refs(n)
    rng = seeded(5)
    a = VecZnx(n, cols, size).fill_uniform(base2k, rng)
    b = rng.integers(-(1 << 11), 1 << 11, 3, dtype=np.int64)
    r_into = VecZnx(n, cols, size)
    po.glwe_mul_const(ref, off, r_into, base2k, a, base2k, b)
    r_asg = VecZnx(n, cols, size, a.data.copy())
    po.glwe_mul_const_assign(ref, off, r_asg, base2k, b)
    assert not np.array_equal(r_asg.data, r_into.data)
    hi, lo = po.offset_split(off, base2k)
    for c in range(cols):
        assert np.array_equal(normalize_exact(_big_const(a.data[:, c], b, hi, size), base2k, size), r_asg.data[:, c])
        assert np.array_equal(normalize_exact(_big_const(a.data[:, c], b, hi, size + b.size - hi), base2k, size), r_into.data[:, c])


def test_ckks_complex_constant_arms(refs):
    """mul.rs:342-415: im alone is X^{N/2} times the im product; re + im is their sum without renormalization; neither is zero."""
    n, cols, size, base2k, off = 64, 2, 3, 12, 24
    ref = refs(n)
    rng = seeded(11)
    a = VecZnx(n, cols, size).fill_uniform(base2k, rng)
    re = rng.integers(-(1 << 11), 1 << 11, 2, dtype=np.int64)
    im = rng.integers(-(1 << 11), 1 << 11, 2, dtype=np.int64)
    r_re, r_im, r_both, r_none = (VecZnx(n, cols, size) for _ in range(4))
    po.ckks_mul_pt_const_into(ref, off, r_re, base2k, a, base2k, re, None)
    po.ckks_mul_pt_const_into(ref, off, r_im, base2k, a, base2k, None, im)
    po.ckks_mul_pt_const_into(ref, off, r_both, base2k, a, base2k, re, im)
    r_none.data[...] = 3
    po.ckks_mul_pt_const_into(ref, off, r_none, base2k, a, base2k, None, None)
    assert not r_none.data.any()
    assert np.array_equal(r_both.data, r_re.data + r_im.data)
    plain_im = VecZnx(n, cols, size)
    po.glwe_mul_const(ref, off, plain_im, base2k, a, base2k, im)
    h = n // 2
    assert np.array_equal(r_im.data[..., h:], plain_im.data[..., :h])
    assert np.array_equal(r_im.data[..., :h], -plain_im.data[..., h:])


def test_library_exports_the_new_entry_points():
    from poulpy_amd.hal import load_library
    lib = load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_header_declares_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "poulpy_hip.h")) as f:
        h = f.read()
    for name in NEW_SYMBOLS + ("pz_glwe_mul_const_params", "PZ_MUL_PLAIN_ASSIGN", "PZ_MUL_CONST_ASSIGN"):
        assert name in h, name
    with open(os.path.join(ROOT, "include", "poulpy_hip.hpp")) as f:
        hpp = f.read()
    for name in ("glwe_mul_plain_batched", "glwe_mul_plain_workspace_bytes", "glwe_mul_const_batched"):
        assert name in hpp, name


def test_hal_binds_the_new_entry_points():
    from poulpy_amd import hal
    lib = hal.load_library()
    assert lib.pz_glwe_mul_plain_workspace_bytes.restype is C.c_size_t
    assert lib.pz_glwe_mul_plain_batched.argtypes is not None and lib.pz_glwe_mul_const_batched.argtypes is not None
    assert [f for f, _ in hal.GlweMulConstParams._fields_] == ["rank", "a_size", "a_base2k", "res_size", "res_base2k", "cnv_offset"]
    for m in ("glwe_mul_plain_batched", "glwe_mul_plain_workspace_bytes", "glwe_mul_const_batched"):
        assert callable(getattr(hal.Module, m)), m
