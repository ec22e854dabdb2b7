"""Secret-key toolkit in exact arithmetic (tests/ only): secrets, encryption, phase and noise, restated from poulpy-core.

It calls neither the oracle (oracle/fft64_ref.c) nor the device (poulpy_amd): every product a * s is an exact integer product in
Z[X]/(X^N+1) on the limbs of a, and every phase and noise is computed on integers, so a convention shared by the oracle and the device
(which key column multiplies which input column, phi_p against phi_p^-1, the limb of a GGLWE row's message) is checked against the
reference's own encryption procedures rather than against itself.

Layouts are those of poulpy_amd/layouts.py: a GLWE is a (size, rank + 1, n) int64 array (VecZnx, limb-major), a GGSW / GGLWE a
(rows, cols_in, size, cols_out, n) int64 array (MatZnx), which vmp_prepare takes as it is.
"""
from __future__ import annotations

import math

import numpy as np

# poulpy-core/src/encryption/mod.rs:76-80
SIGMA = 3.2
BOUND = 6.0 * SIGMA

# above this ring degree the products go through numpy.fft (checked to lie within 1/4 of an integer before rounding)
SCHOOLBOOK_MAX_N = 4096
# mul_small takes the same FFT route from this ring degree on where its digits allow (keys of many entries: a blind-rotation key)
FFT_MIN_N = 512
FFT_MAX_DIGIT = 1 << 24      # |result| <= N 2^24 <= 2^41 up to N = 2^17, far below 2^52


def limbs_for(k: int, base2k: int) -> int:
    return -(-k // base2k)


# ---- secrets (poulpy-core layouts/glwe_secret.rs fill_ternary_prob) ----
def ternary_secret(n: int, rank: int, rng: np.random.Generator, prob: float = 0.5) -> np.ndarray:
    """(rank, n) int64 in {-1, 0, 1}: non-zero with probability `prob`, then a uniform sign."""
    nz = rng.random((rank, n)) < prob
    sign = np.where(rng.random((rank, n)) < 0.5, -1, 1)
    return (nz * sign).astype(np.int64)


# ---- exact arithmetic in Z[X]/(X^N+1) ----
def rotate(a: np.ndarray, k: int) -> np.ndarray:
    """X^k * a (negacyclic), along the last axis."""
    n = a.shape[-1]
    k %= 2 * n
    sign = 1
    if k >= n:
        k -= n
        sign = -1
    r = np.roll(a, k, axis=-1)
    r[..., :k] *= -1
    return sign * r


def automorphism(a: np.ndarray, p: int) -> np.ndarray:
    """phi_p: X^i -> X^(i p mod 2N), the sign flipped past N (poulpy-cpu-ref/src/reference/znx/automorphism.rs:1-17), along the last
    axis; p odd, any sign."""
    n = a.shape[-1]
    idx = (np.arange(n, dtype=np.int64) * int(p)) % (2 * n)
    out = np.zeros_like(a)
    pos = idx < n
    out[..., idx[pos]] = a[..., pos]
    out[..., idx[~pos] - n] = -a[..., ~pos]
    return out


def galois_inv(p: int, n: int) -> int:
    return pow(int(p) % (2 * n), -1, 2 * n)


def mul_small(a: np.ndarray, s: np.ndarray) -> np.ndarray:
    """a * s in Z[X]/(X^N+1) along the last axis, exactly: a int64 digits (|a| < 2^24 on the FFT route), s a small secret polynomial
    (|s| <= 1)."""
    a = np.asarray(a, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    n = a.shape[-1]
    assert s.shape == (n,) and np.abs(s).max(initial=0) <= 1
    if n <= SCHOOLBOOK_MAX_N and (n < FFT_MIN_N or np.abs(a).max(initial=0) >= FFT_MAX_DIGIT):
        out = np.zeros_like(a)
        for k in np.flatnonzero(s):
            r = np.roll(a, int(k), axis=-1)
            r[..., :k] *= -1
            if s[k] > 0:
                out += r
            else:
                out -= r
        return out
    # negacyclic product by a twisted cyclic FFT, its rounding checked below
    assert np.abs(a).max(initial=0) < FFT_MAX_DIGIT and n <= (1 << 17)
    w = np.exp(1j * np.pi * np.arange(n) / n)
    c = np.fft.ifft(np.fft.fft(a * w, axis=-1) * np.fft.fft(s * w), axis=-1) / w
    r = np.rint(c.real)
    assert np.abs(c.real - r).max(initial=0) < 0.25 and np.abs(c.imag).max(initial=0) < 0.25
    return r.astype(np.int64)


def normalize(limbs: np.ndarray, base2k: int) -> np.ndarray:
    """Balanced base-2^base2k digits in [-2^(base2k-1), 2^(base2k-1)) of the limb vector (axis 0, limb 0 most significant); the carry
    out of limb 0 is dropped (the torus is mod 1)."""
    x = np.array(limbs, dtype=np.int64, copy=True)
    half, mask = 1 << (base2k - 1), (1 << base2k) - 1
    carry = np.zeros(x.shape[1:], dtype=np.int64)
    for j in reversed(range(x.shape[0])):
        v = x[j] + carry
        d = ((v + half) & mask) - half
        carry = (v - d) >> base2k
        x[j] = d
    return x


def to_int(limbs: np.ndarray, base2k: int) -> np.ndarray:
    """The integers sum_j limbs[j] 2^(base2k (size - 1 - j)) (Python ints, object array): the torus value times 2^(base2k size)."""
    acc = np.zeros(limbs.shape[1:], dtype=object)
    for j in range(limbs.shape[0]):
        acc = acc * (1 << base2k) + limbs[j].astype(object)
    return acc


def uniform_digits(shape, base2k: int, rng: np.random.Generator) -> np.ndarray:
    """vec_znx_fill_uniform: digits in [-2^(base2k-1), 2^(base2k-1))."""
    h = 1 << (base2k - 1)
    return rng.integers(-h, h, shape, dtype=np.int64)


def gaussian(n: int, rng: np.random.Generator, sigma: float = SIGMA, bound: float = BOUND) -> np.ndarray:
    e = np.rint(rng.normal(0.0, sigma, n))
    return np.clip(e, -bound, bound).astype(np.int64)


# ---- encryption (poulpy-core/src/encryption) ----
def glwe_encrypt(sk: np.ndarray, pt: np.ndarray, base2k: int, k: int, rng: np.random.Generator, col: int = 0,
                 sigma: float = SIGMA) -> np.ndarray:
    """glwe.rs:426-512 (glwe_encrypt_sk_internal): the mask columns uniform, the body -sum_i (c_i - [i = col] pt) s_i + e (+ pt if
    col = 0), e of deviation sigma at 2^-k; so the phase is pt + e (col 0) or pt s_col + e.  pt: (size, n) message limbs at base2k
    (fewer limbs are zero-extended).  Returns the (size, rank + 1, n) normalized ciphertext, size = ceil(k / base2k)."""
    rank, n = sk.shape
    size = limbs_for(k, base2k)
    m = np.zeros((size, n), dtype=np.int64)
    m[:min(size, pt.shape[0])] = pt[:size]
    ct = np.empty((size, rank + 1, n), dtype=np.int64)
    body = np.zeros((size, n), dtype=np.int64)
    for i in range(1, rank + 1):
        ci = uniform_digits((size, n), base2k, rng)
        ct[:, i] = ci
        body -= mul_small(ci - m if col == i else ci, sk[i - 1])
    body[size - 1] += gaussian(n, rng, sigma) << (base2k * size - k)
    if col == 0:
        body += m
    ct[:, 0] = normalize(body, base2k)
    return ct


def _row_plaintext(msg: np.ndarray, size: int, limb: int, base2k: int) -> np.ndarray:
    assert 0 <= limb < size
    pt = np.zeros((size, msg.shape[-1]), dtype=np.int64)
    pt[limb] = msg
    return normalize(pt, base2k)


def ggsw_encrypt(sk: np.ndarray, msg: np.ndarray, base2k: int, k: int, dnum: int, dsize: int, rng: np.random.Generator,
                 limb_shift: int = 0) -> np.ndarray:
    """ggsw.rs:92-118: row i carries msg in limb (dsize - 1) + i dsize, column j encrypts it against column j (msg s_j for j >= 1).
    limb_shift moves every row's message (a negative control).  (dnum, rank + 1, size, rank + 1, n)."""
    rank, n = sk.shape
    size = limbs_for(k, base2k)
    assert dnum * dsize <= size   # ggsw.rs / gglwe.rs: dnum dsize base2k <= max_k
    out = np.zeros((dnum, rank + 1, size, rank + 1, n), dtype=np.int64)
    for row in range(dnum):
        pt = _row_plaintext(msg, size, (dsize - 1) + row * dsize + limb_shift, base2k)
        for c in range(rank + 1):
            out[row, c] = glwe_encrypt(sk, pt, base2k, k, rng, col=c)
    return out


def gglwe_encrypt(sk_out: np.ndarray, msgs: np.ndarray, base2k: int, k: int, dnum: int, dsize: int, rng: np.random.Generator,
                  limb_shift: int = 0) -> np.ndarray:
    """gglwe.rs:114-147: input column i, row r is a GLWE under sk_out of msgs[i] in limb (dsize - 1) + r dsize (:131-135).
    (dnum, rank_in, size, rank_out + 1, n)."""
    rank_in = msgs.shape[0]
    rank_out, n = sk_out.shape
    size = limbs_for(k, base2k)
    assert dnum * dsize <= size
    out = np.zeros((dnum, rank_in, size, rank_out + 1, n), dtype=np.int64)
    for c in range(rank_in):
        for row in range(dnum):
            pt = _row_plaintext(msgs[c], size, (dsize - 1) + row * dsize + limb_shift, base2k)
            out[row, c] = glwe_encrypt(sk_out, pt, base2k, k, rng, col=0)
    return out


def switching_key(sk_in: np.ndarray, sk_out: np.ndarray, base2k: int, k: int, dnum: int, dsize: int, rng, **kw) -> np.ndarray:
    """glwe_switching_key.rs:58-105: the GGLWE of sk_in under sk_out."""
    return gglwe_encrypt(sk_out, sk_in, base2k, k, dnum, dsize, rng, **kw)


def automorphism_key(sk: np.ndarray, p: int, base2k: int, k: int, dnum: int, dsize: int, rng, encrypt_for: int | None = None) -> np.ndarray:
    """glwe_automorphism_key.rs:88-108: the GGLWE of sk under phi_{p^-1}(sk) (:94-96).  encrypt_for replaces p^-1 (a negative
    control: p itself)."""
    n = sk.shape[1]
    g = galois_inv(p, n) if encrypt_for is None else encrypt_for
    return gglwe_encrypt(automorphism(sk, g), sk, base2k, k, dnum, dsize, rng)


# ---- phase and noise (poulpy-core decryption/glwe.rs, noise/glwe.rs:28-46, poulpy-hal layouts/stats.rs:27-57) ----
def glwe_phase(ct: np.ndarray, sk: np.ndarray) -> np.ndarray:
    """c_0 + sum_i c_i s_i per limb (un-normalized, exact): (size, n)."""
    body = np.array(ct[:, 0], dtype=np.int64, copy=True)
    for i in range(1, ct.shape[1]):
        body += mul_small(ct[:, i], sk[i - 1])
    return body


def torus_diff(a: np.ndarray, a_base2k: int, b: np.ndarray, b_base2k: int) -> np.ndarray:
    """a - b as centred torus values in [-1/2, 1/2), computed on integers at the finer of the two precisions and converted to
    float64 only at the end (a difference near 2^-80 of values of order 1 keeps its digits)."""
    ka, kb = a_base2k * a.shape[0], b_base2k * b.shape[0]
    kk = max(ka, kb)
    d = (to_int(a, a_base2k) << (kk - ka)) - (to_int(b, b_base2k) << (kk - kb))
    q = 1 << kk
    d = (d + q // 2) % q - q // 2
    return np.ldexp(np.array([float(x) for x in d.reshape(-1)], dtype=np.float64), -kk).reshape(d.shape)


def noise_log2(ct: np.ndarray, ct_base2k: int, sk: np.ndarray, pt_want: np.ndarray, pt_base2k: int) -> float:
    """log2 of the standard deviation over the coefficients of phase(ct) - pt_want (glwe_noise(...).std().log2())."""
    e = torus_diff(glwe_phase(ct, sk), ct_base2k, pt_want, pt_base2k)
    sd = float(np.std(e))
    return math.log2(sd) if sd > 0 else -math.inf


# ---- closed-form noise bounds (poulpy-core/src/noise/mod.rs) ----
def var_noise_gglwe_product_v2(n, k_ksk, dnum, dsize, base2k, var_xs, var_msg, var_a_err, var_gct_err_lhs, var_gct_err_rhs, rank_in):
    """noise/mod.rs:50-72"""
    var_base = (2.0 ** (dsize * base2k)) ** 2 / 12.0
    scale = 2.0 ** k_ksk
    noise = dnum * n * var_base * (var_gct_err_lhs + var_xs * var_gct_err_rhs)
    noise += var_msg * var_a_err * var_base * n
    noise *= rank_in
    return noise / (scale * scale)


def noise_ggsw_product(n, base2k, var_xs, var_msg, var_a0_err, var_a1_err, var_gct_err_lhs, var_gct_err_rhs, rank, k_in, k_ggsw):
    """noise/mod.rs:106-136"""
    a_logq = min(k_in, k_ggsw)
    a_cols = -(-a_logq // base2k)
    b_scale = 2.0 ** k_ggsw
    a_scale = 2.0 ** (k_ggsw - a_logq)
    var_base = (2.0 ** base2k) ** 2 / 12.0
    noise = (rank + 1.0) * a_cols * n * var_base * (var_gct_err_lhs + var_xs * var_gct_err_rhs)
    noise += var_msg * var_a0_err * a_scale * a_scale * n
    noise += var_msg * var_a1_err * a_scale * a_scale * n * var_xs * rank
    return min(math.log2(math.sqrt(noise) / b_scale), -1.0)


def keyswitch_bound(n, k_ksk, dnum, dsize, key_base2k, rank_in) -> float:
    """The bound of keyswitch/glwe_ct.rs:132-147 and automorphism/glwe_ct.rs:126-150 (with the dsize each test passes)."""
    v = var_noise_gglwe_product_v2(n, k_ksk, dnum, dsize, key_base2k, 0.5, 0.5, 0.0, SIGMA * SIGMA, 0.0, rank_in)
    return math.log2(math.sqrt(v)) + 1.0


def external_product_bound(n, base2k, rank, k_in, k_ggsw) -> float:
    """The bound of external_product/glwe_ct.rs:133-152 (message X^k, var_msg = 1/n); base2k = key_base2k * max_dsize there."""
    return noise_ggsw_product(n, base2k, 0.5, 1.0 / n, SIGMA * SIGMA, 1.0 / 12.0, SIGMA * SIGMA, 0.0, rank, k_in, k_ggsw) + 1.0


def var_noise_gglwe_product(n, base2k, var_xs, var_msg, var_a_err, var_gct_err_lhs, var_gct_err_rhs, rank_in, a_logq, b_logq):
    """noise/mod.rs:18-46 (the form trace.rs:133-147 calls)"""
    a_logq = min(a_logq, b_logq)
    a_cols = -(-a_logq // base2k)
    b_scale = 2.0 ** b_logq
    a_scale = 2.0 ** (b_logq - a_logq)
    var_base = (2.0 ** base2k) ** 2 / 12.0
    noise = a_cols * n * var_base * (var_gct_err_lhs + var_xs * var_gct_err_rhs)
    noise += var_msg * var_a_err * a_scale * a_scale * n
    noise *= rank_in
    return noise / (b_scale * b_scale)


# ---- messages and their exact products ----
def encode(data: np.ndarray, base2k: int, k_pt: int, size: int) -> np.ndarray:
    """encode_vec_i64 (poulpy-hal/src/layouts/encoding.rs:17-57): data 2^-k_pt as (size, n) normalized limbs at base2k; the data sit in
    limb ceil(k_pt / base2k) - 1, shifted up by the bits that limb has below 2^-k_pt."""
    data = np.asarray(data, dtype=np.int64)
    used = limbs_for(k_pt, base2k)
    assert used <= size
    pt = np.zeros((size, data.shape[-1]), dtype=np.int64)
    pt[used - 1] = data << (used * base2k - k_pt)
    return normalize(pt, base2k)


def mul_exact(a, b_int: np.ndarray) -> np.ndarray:
    """The schoolbook negacyclic product on Python ints: a any integers ((n,) object array or int64), b int64; (n,) object array."""
    ao = np.asarray(a).astype(object)
    b = np.asarray(b_int, dtype=np.int64)
    n = ao.shape[-1]
    assert ao.shape == (n,) and b.shape == (n,) and n <= SCHOOLBOOK_MAX_N
    out = np.zeros(n, dtype=object)
    for k in np.flatnonzero(b):
        r = np.roll(ao, int(k))
        r[:k] *= -1
        out += r * int(b[k])
    return out


def mul_msg(a_int: np.ndarray, b_int: np.ndarray) -> np.ndarray:
    """The exact negacyclic product of two small integer message polynomials, (n,) x (n,) -> (n,) int64."""
    a = np.asarray(a_int, dtype=np.int64)
    b = np.asarray(b_int, dtype=np.int64)
    n = a.shape[-1]
    assert a.shape == (n,) and b.shape == (n,)
    if n <= SCHOOLBOOK_MAX_N:
        return mul_exact(a, b).astype(np.int64)
    assert n * int(np.abs(a).max(initial=0)) * int(np.abs(b).max(initial=0)) < (1 << 50)
    w = np.exp(1j * np.pi * np.arange(n) / n)
    c = np.fft.ifft(np.fft.fft(a * w) * np.fft.fft(b * w)) / w
    r = np.rint(c.real)
    assert np.abs(c.real - r).max(initial=0) < 0.25 and np.abs(c.imag).max(initial=0) < 0.25
    return r.astype(np.int64)


def torus_from_int(values: np.ndarray, bits: int, base2k: int = 16) -> np.ndarray:
    """values 2^-bits mod 1 as ((size, n), base2k) normalized limbs covering at least `bits` bits (bits <= 0: an integer, the zero
    torus element), for torus_diff."""
    v = np.asarray(values).astype(object)
    if bits <= 0:
        return np.zeros((1, v.shape[-1]), dtype=np.int64)
    size = limbs_for(bits, base2k)
    q = 1 << bits
    v = (v % q) << (size * base2k - bits)
    pt = np.zeros((size, v.shape[-1]), dtype=np.int64)
    mask = (1 << base2k) - 1
    for j in reversed(range(size)):
        pt[j] = (v & mask).astype(np.int64)
        v = v >> base2k
    return normalize(pt, base2k)


# ---- the tensor product of two GLWE (poulpy-core layouts/glwe_secret_tensor.rs, encryption/glwe_tensor_key.rs, decryption/glwe_tensor.rs) ----
def pair_index(i: int, j: int, rank: int) -> int:
    """glwe_secret_tensor.rs:204: the column of s_i s_j, i <= j."""
    assert 0 <= i <= j < rank
    return i * rank + j - i * (i + 1) // 2


def secret_tensor(sk: np.ndarray) -> np.ndarray:
    """glwe_secret_tensor.rs:200-218: (pairs, n) exact integers s_i s_j, i <= j, in the reference's order (s0^2, s0 s1, s1^2 at rank 2).
    The coefficients reach N in magnitude; they stay plain integers."""
    rank, n = sk.shape
    out = np.zeros((rank * (rank + 1) // 2, n), dtype=np.int64)
    for i in range(rank):
        for j in range(i, rank):
            out[pair_index(i, j, rank)] = mul_small(sk[i], sk[j])
    return out


def tensor_key(sk: np.ndarray, base2k: int, k: int, dnum: int, dsize: int, rng, order=None, limb_shift: int = 0) -> np.ndarray:
    """encryption/glwe_tensor_key.rs:92-96: the GGLWE of secret_tensor(sk) under sk, (dnum, pairs, size, rank + 1, n).  order permutes
    the pair columns and limb_shift moves every row's message (negative controls)."""
    msgs = secret_tensor(sk)
    if order is not None:
        msgs = msgs[list(order)]
    return gglwe_encrypt(sk, msgs, base2k, k, dnum, dsize, rng, limb_shift=limb_shift)


def glwe_tensor_phase(ct: np.ndarray, sk: np.ndarray, base2k: int, reverse_pairs: bool = False) -> np.ndarray:
    """decryption/glwe_tensor.rs:54-66: c_0 + sum_i c_i s_i + sum_{i<=j} c_ij s_i s_j over the columns [0, 1..rank, pairs] of a
    (size, (rank + 1)(rank + 2) / 2, n) tensor at base2k, per limb (un-normalized): (size, n).  c_ij s_i is normalized at base2k
    before it meets s_j (the torus is mod 1: the carry dropped off the top is an integer), which keeps mul_small's digits small.
    reverse_pairs reads the pair columns in reversed order (s1^2 for s0^2 at rank 2: a negative control of this checker)."""
    rank, n = sk.shape
    assert ct.shape[1] == (rank + 1) * (rank + 2) // 2
    body = glwe_phase(ct[:, :rank + 1], sk)
    for i in range(rank):
        for j in range(i, rank):
            col = pair_index(i, j, rank)
            if reverse_pairs:
                col = rank * (rank + 1) // 2 - 1 - col
            body += mul_small(normalize(mul_small(ct[:, rank + 1 + col], sk[i]), base2k), sk[j])
    return body


# ---- LWE: secrets, encryption, phase (poulpy-core layouts/lwe_secret.rs, encryption/lwe.rs, decryption/lwe.rs) ----
# an LWE is a (size, n_lwe + 1) int64 array, limb i = [b, a_0 .. a_{n_lwe - 1}]: the body at index 0, the mask behind it
def ternary_lwe_secret(n_lwe: int, rng: np.random.Generator, prob: float = 0.5) -> np.ndarray:
    """lwe_secret.rs:61-64: (n_lwe,) in {-1, 0, 1}."""
    return ternary_secret(n_lwe, 1, rng, prob)[0]


def binary_block_secret(n_lwe: int, block_size: int, rng: np.random.Generator) -> np.ndarray:
    """lwe_secret.rs:81 / scalar_znx.rs:154-166: every block of block_size coefficients holds at most one 1, at an index drawn uniformly
    from 0 .. block_size (block_size itself: none)."""
    assert n_lwe % block_size == 0
    s = np.zeros(n_lwe, dtype=np.int64)
    for blk in range(0, n_lwe, block_size):
        idx = int(rng.integers(0, block_size + 1))
        if idx != block_size:
            s[blk + idx] = 1
    return s


def encode_int(value: int, base2k: int, k: int, size: int | None = None) -> np.ndarray:
    """encode_coeff_i64 (encoding.rs:116-155) of one integer: value 2^-k as (size, 1) normalized limbs."""
    return encode(np.array([int(value)], dtype=np.int64), base2k, k, limbs_for(k, base2k) if size is None else size)


def _div_round(a: int, b: int) -> int:
    """encoding.rs:311-320: round half away from zero."""
    q, r = abs(a) // b, abs(a) % b
    q += 2 * r >= b
    return q if a >= 0 else -q


def decode_coeff(limbs: np.ndarray, base2k: int, k: int, idx: int = 0) -> int:
    """decode_coeff_i64 (encoding.rs:240-263): the integer that coefficient idx of the (size, n) limbs holds at 2^-k; the last limb used
    is rounded to the bits it has above 2^-k."""
    size = limbs_for(k, base2k)
    rem = base2k - (k % base2k)
    res = 0
    for j in range(size):
        x = int(limbs[j][idx])
        if j == size - 1 and rem != base2k:
            res = (res << ((base2k - rem) % base2k)) + _div_round(x, 1 << rem)
        else:
            res = (res << base2k) + x
    return res


def lwe_encrypt(sk: np.ndarray, value_limbs: np.ndarray, base2k: int, k: int, rng: np.random.Generator, sigma: float = SIGMA) -> np.ndarray:
    """encryption/lwe.rs:88-120: the mask uniform, b = pt - <a, s> + e limb by limb (limbs the plaintext lacks: -<a, s>), e of deviation
    sigma at 2^-k, the body normalized.  value_limbs: (size_pt,) or (size_pt, 1) at base2k.  (size, n_lwe + 1), size = ceil(k / base2k)."""
    n_lwe = sk.shape[0]
    size = limbs_for(k, base2k)
    pt = np.asarray(value_limbs, dtype=np.int64).reshape(-1)
    ct = np.empty((size, n_lwe + 1), dtype=np.int64)
    ct[:, 1:] = uniform_digits((size, n_lwe), base2k, rng)
    body = -(ct[:, 1:] @ sk.astype(np.int64))
    m = min(size, pt.shape[0])
    body[:m] += pt[:m]
    body[size - 1] += int(gaussian(1, rng, sigma)[0]) << (base2k * size - k)
    ct[:, 0] = normalize(body[:, None], base2k)[:, 0]
    return ct


def lwe_phase(ct: np.ndarray, sk: np.ndarray) -> np.ndarray:
    """decryption/lwe.rs: b + <a, s> per limb (un-normalized, exact), as (size, 1) limbs."""
    return (ct[:, 0] + ct[:, 1:] @ sk.astype(np.int64))[:, None]


def lwe_decrypt(ct: np.ndarray, sk: np.ndarray, base2k: int) -> np.ndarray:
    """The normalized phase, (size, 1)."""
    return normalize(lwe_phase(ct, sk), base2k)


def lwe_error(ct: np.ndarray, ct_base2k: int, sk: np.ndarray, pt_want: np.ndarray, pt_base2k: int) -> float:
    """phase(ct) - pt_want as a centred torus value."""
    return float(torus_diff(lwe_phase(ct, sk), ct_base2k, np.asarray(pt_want).reshape(-1, 1), pt_base2k)[0])


def rms_log2(errors) -> float:
    """log2 of the root mean square of a few error samples (an LWE has one coefficient: the deviation is taken over the batch, about zero)."""
    e = np.asarray(list(errors), dtype=np.float64)
    r = float(np.sqrt(np.mean(e * e)))
    return math.log2(r) if r > 0 else -math.inf


def lwe_noise_log2(cts, ct_base2k: int, sk: np.ndarray, pts_want, pt_base2k: int) -> float:
    return rms_log2(lwe_error(ct, ct_base2k, sk, pt, pt_base2k) for ct, pt in zip(cts, pts_want))


def rebase(limbs: np.ndarray, from_base2k: int, to_base2k: int, size: int) -> np.ndarray:
    """The torus value of (size_a, n) limbs at from_base2k as `size` normalized limbs at to_base2k (vec_znx_normalize across bases, offset
    0), for values the target holds exactly: dropped bits must be zero."""
    ka, kr = from_base2k * limbs.shape[0], to_base2k * size
    v = to_int(normalize(limbs, from_base2k), from_base2k)
    if kr >= ka:
        v = v * (1 << (kr - ka))
    else:
        assert all(int(x) % (1 << (ka - kr)) == 0 for x in v.reshape(-1)), "rebase would round"
        v = v // (1 << (ka - kr))
    return torus_from_int(v, kr, to_base2k)


def lwe_as_glwe_secret(sk_lwe: np.ndarray, n: int, embed: bool = True) -> np.ndarray:
    """phi_{-1}(s_lwe || 0) as a rank-1 GLWE secret, (1, n) (lwe_switching_key.rs:101-107): the constant coefficient of a(X) phi_{-1}(s)(X)
    is <a, s>.  embed=False leaves phi_{-1} out (a negative control)."""
    s = np.zeros((1, n), dtype=np.int64)
    s[0, :sk_lwe.shape[0]] = sk_lwe
    return automorphism(s, -1) if embed else s


def lwe_switching_key(sk_lwe_in, sk_lwe_out, n, base2k, k, dnum, rng, dsize: int = 1) -> np.ndarray:
    """lwe_switching_key.rs:95-109: the rank-1 GLWE switching key between the two embedded secrets."""
    return switching_key(lwe_as_glwe_secret(sk_lwe_in, n), lwe_as_glwe_secret(sk_lwe_out, n), base2k, k, dnum, dsize, rng)


def lwe_to_glwe_key(sk_lwe, sk_glwe, base2k, k, dnum, rng, dsize: int = 1, embed: bool = True) -> np.ndarray:
    """lwe_to_glwe_key.rs:92-99: the GGLWE of the embedded LWE secret under sk_glwe."""
    return gglwe_encrypt(sk_glwe, lwe_as_glwe_secret(sk_lwe, sk_glwe.shape[1], embed), base2k, k, dnum, dsize, rng)


def glwe_to_lwe_key(sk_lwe, sk_glwe, base2k, k, dnum, rng, dsize: int = 1, embed: bool = True) -> np.ndarray:
    """glwe_to_lwe_key.rs:88-107: the GGLWE of sk_glwe under the embedded LWE secret (rank_in = rank of sk_glwe, rank_out = 1)."""
    return gglwe_encrypt(lwe_as_glwe_secret(sk_lwe, sk_glwe.shape[1], embed), sk_glwe, base2k, k, dnum, dsize, rng)


# ---- blind rotation (poulpy-bin-fhe blind_rotation: algorithms/cggi/key.rs, lut.rs, algorithms/mod.rs) ----
def blind_rotation_key(sk_glwe, sk_lwe, base2k, k, dnum, rng, dsize: int = 1) -> np.ndarray:
    """cggi/key.rs:53-59: entry i is the GGSW under sk_glwe of the constant polynomial s_lwe[i].  (n_lwe, dnum, rank + 1, size, rank + 1, n)."""
    n = sk_glwe.shape[1]
    keys = []
    for bit in sk_lwe:
        msg = np.zeros(n, dtype=np.int64)
        msg[0] = int(bit)
        keys.append(ggsw_encrypt(sk_glwe, msg, base2k, k, dnum, dsize, rng))
    return np.stack(keys)


def lut_rotate(data: np.ndarray, k: int) -> np.ndarray:
    """lut.rs:342-363: X^k on a table of ext polynomials, data (ext, size, n), in Z[X]/(X^(n ext) + 1) where polynomial i holds the
    coefficients i, i + ext, ...: the first ext - k_lo polynomials turn by k_hi, the others by k_hi + 1, then the list turns by k_lo."""
    ext, _, n = data.shape
    two_n_ext = 2 * n * ext
    k_pos = int(k) % two_n_ext
    k_hi, k_lo = k_pos // ext, k_pos % ext
    out = [rotate(data[i], k_hi if i < ext - k_lo else k_hi + 1) for i in range(ext)]
    return np.stack(out[ext - k_lo:] + out[:ext - k_lo])


def lut_set(f, k: int, n: int, ext: int, base2k: int, lut_k: int, with_drift: bool = True):
    """lut.rs:271-340: the table of f (at most n values) at k message bits: value f[i] 2^-k on the step coefficients [i step, (i + 1) step)
    of the domain n ext, step = round(domain / len(f)); polynomial j takes the coefficients j, j + ext, ...; every polynomial normalized;
    the whole turned by -drift, drift = step / 2, so that a phase within half a step of i step reads f[i].  with_drift=False leaves that
    turn out (a negative control).  Returns (data (ext, size, n), drift)."""
    f = [int(x) for x in f]
    assert len(f) <= n and ext > 0 and ext & (ext - 1) == 0
    limbs = limbs_for(k, base2k)
    size = limbs_for(lut_k, base2k)
    assert limbs <= size
    scale = 1 << (base2k - k % base2k) if k % base2k else 1
    domain = n * ext
    step = (domain + len(f) // 2) // len(f)
    full = np.zeros((size, domain), dtype=np.int64)
    for i, fi in enumerate(f):
        full[limbs - 1, i * step:(i + 1) * step] = fi * scale
    data = np.stack([normalize(full[:, j::ext], base2k) for j in range(ext)])
    drift = step >> 1
    return (lut_rotate(data, -drift) if with_drift else data), drift


def mod_switch_2n(n2: int, lwe: np.ndarray, base2k: int, negate: bool) -> np.ndarray:
    """algorithms/mod.rs:136-176 on exact integers: the (size, n_lwe + 1) LWE to n_lwe + 1 exponents at n2 = 2 N ext; negate (direction
    Left) flips every sign first.  One limb wider than log2n: rounded to its top bits; else limbs are concatenated (the last one partly)."""
    log2n = (n2 - 1).bit_length() + 1
    res = [-int(x) if negate else int(x) for x in lwe[0]]
    if base2k > log2n:
        diff = base2k - (log2n - 1)
        return np.array([(x + (1 << (diff - 1))) >> diff for x in res], dtype=np.int64)
    rem = base2k - (log2n % base2k)
    size = limbs_for(log2n, base2k)
    for i in range(1, size):
        if i == size - 1 and rem != base2k:
            res = [(y << (base2k - rem)) + (int(x) >> rem) for x, y in zip(lwe[i], res)]
        else:
            res = [(y << base2k) + int(x) for x, y in zip(lwe[i], res)]
    return np.array(res, dtype=np.int64)
