"""Oracle compositions and case builders for the key-level forms of key switching (tests/ only): glwe_automorphism_key_automorphism
(poulpy-core automorphism/gglwe_atk.rs:42-155), ggsw_keyswitch (keyswitching/ggsw.rs:37-85) and ggsw_automorphism
(automorphism/ggsw_ct.rs:32-82).  Every expectation is a loop over entries of the oracle's existing methods, as the reference loops:
vec_znx_automorphism per column -> glwe_keyswitch -> vec_znx_automorphism_assign for the key composition, glwe_keyswitch /
glwe_automorphism on the entries (row, 0) -> ggsw_expand_row for the GGSW forms.  Arrays are MatZnx data, (rows, cols_in, size, cols_out, n)."""
from __future__ import annotations

import math

import numpy as np

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import fhe_sk as fs


def prepare(mod, key):
    rows, cols_in, size, cols_out, n = key.shape
    pm = mod.vmp_pmat_alloc(rows, cols_in, cols_out, size)
    mod.vmp_prepare(pm, MatZnx(n, rows, cols_in, cols_out, size, np.ascontiguousarray(key)))
    return pm


def _vec(entry):
    size, cols, n = entry.shape
    return VecZnx(n, cols, size, np.ascontiguousarray(entry))


# ---- oracle compositions ----
def key_composition(ref, a, base2k, a_gal, pm, dsize, key_base2k, res_dnum, res_size):
    """gglwe_atk.rs:77-107 on one GGLWE `a` of Galois element a_gal: entry (row < res_dnum, col) of the result."""
    rows, cols_in, a_size, cols, n = a.shape
    assert res_dnum <= rows
    g = fs.galois_inv(a_gal, n)
    out = np.empty((res_dnum, cols_in, res_size, cols, n), dtype=np.int64)
    for row in range(res_dnum):
        for col in range(cols_in):
            src, tmp, res = _vec(a[row, col]), VecZnx(n, cols, a_size), VecZnx(n, cols, res_size)
            for i in range(cols):
                ref.vec_znx_automorphism(int(a_gal), tmp, i, src, i)
            ref.glwe_keyswitch(res, base2k, tmp, base2k, pm, dsize, key_base2k)
            for i in range(cols):
                ref.vec_znx_automorphism_assign(g, res, i)
            out[row, col] = res.data
    return out


def ggsw_keyswitch(ref, a, a_base2k, pm, dsize, key_base2k, tsk_pms, res_size, rank_out=None):
    """keyswitching/ggsw.rs:52-54 + ggsw_expand_row on one GGSW `a`."""
    rows, cols_a, a_size, _, n = a.shape
    cols = cols_a if rank_out is None else rank_out + 1
    out = MatZnx(n, rows, cols, cols, res_size)
    for row in range(rows):
        res = VecZnx(n, cols, res_size)
        ref.glwe_keyswitch(res, a_base2k, _vec(a[row, 0]), a_base2k, pm, dsize, key_base2k)
        out.data[row, 0] = res.data
    ref.ggsw_expand_row(out, a_base2k, tsk_pms, dsize, key_base2k)
    return out.data


def ggsw_automorphism(ref, a, a_base2k, pm, dsize, key_base2k, gal, tsk_pms, res_dnum, res_size):
    """automorphism/ggsw_ct.rs:54-56 + ggsw_expand_row on one GGSW `a`, rows < res_dnum."""
    rows, cols, a_size, _, n = a.shape
    assert res_dnum <= rows
    out = MatZnx(n, res_dnum, cols, cols, res_size)
    for row in range(res_dnum):
        res = VecZnx(n, cols, res_size)
        ref.glwe_automorphism(res, a_base2k, _vec(a[row, 0]), a_base2k, pm, dsize, key_base2k, int(gal) % (2 * n), "automorphism")
        out.data[row, 0] = res.data
    ref.ggsw_expand_row(out, a_base2k, tsk_pms, dsize, key_base2k)
    return out.data


# ---- the identity behind the fast form, on exact integers ----
def normalize_big(big, base2k):
    """Balanced digits of the limb vector `big` (limbs on axis 0, Python ints), the carry out of limb 0 dropped."""
    x = np.array(big, dtype=object, copy=True)
    half, mod = 1 << (base2k - 1), 1 << base2k
    carry = np.zeros(x.shape[1:], dtype=object)
    for j in reversed(range(x.shape[0])):
        v = x[j] + carry
        d = (v + half) % mod - half
        carry = (v - d) // mod
        x[j] = d
    return x


def galois_signs(n, p):
    """s(i) = -1 where phi_p gives source index i a minus sign: i p mod 2N >= N."""
    idx = (np.arange(n, dtype=np.int64) * (int(p) % (2 * n))) % (2 * n)
    return np.where(idx >= n, -1, 1).astype(object)


def has_tie_sign(out, base2k):
    """A digit +2^(base2k-1) in a result: normalize never writes it, so it is -normalize(-x) on a carry tie - a coefficient where the
    sign rule around the carry chain decides the digits."""
    return bool((out == (1 << (base2k - 1))).any())


# ---- semantics: the reference's encrypt / compose / measure procedure ----
def composition_bound(n, k_ksk, dnum_ksk, dsize, key_base2k, rank):
    """test_suite/automorphism/gglwe_atk.rs:155-170"""
    v = fs.var_noise_gglwe_product_v2(n, k_ksk, dnum_ksk, dsize, key_base2k, 0.5, 0.5, 0.0, fs.SIGMA * fs.SIGMA, 0.0, rank)
    return math.log2(math.sqrt(v)) + 0.5


def composition_case(n, base2k, rank, dsize, seed, p0=-1, p1=-5):
    """The parameters and keys of test_suite/automorphism/gglwe_atk.rs:36-125: the input key (Galois element p0) in base2k - 1, the
    applied key (p1) in base2k."""
    from tests.helpers import seeded
    from types import SimpleNamespace
    rng = seeded(seed)
    in_b, key_b = base2k - 1, base2k
    k_in = 4 * in_b + 1
    k_ksk = k_in + key_b * dsize
    dnum_in, dnum_ksk = k_in // in_b, -(-k_in // (key_b * dsize))
    sk = fs.ternary_secret(n, rank, rng)
    key_in = fs.automorphism_key(sk, p0, in_b, k_in, dnum_in, 1, rng)
    key_apply = fs.automorphism_key(sk, p1, key_b, k_ksk, dnum_ksk, dsize, rng)
    return SimpleNamespace(n=n, rank=rank, dsize=dsize, in_b=in_b, key_b=key_b, k_in=k_in, k_ksk=k_ksk, dnum_in=dnum_in, dnum_ksk=dnum_ksk,
                           sk=sk, p0=p0, p1=p1, key_in=key_in, key_apply=key_apply, res_size=fs.limbs_for(k_ksk, in_b),
                           bound=composition_bound(n, k_ksk, dnum_ksk, dsize, key_b, rank), rng=rng)


def composition_noise(c, out):
    """Noise of every entry of the derived key under phi_{(p0 p1)^-1}(sk), against the plaintext of its row (GGLWE::noise)."""
    sk_auto = fs.automorphism(c.sk, fs.galois_inv(c.p0 * c.p1, c.n))
    have = []
    for row in range(out.shape[0]):
        for col in range(out.shape[1]):
            pt = fs._row_plaintext(c.sk[col], c.res_size, row, c.in_b)
            have.append(fs.noise_log2(out[row, col], c.in_b, sk_auto, pt, c.in_b))
    return have


def derived_key_bound(c):
    """A glwe_automorphism by the DERIVED key: the key-switch bound (keyswitch/glwe_ct.rs:132-147) with the key's error variance
    replaced by the square of the reference's own bound on the derived key's noise (composition_bound, a torus value: times 2^k)."""
    k = c.res_size * c.in_b
    err = 2.0 ** (c.bound + k)
    v = fs.var_noise_gglwe_product_v2(c.n, k, c.dnum_in, 1, c.in_b, 0.5, 0.5, 0.0, err * err, 0.0, c.rank)
    return math.log2(math.sqrt(v)) + 1.0


# ---- GGSW forms: test_suite/keyswitch/ggsw_ct.rs:35-190 and test_suite/automorphism/ggsw_ct.rs:34-180 ----
def var_noise_gglwe_product(n, base2k, var_xs, var_msg, var_a_err, var_gct_err_lhs, var_gct_err_rhs, rank_in, a_logq, b_logq):
    """noise/mod.rs:18-47"""
    a_logq = min(a_logq, b_logq)
    a_cols = -(-a_logq // base2k)
    b_scale, a_scale = 2.0 ** b_logq, 2.0 ** (b_logq - a_logq)
    var_base = (2.0 ** base2k) ** 2 / 12.0
    noise = a_cols * n * var_base * (var_gct_err_lhs + var_xs * var_gct_err_rhs)
    noise += var_msg * var_a_err * a_scale * a_scale * n
    return noise * rank_in / (b_scale * b_scale)


def noise_ggsw_keyswitch(n, base2k, col, var_xs, var_a_err, var_gct_err_lhs, var_gct_err_rhs, rank, k_ct, k_ksk, k_tsk):
    """noise/mod.rs:140-188"""
    noise = var_noise_gglwe_product(n, base2k, var_xs, var_xs, var_a_err, var_gct_err_lhs, var_gct_err_rhs, rank, k_ct, k_ksk)
    if col > 0:
        noise += var_noise_gglwe_product(n, base2k, var_xs, n * var_xs * var_xs, var_a_err + 1.0 / 12.0, var_gct_err_lhs, var_gct_err_rhs,
                                         rank, k_ct, k_tsk)
        noise += n * noise * var_xs * 0.5
    return min(math.log2(math.sqrt(noise)), -1.0)


def tensor_key(sk, base2k, k, dnum, dsize, rng):
    """encryption/gglwe_to_ggsw_key.rs:60-108: key i is the GGLWE under sk of the products s_i s_j, j < rank."""
    rank = sk.shape[0]
    return [fs.gglwe_encrypt(sk, np.stack([fs.mul_small(sk[i], sk[j]) for j in range(rank)]), base2k, k, dnum, dsize, rng)
            for i in range(rank)]


def ggsw_case(op, n, base2k, rank, dsize, seed, p=-5, control=False):
    """op "ks": a GGSW of a message with every coefficient +-1 under sk_in, the switching key sk_in -> sk_out and sk_out's tensor key;
    op "auto": one secret, the automorphism key of p.  control: the key-switching key's messages one limb off / the automorphism key
    for p instead of p^-1."""
    from tests.helpers import seeded
    from types import SimpleNamespace
    rng = seeded(seed)
    in_b, key_b = base2k - 1, base2k
    k_in = 4 * in_b + 1
    k_ksk = k_in + key_b * dsize
    dnum_in, dnum_ksk = k_in // in_b, -(-k_in // (key_b * dsize))
    sk_in = fs.ternary_secret(n, rank, rng)
    if op == "ks":
        sk_out = fs.ternary_secret(n, rank, rng)
        key = fs.switching_key(sk_in, sk_out, key_b, k_ksk, dnum_ksk, dsize, rng, limb_shift=1 if control else 0)
    else:
        sk_out = sk_in
        key = fs.automorphism_key(sk_in, p, key_b, k_ksk, dnum_ksk, dsize, rng, encrypt_for=(p % (2 * n)) if control else None)
    tsk = tensor_key(sk_out, key_b, k_ksk, dnum_ksk, dsize, rng)
    msg = np.where(rng.random(n) < 0.5, -1, 1).astype(np.int64)
    a = fs.ggsw_encrypt(sk_in, msg, in_b, k_in, dnum_in, 1, rng)
    bounds = [noise_ggsw_keyswitch(n, key_b * dsize, col, 0.5, 0.0, fs.SIGMA * fs.SIGMA, 0.0, rank, k_in, k_ksk, k_ksk) + 0.5
              for col in range(rank + 1)]
    return SimpleNamespace(op=op, n=n, rank=rank, dsize=dsize, in_b=in_b, key_b=key_b, a=a, key=key, tsk=tsk, p=p, sk_out=sk_out,
                           want_msg=msg if op == "ks" else fs.automorphism(msg, p), res_size=fs.limbs_for(k_ksk, in_b), bounds=bounds,
                           dnum_in=dnum_in)


def ggsw_run_oracle(ref, c):
    pm, pts = prepare(ref, c.key), [prepare(ref, t) for t in c.tsk]
    if c.op == "ks":
        return ggsw_keyswitch(ref, c.a, c.in_b, pm, c.dsize, c.key_b, pts, c.res_size)
    return ggsw_automorphism(ref, c.a, c.in_b, pm, c.dsize, c.key_b, c.p, pts, c.dnum_in, c.res_size)


def ggsw_noise(c, out):
    """GGSW::noise (noise/ggsw.rs:62-103) of every entry: (noise, bound of its column)."""
    have = []
    for row in range(out.shape[0]):
        for col in range(c.rank + 1):
            pt = fs._row_plaintext(c.want_msg, c.res_size, row, c.in_b)
            if col > 0:
                pt = fs.normalize(fs.mul_small(pt, c.sk_out[col - 1]), c.in_b)
            have.append((fs.noise_log2(out[row, col], c.in_b, c.sk_out, pt, c.in_b), c.bounds[col]))
    return have


def ggsw_check(label, c, out, fail=False):
    have = ggsw_noise(c, out)
    worst = max(h - b for h, b in have)
    print(f"[noise] {label}: worst noise_have - noise_want {worst:.2f} (best {min(h - b for h, b in have):.2f})")
    if fail:
        assert min(h - b for h, b in have) > 0, (label, have, "a negative control met the bound")
    else:
        assert worst <= 0, (label, have)
