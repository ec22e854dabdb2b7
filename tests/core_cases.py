"""Cases for the encrypt / operate / decrypt tests (tests/ only): poulpy-core's core_backend_test_suite! procedures
(poulpy-core/src/test_suite/mod.rs:26-88) as case builders, their negative controls, and the oracle runner and noise check that
tests/test_core_semantics.py (oracle) and tests/test_gpu_core_semantics.py (device) share.  The builders call neither the oracle nor the
device: keys and ciphertexts come from tests/fhe_sk.py, and each case carries what every output must decrypt to and the reference's bound.

The other families built the same way: tests/key_ops_cases.py (automorphism-key composition, the GGSW forms), tests/tensor_cases.py
(tensoring, relinearization, the one-call multiply, the plaintext and constant products), tests/trace_cases.py (trace, packing) and
tests/lwe_cases.py (LWE key switch, LWE <-> GLWE conversion, blind rotation, the gate bootstrap chain, circuit bootstrapping)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import fhe_sk as fs
from tests.helpers import seeded

N = 256
BASE2K = 17     # poulpy-cpu-ref/src/tests.rs:154-158
P_AUTO = -5     # automorphism/glwe_ct.rs:41
AUTO_MODES = ("automorphism", "add", "sub", "sub_negate")


# ---- case builders: encrypted inputs, the key, what every output must decrypt to, the bound ----
def _monomial(n, k):
    m = np.zeros(n, dtype=np.int64)
    m[k] = 1
    return m


def external_product_case(n, rank, dsize, dnum, in_base2k, key_base2k, out_base2k, k_in, k_ggsw, k_out, bound_base2k, batch, seed,
                          limb_shift=0, want_rot=1):
    """external_product/glwe_ct.rs:33-158: GGSW(X^1), GLWE(pt) with pt uniform and pt[0][1] = 1; the output decrypts to X pt.
    want_rot != 1 (a negative control) expects another rotation."""
    rng = seeded(seed)
    sk = fs.ternary_secret(n, rank, rng)
    key = fs.ggsw_encrypt(sk, _monomial(n, 1), key_base2k, k_ggsw, dnum, dsize, rng, limb_shift=limb_shift)
    a_size = fs.limbs_for(k_in, in_base2k)
    cts, wants = [], []
    for _ in range(batch):
        pt = fs.uniform_digits((a_size, n), in_base2k, rng)
        pt[0, 1] = 1
        cts.append(fs.glwe_encrypt(sk, pt, in_base2k, k_in, rng))
        wants.append(fs.rotate(pt, want_rot))
    return SimpleNamespace(op="ep", n=n, rank=rank, rank_out=rank, dsize=dsize, key=key, key_base2k=key_base2k, a=np.stack(cts),
                           a_base2k=in_base2k, res_size=fs.limbs_for(k_out, out_base2k), res_base2k=out_base2k, sk_out=sk, want=wants,
                           bound=fs.external_product_bound(n, bound_base2k, rank, k_in, k_ggsw))


def keyswitch_case(n, rank_in, rank_out, dsize, dnum, in_base2k, key_base2k, out_base2k, k_in, k_ksk, k_out, batch, seed, swap=False,
                   limb_shift=0):
    """keyswitch/glwe_ct.rs:33-160: the switching key of sk_in under sk_out; the output decrypts under sk_out to pt.  swap exchanges
    the key's two input columns (a negative control)."""
    rng = seeded(seed)
    sk_in = fs.ternary_secret(n, rank_in, rng)
    sk_out = fs.ternary_secret(n, rank_out, rng)
    key = fs.switching_key(sk_in, sk_out, key_base2k, k_ksk, dnum, dsize, rng, limb_shift=limb_shift)
    if swap:
        key = np.ascontiguousarray(key[:, ::-1])
    a_size = fs.limbs_for(k_in, in_base2k)
    cts, wants = [], []
    for _ in range(batch):
        pt = fs.uniform_digits((a_size, n), in_base2k, rng)
        cts.append(fs.glwe_encrypt(sk_in, pt, in_base2k, k_in, rng))
        wants.append(pt)
    return SimpleNamespace(op="ks", n=n, rank=rank_in, rank_out=rank_out, dsize=dsize, key=key, key_base2k=key_base2k, a=np.stack(cts),
                           a_base2k=in_base2k, res_size=fs.limbs_for(k_out, out_base2k), res_base2k=out_base2k, sk_out=sk_out, want=wants,
                           bound=fs.keyswitch_bound(n, k_ksk, dnum, dsize, key_base2k, rank_in))


def automorphism_case(n, rank, dsize, dnum, in_base2k, key_base2k, out_base2k, k_in, k_ksk, k_out, bound_dsize, batch, seed, mode="automorphism",
                      p=P_AUTO, encrypt_for=None, want_mode=None):
    """automorphism/glwe_ct.rs:35-151: the automorphism key of p; the output decrypts to phi_p(pt).  The device-only forms by linearity
    (automorphism/glwe_ct.rs:96-357 on the reference's side): add -> pt + phi_p(pt), sub -> phi_p(pt) - pt, sub_negate -> pt - phi_p(pt),
    whose output noise is phi_p(e_ks + e_in) +- e_in: the input's noise (sigma at 2^-k_in) enters twice, so its variance is counted twice on top
    of the key switch's bound (the reference's bound for the plain form counts it in neither place).  want_mode (a negative control) expects
    another form."""
    rng = seeded(seed)
    sk = fs.ternary_secret(n, rank, rng)
    key = fs.automorphism_key(sk, p, key_base2k, k_ksk, dnum, dsize, rng, encrypt_for=encrypt_for)
    a_size = fs.limbs_for(k_in, in_base2k)
    wm = want_mode or mode
    cts, wants = [], []
    for _ in range(batch):
        pt = fs.uniform_digits((a_size, n), in_base2k, rng)
        cts.append(fs.glwe_encrypt(sk, pt, in_base2k, k_in, rng))
        f = fs.automorphism(pt, p)
        wants.append({"automorphism": f, "add": pt + f, "sub": f - pt, "sub_negate": pt - f}[wm])
    bound = fs.keyswitch_bound(n, k_ksk, dnum, bound_dsize, key_base2k, rank)
    if mode != "automorphism":
        bound = 0.5 * math.log2(4.0 ** (bound - 1.0) + 2.0 * (fs.SIGMA * 2.0 ** -k_in) ** 2) + 1.0
    return SimpleNamespace(op="auto", mode=mode, p=p, n=n, rank=rank, rank_out=rank, dsize=dsize, key=key, key_base2k=key_base2k,
                           a=np.stack(cts), a_base2k=in_base2k, res_size=fs.limbs_for(k_out, out_base2k), res_base2k=out_base2k, sk_out=sk,
                           want=wants, bound=bound)


def reference_cases(kind, batch, base2k=BASE2K, n=N):
    """The parameter loops of the reference tests, as (label, case, in_place)."""
    seed = 0
    if kind in ("ep", "ks", "auto"):
        in_b, key_b, out_b = base2k - 1, base2k, base2k - 2
        k_in = 4 * in_b + 1
        max_dsize = -(-k_in // key_b)
        for rank in (1, 2):
            for dsize in range(1, max_dsize + 1):
                k_key = k_in + key_b * dsize
                seed += 1
                if kind == "ep":
                    dnum = -(-k_in // (k_key * dsize))          # external_product/glwe_ct.rs:45
                    yield ((kind, rank, dsize), external_product_case(n, rank, dsize, dnum, in_b, key_b, out_b, k_in, k_key, k_key,
                                                                      key_b * max_dsize, batch, seed), False)
                elif kind == "ks":
                    for rank_out in (1, 2):
                        yield ((kind, rank, rank_out, dsize), keyswitch_case(n, rank, rank_out, dsize, -(-k_in // (key_b * dsize)), in_b, key_b,
                                                                             out_b, k_in, k_key, k_key, batch, seed + 100 * rank_out), False)
                else:
                    for mode in AUTO_MODES:
                        yield ((kind, mode, rank, dsize), automorphism_case(n, rank, dsize, -(-k_in // (key_b * dsize)), in_b, key_b, out_b,
                                                                            k_in, k_key, k_key, max_dsize, batch, seed, mode=mode), False)
    else:   # the assign forms: one base for the ciphertext, res = a
        out_b, key_b = base2k - 1, base2k
        k_out = 4 * out_b + 1
        max_dsize = -(-k_out // key_b)
        for rank in (1, 2):
            for dsize in range(1, max_dsize + 1):
                k_key = k_out + key_b * dsize
                seed += 1
                if kind == "ep_assign":
                    dnum = -(-k_out // (out_b * max_dsize))     # external_product/glwe_ct.rs:188
                    yield ((kind, rank, dsize), external_product_case(n, rank, dsize, dnum, out_b, key_b, out_b, k_out, k_key, k_out,
                                                                      key_b * max_dsize, batch, seed), True)
                elif kind == "ks_assign":
                    yield ((kind, rank, dsize), keyswitch_case(n, rank, rank, dsize, -(-k_out // (key_b * dsize)), out_b, key_b, out_b,
                                                               k_out, k_key, k_out, batch, seed), True)
                else:
                    yield ((kind, rank, dsize), automorphism_case(n, rank, dsize, -(-k_out // (key_b * dsize)), out_b, key_b, out_b, k_out,
                                                                  k_key, k_out, dsize, batch, seed), True)


def control_cases(batch, n=N, base2k=BASE2K):
    """One negative control per convention, each through the procedure of its operation (label, case, in_place)."""
    in_b, key_b, out_b = base2k - 1, base2k, base2k - 2
    k_in = 4 * in_b + 1
    k_key = k_in + key_b
    dnum = -(-k_in // key_b)
    yield ("GGSW messages one limb off", external_product_case(n, 1, 1, 1, in_b, key_b, out_b, k_in, k_key, k_key, key_b * 4, batch, 501,
                                                                limb_shift=1), False)
    yield ("rotation the other way", external_product_case(n, 1, 1, 1, in_b, key_b, out_b, k_in, k_key, k_key, key_b * 4, batch, 502,
                                                            want_rot=-1), False)
    yield ("GGLWE messages one limb off", keyswitch_case(n, 1, 1, 1, dnum, in_b, key_b, out_b, k_in, k_key, k_key, batch, 503,
                                                         limb_shift=1), False)
    yield ("rank-2 switching key, input columns swapped", keyswitch_case(n, 2, 1, 1, dnum, in_b, key_b, out_b, k_in, k_key, k_key, batch,
                                                                         504, swap=True), False)
    yield ("automorphism key for p, not p^-1", automorphism_case(n, 1, 1, dnum, in_b, key_b, out_b, k_in, k_key, k_key, 1, batch, 505,
                                                                 encrypt_for=P_AUTO % (2 * n)), False)
    yield ("sub read as sub_negate", automorphism_case(n, 1, 1, dnum, in_b, key_b, out_b, k_in, k_key, k_key, 1, batch, 506, mode="sub",
                                                       want_mode="sub_negate"), False)


# ---- running and checking ----
def prepare(mod, key):
    rows, cols_in, size, cols_out, n = key.shape
    pm = mod.vmp_pmat_alloc(rows, cols_in, cols_out, size)
    mod.vmp_prepare(pm, MatZnx(n, rows, cols_in, cols_out, size, np.ascontiguousarray(key)))
    return pm


def run_oracle(ref, c):
    rows, cols_in, ksz, cols_out, n = c.key.shape
    pm = prepare(ref, c.key)
    out = np.empty((len(c.a), c.res_size, cols_out, n), dtype=np.int64)
    for b, ct in enumerate(c.a):
        a = VecZnx(n, ct.shape[1], ct.shape[0], np.ascontiguousarray(ct))
        res = VecZnx(n, cols_out, c.res_size)
        if c.op == "ep":
            ref.glwe_external_product(res, c.res_base2k, a, c.a_base2k, pm, c.dsize, c.key_base2k)
        elif c.op == "ks":
            ref.glwe_keyswitch(res, c.res_base2k, a, c.a_base2k, pm, c.dsize, c.key_base2k)
        else:
            ref.glwe_automorphism(res, c.res_base2k, a, c.a_base2k, pm, c.dsize, c.key_base2k, c.p % (2 * n), c.mode)
        out[b] = res.data
    return out


def check(label, c, out, fail=False):
    """Every output against its own plaintext: the worst noise within the bound, or (a control) the best one beyond it."""
    have = [fs.noise_log2(out[b], c.res_base2k, c.sk_out, c.want[b], c.a_base2k) for b in range(len(out))]
    print(f"[noise] {label}: noise_have {max(have):.2f} (min {min(have):.2f}) noise_want {c.bound:.2f}")
    if fail:
        assert min(have) > c.bound, (label, have, c.bound, "a negative control met the bound")
    else:
        assert max(have) <= c.bound, (label, have, c.bound)
    return have
